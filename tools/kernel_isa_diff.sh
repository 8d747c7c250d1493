#!/bin/bash
# Device code of two csrc trees, kernel by kernel (CPU only: no GPU is opened):
#   tools/kernel_isa_diff.sh OLD_CSRC NEW_CSRC [OUT_DIR]
# Every .hip file of a tree's SOURCES is compiled to its gfx950 code object with the flags of csrc/build.sh (and one fixed source-hash
# string for both trees).  Per kernel symbol the script writes the resource metadata of the code object's notes — VGPRs, AGPRs, SGPRs,
# both spill counts, LDS bytes, scratch bytes, kernarg size — and the disassembly without addresses and encodings, the kernels sorted
# by name whichever unit they come from, and diffs the two trees.  A move of kernels between files shows as no difference at all.
# Exit status: 0 the same kernels with the same metadata and instructions, 1 otherwise.  JOBS: compiles at a time (default 8).
set -euo pipefail
export LC_ALL=C
[ $# -ge 2 ] || { echo "usage: $0 OLD_CSRC NEW_CSRC [OUT_DIR]" >&2; exit 2; }
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
LLVM="${LLVM_BIN:-/opt/rocm/llvm/bin}"
out="${3:-$(mktemp -d)}"
mkdir -p "$out"

listing() {      # $1 = csrc tree, $2 = tag: -> $out/$2.txt, $out/$2.units (kernel name, unit)
    local src; src="$(cd "$1" && pwd)"
    local obj="$out/$2.obj"; mkdir -p "$obj"; : > "$out/$2.warnings"
    grep -E '\.hip$' "$src/SOURCES" | xargs -P "${JOBS:-8}" -I{} "$HIPCC" -DROVER_SRC_HASH='"isa-diff"' --offload-arch=gfx950 -O3 -std=c++17 \
        -ffp-contract=off -fPIC -fvisibility=hidden -Wall -Wno-unused-result ${ROVER_EXTRA_FLAGS:-} --cuda-device-only --no-gpu-bundle-output -c "$src/{}" -o "$obj/{}.o" 2>> "$out/$2.warnings"
    : > "$out/$2.meta"; : > "$out/$2.isa"; : > "$out/$2.units"
    for o in "$obj"/*.o; do
        # one line per kernel: name <TAB> metadata (the keys of a kernel's record sit four columns in; its arguments' deeper)
        "$LLVM/llvm-readelf" --notes "$o" | awk -v unit="$(basename "$o" .o)" -v units="$out/$2.units" '
            function flush() { if (name != "") { print name "\t" rec; print name "\t" unit >> units } name = ""; rec = "" }
            /^  - \./ { flush() }
            /^  [ -] \.name:/ { name = $NF }
            /^  [ -] \.(vgpr_count|agpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size|private_segment_fixed_size|kernarg_segment_size):/ {
                k = $(NF - 1); sub(/^\./, "", k); rec = rec " " k $NF }
            /^amdhsa\.(target|version)/ { flush() }
            END { flush() }' >> "$out/$2.meta"
        # where every function ends (symbol value + size, as the 12 hex digits the disassembly prints): what follows is padding up to
        # the next function's alignment, and depends on the neighbour
        "$LLVM/llvm-readelf" -sW "$o" | awk '$4 == "FUNC" { print $8, $2, $3 }' | sort -u | while read -r n v sz; do
            printf '%s\t%012X\n' "$n" $((16#$v + sz)); done > "$out/$2.ends"
        # one line per function symbol: name <TAB> instructions joined by \001
        "$LLVM/llvm-objdump" -d "$o" | awk -v ends="$out/$2.ends" '
            BEGIN { while ((getline l < ends) > 0) { split(l, f, "\t"); end[f[1]] = f[2] } }
            function flush() { if (name != "") print name "\t" body; name = ""; body = "" }
            /^[0-9a-f]+ <.*>:$/ { flush(); name = $0; sub(/^[0-9a-f]+ </, "", name); sub(/>:$/, "", name); next }
            name != "" && /\/\/ [0-9A-F]+:/ {          # (a line without an address holds no instruction: the "..." of a run of zeros)
                line = $0; addr = line; sub(/^.*\/\/ /, "", addr); sub(/:.*$/, "", addr)
                if ((name in end) && addr >= end[name]) next
                sub(/[ \t]*\/\/.*$/, "", line); sub(/^[ \t]+/, "", line); gsub(/[ \t]+/, " ", line); body = body "\001    " line }
            END { flush() }' >> "$out/$2.isa"
    done
    sort -o "$out/$2.meta" "$out/$2.meta"; sort -o "$out/$2.isa" "$out/$2.isa"; sort -o "$out/$2.units" "$out/$2.units"
    join -t $'\t' -a 2 "$out/$2.meta" "$out/$2.isa" | awk -F '\t' '
        NF == 3 { print "== kernel " $1; print "   " $2; print $3 }
        NF == 2 { print "== function " $1; print $2 }' | tr '\001' '\n' > "$out/$2.txt"
}

listing "$1" old
listing "$2" new
echo "kernels: old $(wc -l < "$out/old.meta"), new $(wc -l < "$out/new.meta"); listings in $out"
for t in old new; do echo "--- $t: kernels per unit"; cut -f2 "$out/$t.units" | sort | uniq -c; done
echo "--- kernel names in one tree only (< old, > new)"
diff <(cut -f1 "$out/old.meta") <(cut -f1 "$out/new.meta") && echo "(none)" || true
echo "--- resource metadata that differs"
diff "$out/old.meta" "$out/new.meta" && echo "(none)" || true
echo "--- kernels and functions whose listing differs, then the lines"
if diff -U0 -F '^== ' "$out/old.txt" "$out/new.txt" > "$out/diff.txt"; then echo "(none)"; exit 0; fi
grep '^@@' "$out/diff.txt" | sed 's/^@@.*@@ *//' | sort | uniq -c
cat "$out/diff.txt"
exit 1
