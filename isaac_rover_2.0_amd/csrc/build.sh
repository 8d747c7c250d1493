#!/bin/bash
# Builds librover_step.so (HIP kernels + C ABI) for gfx950 next to this script.
# -ffp-contract=off: one IEEE rounding per operation, in the reference's evaluation order.
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
# SOURCES lists what the library is built from, one file per line: the .cpp / .hip files are compiled, and all of it is hashed.
# rover_version() carries that hash: bench.py compares it with the hash recorded next to the PMC counts in profiles/ (a profile of another
# binary is reported as stale); _lib.source_hash() computes the same value from the same list.
cd "$here"
mapfile -t SOURCES < SOURCES
SRC_HASH="$(cat "${SOURCES[@]}" | sha256sum | cut -c1-12)"
UNITS=()
for f in "${SOURCES[@]}"; do case "$f" in *.cpp|*.hip) UNITS+=("$here/$f");; esac; done
exec "$HIPCC" -DROVER_SRC_HASH="\"$SRC_HASH\"" --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -fvisibility=hidden \
  -Wall -Wno-unused-result ${ROVER_EXTRA_FLAGS:-} \
  -o "$here/librover_step.so" "${UNITS[@]}"
