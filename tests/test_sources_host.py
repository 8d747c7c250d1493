"""CPU: csrc/SOURCES names every file the library is built from.  build.sh compiles and hashes that list and _lib.build() watches it, so a
file outside it is outside the hash in rover_version() and outside the staleness check: an edit to it would silently run the old library."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaac_rover_2.0_amd", "csrc")
INCLUDE = re.compile(r'^\s*#\s*include\s*"([^"]+)"', re.M)


def _listed():
    with open(os.path.join(CSRC, "SOURCES")) as f:
        return [os.path.normpath(os.path.join(CSRC, line.strip())) for line in f if line.strip()]


def test_every_source_file_is_listed():
    on_disk = {os.path.normpath(p) for ext in ("cpp", "hip", "h") for p in glob.glob(os.path.join(CSRC, "*." + ext))}
    assert on_disk, CSRC
    assert sorted(on_disk - set(_listed())) == []


def test_every_listed_file_exists():
    listed = _listed()
    assert len(listed) == len(set(listed))
    assert [p for p in listed if not os.path.isfile(p)] == []


def test_every_quoted_include_is_listed():
    listed = set(_listed())
    missing = []
    for path in sorted(listed):
        with open(path) as f:
            for name in INCLUDE.findall(f.read()):
                target = os.path.normpath(os.path.join(os.path.dirname(path), name))
                if target not in listed:
                    missing.append((os.path.relpath(path, ROOT), name))
    assert missing == []
