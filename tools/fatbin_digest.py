#!/usr/bin/env python3
"""SHA-256 and size of the device code (.hip_fatbin section) of every object of the kernel library and of libnsid_hip.so itself:
a check, without a GPU, that a host-side change left every device code object as it was. Builds nothing.

    python -m neuralsampleid_amd.build --force && python tools/fatbin_digest.py > branch.txt
    (the same in a checkout of the other commit AT THE SAME PATH)  > other.txt;  diff other.txt branch.txt

The same path, because hipcc derives the unique id it appends to the symbols of internal-linkage kernels from the path of the
source and from its command line (the object path included): two builds of one source at different paths differ in those names."""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuralsampleid_amd.build import LIB, OBJ_DIR, SOURCES  # noqa: E402

OBJCOPY = "/opt/rocm/lib/llvm/bin/llvm-objcopy"


def fatbin(path: str, tmp: str) -> bytes:
    out = os.path.join(tmp, "fatbin")
    r = subprocess.run([OBJCOPY, f"--dump-section=.hip_fatbin={out}", path, os.path.join(tmp, "null")], capture_output=True, text=True)
    if r.returncode != 0 and "section '.hip_fatbin' not found" in r.stderr:
        return b""                      # a source without a kernel (tuning.hip): 0 bytes
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    return open(out, "rb").read()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("obj_dir", nargs="?", default=OBJ_DIR, help="directory of the objects (default: the in-tree build's)")
    ap.add_argument("--lib", default=LIB, help="the linked library")
    a = ap.parse_args()
    paths = [(s, os.path.join(a.obj_dir, s.replace(".hip", ".o"))) for s in SOURCES] + [(os.path.basename(a.lib), a.lib)]
    with tempfile.TemporaryDirectory() as tmp:
        for name, path in paths:
            blob = fatbin(path, tmp)
            print(f"{hashlib.sha256(blob).hexdigest()}  {len(blob):8d}  {name}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
