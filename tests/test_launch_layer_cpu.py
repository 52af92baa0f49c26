"""The launch layer's status rule (csrc/nsid_common.h) in a stand-alone host program, tests/launch_layer_main.hip: built with the
library's compiler and flags, run once. No device, nothing loaded into this process."""
import os
import subprocess

from neuralsampleid_amd.build import FLAGS, HIPCC

HERE = os.path.dirname(os.path.abspath(__file__))


def test_first_error_is_reported_and_cleared(tmp_path):
    exe = str(tmp_path / "launch_layer_main")
    src = os.path.join(HERE, "launch_layer_main.hip")
    # the host side alone where the compiler takes that; a plain compile otherwise
    r = subprocess.run([HIPCC, *FLAGS, "--offload-host-only", src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run([HIPCC, *FLAGS, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    first, second, other = run.stdout.splitlines()
    assert other.startswith("not: ") and len({first, second, other[5:]}) == 3
    # one line per failed entry, each with the FIRST error of that entry; the later error of the last entry appears nowhere
    assert run.stderr.splitlines() == [f"[nsid] kernel launch failed: {first}", f"[nsid] kernel launch failed: {second}"]
