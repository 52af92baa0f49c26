"""CPU: the host-side queries behind the kernel table -- NSID_DECLINED, nsid_debug_last_kernel and nsid_ws_layer (include/nsid.h).
The library loads without a GPU and none of these launches anything."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (Cin, Cout, groups) of csrc/wsgemm.hip NSID_WS_LAYERS, and neighbours that are no layer of it
WS_LAYERS = [(64, 64, 1), (32, 32, 4), (128, 64, 1), (64, 256, 1), (256, 64, 1), (128, 128, 1), (64, 64, 4), (256, 128, 1), (128, 128, 4)]
NO_LAYERS = [(64, 128, 1), (64, 64, 2), (256, 256, 1), (128, 128, 2), (0, 0, 1)]


@pytest.fixture(scope="module")
def L():
    from neuralsampleid_amd.build import build_lib
    build_lib(verbose=False)
    from neuralsampleid_amd import _lib
    return _lib


def test_declined_and_the_two_queries_are_declared(L):
    assert L.DEFINES["NSID_DECLINED"] == 1 and L.DEFINES["NSID_OK"] == 0
    assert "NSID_DECLINED" in L._ERR[1]
    assert L.PROTOTYPES["nsid_debug_last_kernel"] == ("c", "") and L.PROTOTYPES["nsid_ws_layer"] == ("i", "iii")


def test_ws_layer_table(L):
    assert [L.lib.nsid_ws_layer(*s) for s in WS_LAYERS] == [1] * 9
    assert [L.lib.nsid_ws_layer(*s) for s in NO_LAYERS] == [0] * 5
    # every (Cin, Cout, groups) over the table's own values: exactly the nine
    vals = sorted({v for s in WS_LAYERS for v in s[:2]})
    hits = {(ci, co, g) for ci in vals for co in vals for g in (1, 2, 4) if L.lib.nsid_ws_layer(ci, co, g) == 1}
    assert hits == set(WS_LAYERS)


def test_no_kernel_taken_in_a_fresh_process(L):
    """before any entry that chooses between kernels has run the library names none"""
    code = "from neuralsampleid_amd import _lib; import sys; sys.stdout.write(repr(_lib.lib.nsid_debug_last_kernel()))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "b''", (r.stdout, r.stderr[-400:])
