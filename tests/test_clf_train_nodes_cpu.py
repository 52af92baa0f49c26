"""Classifier training on node matrices of up to 128 nodes, the parts that need no GPU: the multi-tile training entry points of the
kernel library and their bindings, their refusals (and the unchanged bound of the N <= 32 entries), downstream.clf_train_scores_n,
and the golden's rule inputs and its recorded reference error (tests/golden/clf_train_nodes.npz)."""
import ctypes
import os
import re

import numpy as np
import pytest

NEW_ENTRIES = {
    # name: (the documented argument types in include/nsid.h's order (p = pointer, i = int, s = stream), the entry whose argument
    # list it shares)
    "nsid_clf_attn_fwd_n": ("pipiiippippps", "nsid_clf_attn_fwd_c"),
    "nsid_clf_attn_bwd_n": ("pppipiiippipps", "nsid_clf_attn_bwd_c"),
    "nsid_clf_seg_reduce_n": ("ppppppiiiiipps", "nsid_clf_seg_reduce_c"),
}
NEW_COUNTERS = ("clf_attn_fwd_n", "clf_attn_bwd_n", "clf_seg_reduce_n")


@pytest.fixture(scope="module")
def libpath():
    from neuralsampleid_amd.build import build_lib
    return build_lib(verbose=False)


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "include", "nsid.h")).read()


def test_header_declares_and_documents_the_entries():
    h = _header()
    flat = re.sub(r"\s+", " ", h)
    assert ("int nsid_clf_attn_fwd_n(const float* q, int nq_seg, const float* kv, int nc_seg, int C, int N, const int* qi, "
            "const int* ci, int P, float* obar, float* attn, float* abar, void* stream);") in flat
    assert ("int nsid_clf_attn_bwd_n(const float* dobar, const float* attn, const float* q, int nq_seg, const float* kv, int nc_seg, "
            "int C, int N, const int* qi, const int* ci, int P, float* dq, float* dk, void* stream);") in flat
    assert ("int nsid_clf_seg_reduce_n(const float* dq, const float* dk, const float* abar, const float* dobar, const int* qi, "
            "const int* ci, int P, int C, int N, int nq_seg, int nc_seg, float* dq_seg, float* dkv_seg, void* stream);") in flat
    # the saved-attention layout, abar's stride and the limits
    assert "clf_attn_fwd_n, clf_attn_bwd_n, clf_seg_reduce_n:" in h
    assert "attn (P x 4 x nT x nT x 16 x 64)" in flat and "abar (P x 4 x 128)" in flat and "nT = ceil(N / 32)" in flat
    assert "#define NSID_CLF_MAX_N 32 " in flat and "#define NSID_CLF_MAX_N_EVAL 128 " in flat


def test_library_exports_and_bindings(libpath):
    from neuralsampleid_amd import _lib
    lib = ctypes.CDLL(libpath)
    ct = {"p": ctypes.c_void_p, "i": ctypes.c_int, "s": ctypes.c_void_p}
    for name, (sig, same_as) in NEW_ENTRIES.items():
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name] == sig == _lib.SIGNATURES[same_as], name
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == [ct[c] for c in sig] and fn.restype is ctypes.c_int, name
    assert set(NEW_COUNTERS) | {"clf_attn_fwd", "clf_attn_bwd", "clf_seg_reduce"} <= set(_lib.launch_counters())


def _calls(L, C, N, P, S):
    """the three entries with null pointers: P pairs, S segments per side for the reduce"""
    return (L.nsid_clf_attn_fwd_n(None, 1, None, 1, C, N, None, None, P, None, None, None, None),
            L.nsid_clf_attn_bwd_n(None, None, None, 1, None, 1, C, N, None, None, P, None, None, None),
            L.nsid_clf_seg_reduce_n(None, None, None, None, None, None, P, C, N, S, S, None, None, None))


def test_new_entries_refuse_without_a_gpu(libpath):
    """NSID_EINVAL comes before any pointer is read or anything is launched, and an empty call is NSID_OK with nothing launched:
    callable with null pointers on a machine without a GPU"""
    from neuralsampleid_amd import _lib
    L = _lib.lib
    _lib.launch_counters(reset=True)
    for C in (512, 640, 768, 1024):
        for N in (128, 33, 1):
            assert _calls(L, C, N, 0, 0) == (0, 0, 0), (C, N)                     # P = 0, no segments
    for C, N in [(512, 129), (512, 0), (576, 128), (1024, 129), (512, -1), (256, 64), (2048, 64), (0, 64), (576, 32)]:
        assert _calls(L, C, N, 0, 0) == (-1, -1, -1), (C, N)
        assert _calls(L, C, N, 1, 1) == (-1, -1, -1), (C, N)
    # a good shape with null pointers, and misaligned pointers, are refused as well
    for C, N in ((512, 128), (640, 33), (768, 70), (1024, 1)):
        assert _calls(L, C, N, 1, 1) == (-1, -1, -1), (C, N)
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    for qa, ka in ((a + 4, a), (a, a + 8)):
        assert L.nsid_clf_attn_fwd_n(qa, 1, ka, 1, 512, 128, a, a, 1, a, a, a, None) == -1
    for da, ka in ((a + 4, a), (a, a + 8)):
        assert L.nsid_clf_attn_bwd_n(da, a, a, 1, ka, 1, 512, 128, a, a, 1, a, a, None) == -1
    for bad in range(5):
        ptr = [a + 4 if i == bad else a for i in range(5)]                        # dq, dk, dobar, dq_seg, dkv_seg
        assert L.nsid_clf_seg_reduce_n(ptr[0], ptr[1], a, ptr[2], a, a, 1, 512, 128, 1, 1, ptr[3], ptr[4], None) == -1, bad
    c = _lib.launch_counters()
    assert all(c[k] == 0 for k in NEW_COUNTERS) and sum(c.values()) == 0, {k: v for k, v in c.items() if v}


def test_old_entries_keep_their_bound(libpath):
    from neuralsampleid_amd import _lib, ops
    L = _lib.lib
    _lib.launch_counters(reset=True)
    assert L.nsid_clf_attn_fwd_c(None, 1, None, 1, 512, 33, None, None, 0, None, None, None, None) == -1
    assert L.nsid_clf_attn_bwd_c(None, None, None, 1, None, 1, 512, 33, None, None, 0, None, None, None) == -1
    assert L.nsid_clf_seg_reduce_c(None, None, None, None, None, None, 0, 512, 33, 0, 0, None, None, None) == -1
    assert L.nsid_clf_attn_fwd(None, 1, None, 1, 33, None, None, 0, None, None, None, None) == -1
    assert sum(_lib.launch_counters().values()) == 0
    assert ops.CLF_MAX_N == 32 and ops.CLF_MAX_N_EVAL == 128
    for name in ("clf_attn_fwd_n", "clf_attn_bwd_n", "clf_seg_reduce_n"):
        assert callable(getattr(ops, name))


def test_downstream_exports_the_entry():
    from neuralsampleid_amd import downstream
    assert callable(downstream.clf_train_scores_n) and "clf_train_scores_n" in downstream.__all__
    assert "clf_train_scores" in downstream.__all__
    assert "128" in downstream.clf_train_scores_n.__doc__


@pytest.fixture(scope="module")
def golden():
    from make_clf_train_nodes_golden import load_golden_inputs
    return load_golden_inputs()                          # asserts the stored digests


def test_golden_rule_inputs_regenerate(golden):
    from make_clf_train_golden import PARAM_NAMES
    z, cases = golden
    assert sorted(cases) == ["n128", "n70"]
    for case, (C, B, N, nodes, nsteps) in {"n128": (512, 8, 128, 128, 3), "n70": (1024, 4, 70, 100, 1)}.items():
        p, steps, state = cases[case]
        assert (p["C"], p["B"], p["N"], p["num_nodes"], p["steps"], p["k"]) == (C, B, N, nodes, nsteps, 3)
        assert len(steps) == nsteps and steps[0]["nodes_i"].shape == (B, C, N) and steps[0]["nodes_i"].dtype == np.float32
        assert state["positional_embedding"].shape == (1, nodes, C) and state["attn.in_proj_weight"].shape == (3 * C, C)
        P = 4 * B
        assert z[f"{case}/hn"].shape == (nsteps, B, 3) and z[f"{case}/keep_bits"].shape == (nsteps, P, 16)
        s = z[f"{case}/scores"]
        assert s.shape == (nsteps, P) and s.dtype == np.float32 and 0.02 < s.min() and s.max() < 0.98 and s.std() > 1e-3
        assert z[f"{case}/losses"].shape == (nsteps,) and abs(float(z[f"{case}/mean_loss"]) - z[f"{case}/losses"].mean()) < 1e-6
        for n in PARAM_NAMES:
            for kind in ("grad0", "final"):
                assert z[f"{case}/{kind}/{n}/samples"].size == min(1024, state[n].numel()), (case, kind, n)
                assert float(z[f"{case}/{kind}/{n}/l2"][0]) > 0
        # a candidate that serves two or more pairs of a step
        cand = np.concatenate([np.arange(B) + B, z[f"{case}/hn"][0].reshape(-1)])
        assert np.bincount(cand).max() >= 2


def test_reference_fp32_error_leaves_the_margin(golden):
    """the GPU tests' bounds are 1e-5 against fp64 (scores absolute, gradients relative L2); the reference module's own fp32 on the
    golden's inputs stays below 1e-6 on the scores and 2e-6 on every gradient. The generator measured 1.7e-7 / 8.2e-7 (n128) and
    8.0e-8 / 7.9e-7 (n70), the worst gradient being attn.in_proj_weight in both."""
    z = golden[0]
    for case in ("n128", "n70"):
        assert 0 < float(z[f"{case}/dev_scores"]) <= 1e-6, case
        assert 0 < float(z[f"{case}/dev_grads"]) <= 2e-6, case


def test_fixture_is_small():
    from make_clf_train_nodes_golden import FIXTURE
    assert os.path.getsize(FIXTURE) < 1024 * 1024
