"""Classifier re-rank for node matrices of up to 128 nodes, the parts that need no GPU: the wide-N entry points of the kernel
library and their bindings, their refusals (and the unchanged bound of the N <= 32 entries), the num_nodes inference of the re-rank
command line, reference-layout state_dicts with 100 and 128 nodes, and the golden's rule inputs and its recorded reference error
(tests/golden/clf_nodes.npz)."""
import ctypes
import re

import numpy as np
import pytest
import torch

NEW_ENTRIES = {
    # name: (the documented argument types in include/nsid.h's order (p = pointer, i = int, l = int64, s = stream), the entry whose
    # argument list it shares)
    "nsid_clf_node_rows_n": ("piiipps", "nsid_clf_node_rows"),
    "nsid_clf_pair_scores_n": ("pipiiipppiipppls", "nsid_clf_pair_scores_c"),
}


@pytest.fixture(scope="module")
def libpath():
    from neuralsampleid_amd.build import build_lib
    return build_lib(verbose=False)


def _header():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "include", "nsid.h")).read()


def test_header_declares_and_documents_the_entries():
    h = _header()
    flat = re.sub(r"\s+", " ", h)
    assert ("int nsid_clf_node_rows_n(const float* x, int S, int C, int N, const float* pos, float* rows, void* stream);") in flat
    assert ("int nsid_clf_pair_scores_n(const float* q, int nq_seg, const float* kp, int nc_seg, int C, int N, const int* groups, "
            "const int64_t* out_off, const int* tile_off, int ngroups, int ntiles, const int* cidx, const float* tail, float* out, "
            "int64_t out_len, void* stream);") in flat
    assert "clf_node_rows_n, clf_pair_scores_n:" in h and "1 <= N <= 128" in h


def test_library_exports_and_bindings(libpath):
    from neuralsampleid_amd import _lib
    lib = ctypes.CDLL(libpath)
    ct = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_long, "s": ctypes.c_void_p}
    for name, (sig, same_as) in NEW_ENTRIES.items():
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name] == sig == _lib.SIGNATURES[same_as], name
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == [ct[c] for c in sig] and fn.restype is ctypes.c_int, name
    assert {"clf_node_rows_n", "clf_pair_scores_n", "clf_node_rows", "clf_pair_scores"} <= set(_lib.launch_counters())


def test_new_entries_refuse_without_a_gpu(libpath):
    """NSID_EINVAL comes before any pointer is read or anything is launched: callable with null pointers on a machine without a GPU"""
    from neuralsampleid_amd import _lib
    L = _lib.lib
    _lib.launch_counters(reset=True)
    bad = [(512, 0), (512, 129), (512, -1), (1024, 129), (576, 128), (256, 128), (2048, 128), (576, 32), (0, 64)]
    for C, N in bad:
        assert L.nsid_clf_node_rows_n(None, 1, C, N, None, None, None) == -1, (C, N)
        assert L.nsid_clf_pair_scores_n(None, 1, None, 1, C, N, None, None, None, 1, 1, None, None, None, 1, None) == -1, (C, N)
    # a good shape with null pointers, and misaligned q / kp, are refused as well
    for C, N in ((512, 128), (640, 33), (768, 70), (1024, 1)):
        assert L.nsid_clf_node_rows_n(None, 1, C, N, None, None, None) == -1, (C, N)
        assert L.nsid_clf_pair_scores_n(None, 1, None, 1, C, N, None, None, None, 1, 1, None, None, None, 1, None) == -1, (C, N)
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    for qa, ka in ((a + 4, a), (a, a + 8)):
        assert L.nsid_clf_pair_scores_n(qa, 1, ka, 1, 512, 128, a, a, a, 1, 1, a, a, a, 1, None) == -1
    c = _lib.launch_counters()
    assert c["clf_node_rows_n"] == 0 and c["clf_pair_scores_n"] == 0 and sum(c.values()) == 0, {k: v for k, v in c.items() if v}


def test_old_entries_keep_their_bound(libpath):
    from neuralsampleid_amd import _lib, ops
    L = _lib.lib
    _lib.launch_counters(reset=True)
    assert L.nsid_clf_pair_scores_c(None, 1, None, 1, 768, 33, None, None, None, 1, 1, None, None, None, 1, None) == -1
    assert L.nsid_clf_pair_scores(None, 1, None, 1, 33, None, None, None, 1, 1, None, None, None, 1, None) == -1
    assert L.nsid_clf_node_rows(None, 1, 768, 33, None, None, None) == -1
    assert sum(_lib.launch_counters().values()) == 0
    assert ops.CLF_MAX_N == 32 and ops.CLF_MAX_N_EVAL == 128


def rule_state(num_nodes, C=512, pos_embed=True):
    from make_rerank_golden import classifier_state
    state = classifier_state(5, 0.125, {"C": C, "num_nodes": num_nodes})
    if not pos_embed:
        del state["positional_embedding"]
    return state


def test_checkpoint_num_nodes():
    from neuralsampleid_amd.rerank import checkpoint_num_nodes
    for n in (32, 100, 128):
        assert checkpoint_num_nodes(rule_state(n)) == (n, True)
    assert checkpoint_num_nodes(rule_state(100, C=1024)) == (100, True)
    nn_, pos = checkpoint_num_nodes(rule_state(128, pos_embed=False))
    assert pos is False
    with pytest.raises(ValueError):
        checkpoint_num_nodes({"positional_embedding": torch.zeros(128, 512)})


@pytest.mark.parametrize("num_nodes", [32, 100, 128])
def test_state_dicts_load_strict_through_the_helper(num_nodes):
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    from neuralsampleid_amd.rerank import checkpoint_in_dim, checkpoint_num_nodes
    state = rule_state(num_nodes)
    clf = CrossAttentionClassifier(512, num_nodes=128) if num_nodes == 128 else (
        CrossAttentionClassifier(512) if num_nodes == 100 else CrossAttentionClassifier(512, num_nodes=32))
    clf.load_state_dict(state, strict=True)
    assert clf.positional_embedding.shape == (1, num_nodes, 512)
    # as the command line builds it
    n, pos = checkpoint_num_nodes(state)
    built = CrossAttentionClassifier(in_dim=checkpoint_in_dim(state), num_nodes=n, pos_embed=pos)
    built.load_state_dict(state, strict=True)
    assert sorted(built.state_dict()) == sorted(state)
    built._check_module()


def test_state_dict_without_positional_embedding_loads_through_the_helper():
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    from neuralsampleid_amd.rerank import checkpoint_in_dim, checkpoint_num_nodes
    state = rule_state(128, C=768, pos_embed=False)
    n, pos = checkpoint_num_nodes(state)
    built = CrossAttentionClassifier(in_dim=checkpoint_in_dim(state), num_nodes=n, pos_embed=pos)
    built.load_state_dict(state, strict=True)
    assert "positional_embedding" not in built.state_dict()


@pytest.fixture(scope="module")
def golden():
    from make_clf_nodes_golden import load_golden_inputs
    return load_golden_inputs()                          # asserts the stored digests


def test_golden_rule_inputs_regenerate(golden):
    z, cases, (p, inp, state) = golden
    assert sorted(cases) == [(512, "n128"), (512, "n70"), (1024, "n128"), (1024, "n70")]
    for (C, case), (cp, nm, st) in cases.items():
        N, nodes, Sq, Sc = (128, 128, 5, 4) if case == "n128" else (70, 100, 3, 2)
        assert cp["C"] == C and cp["N"] == N and cp["num_nodes"] == nodes
        assert nm[0].shape == (Sq, C, N) and nm[1].shape == (Sc, C, N) and nm[0].dtype == np.float32
        assert st["positional_embedding"].shape == (1, nodes, C) and st["attn.in_proj_weight"].shape == (3 * C, C)
        s = z[f"{C}/{case}/scores"]
        assert s.shape == (Sq, Sc) and s.dtype == np.float32 and 0.02 < s.min() and s.max() < 0.98 and s.std() > 1e-3
    assert p["C"] == 512 and p["N"] == 128 and p["num_nodes"] == 128
    assert all(a.shape[1:] == (512, 128) for a in inp["ref_nm"].values())
    assert state["positional_embedding"].shape == (1, 128, 512)
    L = len(p["test_seq_len"].split())
    assert z["eval/hit_rates"].shape == (3, L) and z["eval/raw_score"].shape[1] == 3 * L and 0 < float(z["eval/map_score"]) < 1


def test_reference_fp32_error_leaves_the_margin(golden):
    """the GPU tests' bound is 1e-5 against fp64; the reference module's own fp32 on the golden's inputs stays 10x below it"""
    z = golden[0]
    devs = [float(z[f"{C}/{case}/dev"]) for C in (512, 1024) for case in ("n128", "n70")]
    assert float(z["ref_fp32_vs_fp64"]) == max(devs)
    assert 0 < max(devs) <= 1e-6, devs


def test_fixture_is_small():
    import os
    from make_clf_nodes_golden import FIXTURE
    assert os.path.getsize(FIXTURE) < 100 * 1024
