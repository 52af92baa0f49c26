"""Stage-2 classifier at in_dim 640, 768 and 1024, the parts that need no GPU: the width-carrying entry points of the kernel library
and their bindings, the golden's rule inputs (tests/golden/clf_wide.npz), reference-layout state_dicts at every width, and the
checkpoint-width inference of the re-rank command line."""
import ctypes

import numpy as np
import pytest
import torch

WIDTHS = (512, 640, 768, 1024)
NEW_ENTRIES = {
    # name: the documented argument types, in include/nsid.h's order (p = pointer, i = int, l = int64, s = stream)
    "nsid_clf_pair_scores_c": "pipiiipppiipppls",
    "nsid_clf_attn_fwd_c": "pipiiippippps",
    "nsid_clf_attn_bwd_c": "pppipiiippipps",
    "nsid_clf_seg_reduce_c": "ppppppiiiiipps",
}


@pytest.fixture(scope="module")
def libpath():
    from neuralsampleid_amd.build import build_lib
    return build_lib(verbose=False)


def test_library_exports_width_entries(libpath):
    lib = ctypes.CDLL(libpath)
    missing = [n for n in NEW_ENTRIES if not hasattr(lib, n)]
    assert not missing, missing


def test_bindings_have_documented_types(libpath):
    from neuralsampleid_amd import _lib
    ct = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_long, "s": ctypes.c_void_p}
    for name, sig in NEW_ENTRIES.items():
        assert _lib.SIGNATURES[name] == sig, name
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == [ct[c] for c in sig] and fn.restype is ctypes.c_int, name
        # one int more than the C = 512 entry it generalises, right before N
        old = _lib.SIGNATURES[name[:-2]]
        assert any(sig[:j] + sig[j + 1:] == old and sig[j] == "i" for j in range(len(sig))), name


def test_entries_refuse_other_widths_without_a_gpu(libpath):
    """NSID_EINVAL comes before any pointer is read or anything is launched: callable with null pointers on a machine without a GPU"""
    from neuralsampleid_amd import _lib
    L = _lib.lib
    for C, N in ((576, 32), (256, 32), (0, 32), (2048, 32), (768, 33), (768, 0)):
        assert L.nsid_clf_pair_scores_c(None, 1, None, 1, C, N, None, None, None, 1, 1, None, None, None, 1, None) == -1, (C, N)
        assert L.nsid_clf_attn_fwd_c(None, 1, None, 1, C, N, None, None, 1, None, None, None, None) == -1, (C, N)
        assert L.nsid_clf_attn_bwd_c(None, None, None, 1, None, 1, C, N, None, None, 1, None, None, None) == -1, (C, N)
        assert L.nsid_clf_seg_reduce_c(None, None, None, None, None, None, 1, C, N, 1, 1, None, None, None) == -1, (C, N)
    assert _lib.launch_counters().get("clf_pair_scores", 0) == 0


def test_golden_rule_inputs_regenerate():
    from make_clf_wide_golden import load_golden_inputs
    z, cases = load_golden_inputs()                      # asserts the stored digests
    assert sorted(cases) == [640, 768, 1024]
    for C, (p, ev, steps, state) in cases.items():
        assert p["C"] == C and p["B"] == 4 and p["k"] == 3
        assert ev[0].shape == (5, C, 32) and ev[1].shape == (4, C, 32) and ev[2].shape[2] == ev[3].shape[2] == 7
        assert z[f"{C}/eval_scores"].shape == (5, 4) and z[f"{C}/scores"].shape == (16,) and z[f"{C}/hn"].shape == (4, 3)
        assert steps[0]["nodes_i"].shape == (4, C, 32) and state["attn.in_proj_weight"].shape == (3 * C, C)
        assert z[f"{C}/grad0/attn.in_proj_weight/rows"].shape == (3 * C,)


@pytest.mark.parametrize("C", WIDTHS)
def test_reference_state_dict_loads_strict(C):
    from make_rerank_golden import classifier_state
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    state = classifier_state(3, 0.25, {"C": C, "num_nodes": 32})
    clf = CrossAttentionClassifier(C, num_nodes=32)
    clf.load_state_dict(state, strict=True)
    assert sorted(clf.state_dict()) == sorted(state)
    clf._check_module()                                   # the width is accepted
    assert clf.attn.head_dim == C // 4


@pytest.mark.parametrize("kw", [{"in_dim": 576}, {"in_dim": 256}, {"in_dim": 768, "num_heads": 8}, {"in_dim": 640, "hidden_dim": 64}])
def test_other_configurations_stay_refused(kw):
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    with pytest.raises(NotImplementedError):
        CrossAttentionClassifier(num_nodes=32, **kw)._check_module()


def test_checkpoint_width_inference():
    from make_rerank_golden import classifier_state
    from neuralsampleid_amd.rerank import checkpoint_in_dim
    for C in WIDTHS:
        assert checkpoint_in_dim(classifier_state(0, 0.0, {"C": C, "num_nodes": 32})) == C
    state = classifier_state(0, 0.0, {"C": 768, "num_nodes": 32})
    del state["positional_embedding"]                     # a pos_embed=False checkpoint
    assert checkpoint_in_dim(state) == 768
    with pytest.raises(ValueError):
        checkpoint_in_dim({"fc.0.weight": torch.zeros(128, 768)})
    with pytest.raises(ValueError):
        checkpoint_in_dim({"attn.in_proj_weight": torch.zeros(768, 768)})


def test_node_matrix_width_must_match_the_classifier():
    from neuralsampleid_amd.rerank import _check_nm
    assert _check_nm(np.zeros((3, 768, 32), np.float32), "x", 768) == 32
    with pytest.raises(ValueError, match="768"):
        _check_nm(np.zeros((3, 512, 32), np.float32), "x", 768)
