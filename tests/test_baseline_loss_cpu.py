"""CPU: the fp64 oracle of the baseline's training objective (tests/baseline_loss_oracle.py) reproduces the numbers the reference's own
functions wrote into tests/golden/baseline_loss.npz; the inputs are in the regime the GPU test needs (a real mix of valid and
invalid anchors, hardly any near tie); the public names exist and refuse CPU tensors."""
import os

import numpy as np
import pytest
import torch

import baseline_loss_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baseline_loss.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def stored(golden, name, key):
    """a compact gradient of the golden as baseline_loss_oracle.compact wrote it"""
    pre = f"{name}/{key}."
    return {k[len(pre):]: v for k, v in golden.items() if k.startswith(pre)}


@pytest.mark.parametrize("name", list(O.CASES))
def test_oracle_reproduces_the_reference(golden, name):
    kind, _ = O.CASES[name]
    a, b = O.make_case(name)
    assert O.input_digest(a, b) == str(golden[f"{name}/sha256"]), "the inputs are not the ones the golden was written from"
    if kind == "pair":
        r = O.objective64(a, b)
        for k in ("cls", "trip", "loss"):
            assert abs(float(r[k]) - float(golden[f"{name}/{k}64"])) <= 1e-12, k
        for k in ("dz", "dcls", "dtrip"):
            assert O.compact_maxerr(r[k], stored(golden, name, k + "64")) <= 1e-12, k
    else:
        r = O.triplet64(a, b)
        assert abs(float(r["trip"]) - float(golden[f"{name}/trip64"])) <= 1e-12
        assert O.compact_maxerr(r["de"], stored(golden, name, "de64")) <= 1e-12
    d = r["mining"]
    clear = torch.from_numpy(golden[f"{name}/gap"]) >= O.GAP_MIN      # the golden's decisions are the reference's fp32 ones
    assert bool((d["valid"][clear] == torch.from_numpy(golden[f"{name}/valid"])[clear]).all())
    assert bool((d["pidx"][clear] == torch.from_numpy(golden[f"{name}/pidx"]).long()[clear]).all())
    assert bool((d["nidx"][clear] == torch.from_numpy(golden[f"{name}/nidx"]).long()[clear]).all())
    if bool(clear.all()):
        assert r["n_valid"] == int(golden[f"{name}/valid"].sum())


@pytest.mark.parametrize("name", O.RECIPE)
def test_recipe_inputs_mix_valid_and_invalid_anchors(golden, name):
    valid, gap = golden[f"{name}/valid"], golden[f"{name}/gap"]
    share = valid.mean()
    near = (gap < O.GAP_MIN).mean()
    print(f"{name}: valid share {share:.3f}, near-tie share {near:.4f}")
    assert 0.25 <= share <= 0.98
    assert near <= 0.05


def test_degenerate_cases_are_what_they_claim(golden):
    assert golden["b1/valid"].sum() == 0 and float(golden["b1/cls32"]) == 0.0 and float(golden["b1/trip32"]) == 0.0
    assert golden["novalid/valid"].sum() == 0 and float(golden["novalid/trip32"]) == 0.0 and float(golden["novalid/cls32"]) > 0.0
    # hand8: anchor 0 alone is valid, and its hinge is inactive: the loss is 0 with a count of 1
    assert golden["hand8/valid"].tolist() == [True] + [False] * 7 and float(golden["hand8/trip32"]) == 0.0
    e, labels = O.make_case("hand8")
    d = O.mine(e @ e.T, labels)
    assert not bool(d["active"].any()) and float(d["neg"][0]) > float(d["pos"][0]) + O.MARGIN
    # labels20: anchors without a positive are valid and contribute 0
    lab = golden["labels20/pidx"]
    assert (lab < 0).sum() == 15 and golden["labels20/valid"][lab < 0].all()
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_public_names_and_no_cpu_path():
    from neuralsampleid_amd.simclr.triplet import BaselineModel, baseline_objective, classifier_loss, triplet_loss  # noqa: F401
    from neuralsampleid_amd import ops
    z_i, z_j = O.make_case("r8x64")
    with pytest.raises(RuntimeError):
        classifier_loss(z_i, z_j)
    with pytest.raises(RuntimeError):
        triplet_loss(torch.cat([z_i, z_j]), O.pair_labels(8))
    with pytest.raises(RuntimeError):
        baseline_objective(z_i, z_j)
    for fn, args in ((ops.pair_ce_fwd_bwd, (z_i, z_j)), (ops.triplet_fwd_bwd, (z_i, O.pair_labels(4))),
                     (ops.baseline_objective_fwd_bwd, (z_i, z_j))):
        with pytest.raises(RuntimeError):
            fn(*args)


def test_workspace_query_and_limits():
    from neuralsampleid_amd._lib import lib
    assert lib.nsid_workspace_bytes(b"baseline_loss", 1024, 2048) == lib.nsid_baseline_loss_ws_floats(1024, 2048) * 4
    assert lib.nsid_baseline_loss_ws_floats(1024, 2048) >= 2 * 1024 * 1024 + 1024 * 2048
    assert lib.nsid_workspace_bytes(b"gem_pool_bwd", 3, 1024) == 3 * 16 * 4
