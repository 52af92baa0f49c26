"""GPU: the objective of one data-parallel rank (ops.baseline_objective_rows_fwd_bwd, csrc/baseline_loss.hip): the forward over the
gathered global batch of up to 4096 rows, the backward for the pairs [p0, p0 + n) the rank owns.

* With p0 = 0, n = B it equals the unsharded ops.baseline_objective_fwd_bwd bit for bit.
* Shard invariance: the gradient rows of any cut equal the same rows of the p0 = 0, n = B call bit for bit, and so do the losses.
* Past the unsharded limit (tests/golden/baseline_loss_dp.npz, written by the reference's own functions): decisions equal the
  reference's at every anchor with a clear decision; values and gradient within 4 x the reference's own fp32-vs-fp64 distance of
  fp64 (the margin of tests/test_baseline_loss_gpu.py for another summation order), against the fp64 oracle with the kernel's own
  decisions if a near-tie anchor decided differently. Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

import baseline_loss_oracle as O
from make_baseline_loss_dp_golden import CASES as BIG_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baseline_loss_dp.npz")
BG = (0.5, 2.0)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def stored(golden, name, key):
    pre = f"{name}/{key}."
    return {k[len(pre):]: v for k, v in golden.items() if k.startswith(pre)}


def rows(z_i, z_j, p0=0, n=None, bg=BG, **kw):
    from neuralsampleid_amd import ops
    return ops.baseline_objective_rows_fwd_bwd(z_i, z_j, p0, n, O.MARGIN, bg[0], bg[1], **kw)


def assert_shards_equal_whole(z_i, z_j, whole, cuts, bg=BG):
    out, dzi, dzj = whole[:3]
    for p0, n in cuts:
        o, gi, gj = rows(z_i, z_j, p0, n, bg)
        assert torch.equal(o, out), f"the losses of shard [{p0}, {p0 + n}) differ from the whole call's"
        assert gi.shape == (n, z_i.shape[1]) and gj.shape == gi.shape
        assert torch.equal(gi, dzi[p0:p0 + n]) and torch.equal(gj, dzj[p0:p0 + n]), f"shard [{p0}, {p0 + n})"


@pytest.mark.parametrize("name", ["r8x64", "r72x256", "r40x2048", "b1", "b3x16", "novalid"])
def test_whole_range_equals_the_unsharded_op(name):
    from neuralsampleid_amd import ops
    z_i, z_j = (t.to(DEV) for t in O.make_case(name))
    want = ops.baseline_objective_fwd_bwd(z_i, z_j, O.MARGIN, *BG, mining=True)
    got = rows(z_i, z_j, 0, z_i.shape[0], mining=True)
    for k in range(3):
        assert torch.equal(got[k], want[k]), ("out", "dz_i", "dz_j")[k]
    for k in ("pidx", "nidx", "valid", "active"):
        assert torch.equal(got[3][k], want[3][k]), k
    default = rows(z_i, z_j)                                # npairs=None: every pair from p0
    assert all(torch.equal(a, b) for a, b in zip(default, got[:3]))
    out_f, none_i, none_j = rows(z_i, z_j, want_grad=False)
    assert none_i is None and none_j is None and torch.equal(out_f, got[0])


@pytest.mark.parametrize("name,cuts", [
    ("r72x256", [(0, 36), (36, 36)]),
    ("r72x256", [(0, 24), (24, 24), (48, 24)]),
    ("r72x256", [(0, 5), (5, 7), (12, 60)]),               # a tile of owned rows straddles the two views and ends short
    ("r40x2048", [(0, 10), (10, 10), (20, 10), (30, 10)]),
    ("b3x16", [(0, 1), (1, 1), (2, 1)]),
])
def test_shard_invariance(name, cuts):
    z_i, z_j = (t.to(DEV) for t in O.make_case(name))
    whole = rows(z_i, z_j, 0, z_i.shape[0])
    assert_shards_equal_whole(z_i, z_j, whole, cuts)
    cat_i = torch.cat([rows(z_i, z_j, p0, n)[1] for p0, n in cuts])
    cat_j = torch.cat([rows(z_i, z_j, p0, n)[2] for p0, n in cuts])
    assert torch.equal(cat_i, whole[1]) and torch.equal(cat_j, whole[2])


def within(what, got, want, floor):
    err = abs(float(got) - float(want))
    print(f"  {what}: |kernel - fp64| = {err:.3g}, allowed 4 x {float(floor):.3g}")
    return err <= 4.0 * float(floor)


@pytest.mark.parametrize("name,cuts", [
    ("r1032x64", [(129 * r, 129) for r in range(8)]),
    ("r2048x64", [(256 * r, 256) for r in (0, 3, 7)]),
])
def test_past_the_unsharded_limit_against_the_reference(golden, name, cuts):
    a, b = O.recipe(**BIG_CASES[name])
    assert O.input_digest(a, b) == str(golden[f"{name}/sha256"])
    z_i, z_j = a.to(DEV), b.to(DEV)
    B = z_i.shape[0]
    out, dzi, dzj, mining = rows(z_i, z_j, 0, B, (1.0, 1.0), mining=True)
    o = out.cpu()
    print(f"{name}: loss {float(o[0]):.8f} cls {float(o[1]):.8f} trip {float(o[2]):.8f} n_valid {int(o[3])}")
    # decisions: the reference's at every anchor with a clear decision
    clear = torch.from_numpy(golden[f"{name}/gap"]) >= O.GAP_MIN
    same = torch.ones_like(clear)
    for key in ("valid", "pidx", "nidx"):
        got = mining[key].cpu().long()
        want = torch.from_numpy(golden[f"{name}/{key}"]).long()
        differ = got != want
        print(f"  {key}: {int(differ.sum())} anchors differ from the reference, {int((differ & clear).sum())} of them with a clear decision")
        assert not bool((differ & clear).any()), f"{name}: {key} differs at an anchor with a clear decision"
        same &= ~differ
    assert int(o[3]) == int(mining["valid"].sum())
    if bool(same.all()):
        assert int(o[3]) == int(golden[f"{name}/valid"].sum())
        dcls, dtrip = stored(golden, name, "dcls64"), stored(golden, name, "dtrip64")
        ref = {k: float(golden[f"{name}/{k}64"]) for k in ("cls", "trip", "loss")}
        ref_dz = {k: dcls[k] + dtrip[k] for k in dcls}         # beta = gamma = 1; the compact form is linear
    else:
        r = O.objective64(a, b, O.MARGIN, decisions=(mining["valid"].cpu(), mining["pidx"].cpu(), mining["nidx"].cpu()))
        ref = {k: float(r[k]) for k in ("cls", "trip", "loss")}
        ref_dz = O.compact(r["dz"], False)
    f = lambda k: float(golden[f"{name}/floor_{k}"])       # noqa: E731
    err_dz = O.compact_maxerr(torch.cat([dzi, dzj]), ref_dz)
    print(f"  dz: max |kernel - fp64| = {err_dz:.3g}, allowed 4 x {f('dz'):.3g}")
    ok = [within("cls", o[1], ref["cls"], f("cls")), within("trip", o[2], ref["trip"], f("trip")),
          within("loss", o[0], ref["loss"], f("loss")), err_dz <= 4.0 * f("dz")]
    assert_shards_equal_whole(z_i, z_j, (out, dzi, dzj), cuts, (1.0, 1.0))
    assert all(ok)


def test_two_runs_are_bitwise_equal():
    z_i, z_j = (t.to(DEV) for t in O.recipe(**BIG_CASES["r1032x64"]))
    runs = [rows(z_i, z_j, 3 * 129, 129) for _ in range(2)]
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_limits_are_refused():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd._lib import lib
    z = torch.zeros(8, 16, device=DEV)
    for zz, kw in ((torch.zeros(2049, 16, device=DEV), {}), (torch.zeros(4, 24, device=DEV), {}), (z, dict(p0=5, npairs=4)),
                   (z, dict(p0=0, npairs=0)), (z, dict(p0=-1, npairs=2)),
                   (z, dict(ws=torch.empty(lib.nsid_baseline_loss_rows_ws_floats(16, 16) - 1, device=DEV)))):
        with pytest.raises((ValueError, RuntimeError)):
            ops.baseline_objective_rows_fwd_bwd(zz, zz.clone(), **kw)
    # the C entry itself refuses what the wrapper refuses
    ws = torch.empty(lib.nsid_baseline_loss_rows_ws_floats(16, 16), device=DEV)
    out = torch.empty(4, device=DEV)
    for Bg, D, p0, n in ((2049, 16, 0, 1), (8, 24, 0, 8), (8, 16, 5, 4), (8, 16, 0, 0), (8, 16, -1, 2)):
        assert lib.nsid_baseline_objective_rows_fwd_bwd(z.data_ptr(), z.data_ptr(), Bg, D, p0, n, 0.2, 1.0, 1.0, ws.data_ptr(),
                                                        out.data_ptr(), None, None, None) == -1
    # the unsharded entries keep their limit
    big = torch.zeros(1025, 16, device=DEV)
    with pytest.raises((ValueError, RuntimeError)):
        ops.pair_ce_fwd_bwd(big, big.clone())
    with pytest.raises((ValueError, RuntimeError)):
        ops.baseline_objective_fwd_bwd(big, big.clone())


def test_rows_form_replays_from_a_captured_graph():
    """captured once on a single stream with caller-owned buffers, shard 1 of 2; replayed on the no-valid-anchor input and then on a
    recipe input copied into the same buffers"""
    from neuralsampleid_amd._lib import lib
    B, D, p0, n = 8, 64, 4, 4
    inputs = {k: tuple(t.to(DEV) for t in O.make_case(k)) for k in ("novalid", "r8x64")}
    eager = {k: rows(zi, zj, p0, n) for k, (zi, zj) in inputs.items()}
    zi, zj = torch.empty(B, D, device=DEV), torch.empty(B, D, device=DEV)
    ws = torch.empty(lib.nsid_baseline_loss_rows_ws_floats(2 * B, D), device=DEV)
    out, dz = torch.empty(4, device=DEV), (torch.empty(n, D, device=DEV), torch.empty(n, D, device=DEV))
    zi.copy_(inputs["r8x64"][0])
    zj.copy_(inputs["r8x64"][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rows(zi, zj, p0, n, ws=ws, out=out, dz=dz)        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rows(zi, zj, p0, n, ws=ws, out=out, dz=dz)
    for k in ("novalid", "r8x64"):
        zi.copy_(inputs[k][0])
        zj.copy_(inputs[k][1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[k][0]) and torch.equal(dz[0], eager[k][1]) and torch.equal(dz[1], eager[k][2]), k
    assert int(eager["novalid"][0][3]) == 0 and float(eager["novalid"][0][2]) == 0.0 and int(eager["r8x64"][0][3]) > 0
