"""GPU: the fused losses of csrc/baseline_loss.hip against the reference's numbers (tests/golden/baseline_loss.npz).

Mining decisions: n_valid, valid, p*, n* equal the golden's (the reference's fp32 decisions) for every anchor whose decision gap is
at least 1e-5. If a near-tie anchor decides differently, values and gradients of that case are compared against the fp64 oracle
evaluated with the kernel's own decisions; otherwise against the golden's fp64 run.

Tolerance: the golden records, per case and quantity, how far the reference's own fp32 run is from its fp64 run (floor_*). The
kernels sum in another order, so they may be 4 x that far from fp64. (A floor of exactly 0 -- a loss that is exactly 0, a gradient
that is exactly zero -- demands the exact value.) Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

import baseline_loss_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baseline_loss.npz")
PAIR_CASES = [n for n, (k, _) in O.CASES.items() if k == "pair"]
TRIPLET_CASES = [n for n, (k, _) in O.CASES.items() if k == "triplet"]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def stored(golden, name, key):
    pre = f"{name}/{key}."
    return {k[len(pre):]: v for k, v in golden.items() if k.startswith(pre)}


def within(what, got, want, floor):
    err = abs(float(got) - float(want))
    print(f"  {what}: |kernel - fp64| = {err:.3g}, allowed 4 x {float(floor):.3g}")
    return err <= 4.0 * float(floor)


def grad_within(what, got, ref, floor):
    err = O.compact_maxerr(got, ref)
    print(f"  {what}: max |kernel - fp64| = {err:.3g}, allowed 4 x {float(floor):.3g}")
    return err <= 4.0 * float(floor)


def check_decisions(golden, name, mining, n_valid):
    """True: every decision equals the golden's; False: only near-tie anchors differ (the caller switches to the oracle)"""
    gap = torch.from_numpy(golden[f"{name}/gap"])
    clear = gap >= O.GAP_MIN
    same = torch.ones_like(clear)
    for key in ("valid", "pidx", "nidx"):
        got = mining[key].cpu().long()
        want = torch.from_numpy(golden[f"{name}/{key}"]).long()
        assert bool((got[clear] == want[clear]).all()), f"{name}: {key} differs at an anchor with a clear decision"
        same &= got == want
    if bool(same.all()):
        assert int(n_valid) == int(golden[f"{name}/valid"].sum())
        return True
    assert int(n_valid) == int(mining["valid"].sum())
    return False


def pair_reference(golden, name, mining, same, beta=1.0, gamma=1.0):
    """fp64 values and compact gradients of a pair case: the golden's, or the oracle's with the kernel's decisions"""
    if same:
        ref = {k: float(golden[f"{name}/{k}64"]) for k in ("cls", "trip")}
        ref.update({k: stored(golden, name, k + "64") for k in ("dcls", "dtrip")})
        if (beta, gamma) == (1.0, 1.0):
            ref["loss"], ref["dz"] = float(golden[f"{name}/loss64"]), stored(golden, name, "dz64")
            return ref
        ref["loss"] = beta * ref["cls"] + gamma * ref["trip"]
        ref["dz"] = {k: beta * ref["dcls"][k] + gamma * ref["dtrip"][k] for k in ref["dcls"]}       # the compact form is linear
        return ref
    z_i, z_j = O.make_case(name)
    r = O.objective64(z_i, z_j, O.MARGIN, beta, gamma,
                      decisions=(mining["valid"].cpu(), mining["pidx"].cpu(), mining["nidx"].cpu()))
    whole = z_i.shape[1] <= 256
    return dict(cls=float(r["cls"]), trip=float(r["trip"]), loss=float(r["loss"]), dz=O.compact(r["dz"], whole),
                dcls=O.compact(r["dcls"], False), dtrip=O.compact(r["dtrip"], False))


@pytest.mark.parametrize("bg", [(1.0, 1.0), (0.5, 2.0)])
@pytest.mark.parametrize("name", PAIR_CASES)
def test_objective_matches_the_reference(golden, name, bg):
    from neuralsampleid_amd import ops
    beta, gamma = bg
    z_i, z_j = (t.to(DEV) for t in O.make_case(name))
    out, dzi, dzj, mining = ops.baseline_objective_fwd_bwd(z_i, z_j, O.MARGIN, beta, gamma, mining=True)
    out = out.cpu()
    print(f"{name} beta={beta} gamma={gamma}: loss {float(out[0]):.8f} cls {float(out[1]):.8f} trip {float(out[2]):.8f} "
          f"n_valid {int(out[3])}")
    same = check_decisions(golden, name, mining, out[3])
    ref = pair_reference(golden, name, mining, same, beta, gamma)
    f = lambda k: float(golden[f"{name}/floor_{k}"])       # noqa: E731
    # the floors of loss and dz were recorded at beta = gamma = 1: other weights scale the parts
    floor_loss = f("loss") if bg == (1.0, 1.0) else beta * f("cls") + gamma * f("trip")
    floor_dz = f("dz") if bg == (1.0, 1.0) else beta * f("dcls") + gamma * f("dtrip")
    ok = [within("cls", out[1], ref["cls"], f("cls")), within("trip", out[2], ref["trip"], f("trip")),
          within("loss", out[0], ref["loss"], floor_loss),
          grad_within("dz", torch.cat([dzi, dzj]), ref["dz"], floor_dz)]
    assert all(ok)
    # forward only: the same losses, bit for bit
    out_f, none_i, none_j = ops.baseline_objective_fwd_bwd(z_i, z_j, O.MARGIN, beta, gamma, want_grad=False)
    assert none_i is None and none_j is None and torch.equal(out_f.cpu(), out)


@pytest.mark.parametrize("name", PAIR_CASES)
def test_losses_through_autograd(golden, name):
    """classifier_loss and triplet_loss with the reference's signatures, a non-unit upstream gradient, and the parts of the objective"""
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.simclr.triplet import baseline_objective, classifier_loss, triplet_loss
    up = 1.75
    z_i, z_j = (t.to(DEV).requires_grad_(True) for t in O.make_case(name))
    B = z_i.shape[0]
    f = lambda k: float(golden[f"{name}/floor_{k}"])       # noqa: E731
    cls = classifier_loss(z_i, z_j)
    assert cls.dim() == 0
    (cls * up).backward()
    dcls = torch.cat([z_i.grad, z_j.grad]) / up
    print(name)
    ok = [within("classifier_loss", cls, golden[f"{name}/cls64"], f("cls")),
          grad_within("d classifier_loss", dcls, stored(golden, name, "dcls64"), f("dcls"))]
    # triplet_loss alone, on the rows the step hands it. They are normalised in fp64 and rounded once, so that the golden's fp64 run
    # is the reference of this call too; its gradient wrt the rows goes through the normalisation's backward in fp64 on the host
    z64 = torch.cat([z_i, z_j]).detach().cpu().double().requires_grad_(True)
    zn64 = torch.nn.functional.normalize(z64, dim=1)
    e = zn64.detach().float().to(DEV).requires_grad_(True)
    labels = O.pair_labels(B).to(DEV)
    _, _, mining = ops.triplet_fwd_bwd(e.detach(), labels, O.MARGIN, mining=True)
    trip = triplet_loss(e, labels, margin=O.MARGIN)
    assert trip.dim() == 0
    (trip * up).backward()
    same = check_decisions(golden, name, mining, int(mining["valid"].sum()))
    ref = pair_reference(golden, name, mining, same)
    (zn64 * (e.grad.cpu().double() / up)).sum().backward()
    ok += [within("triplet_loss", trip, ref["trip"], f("trip")),
           grad_within("d triplet_loss", z64.grad, ref["dtrip"], f("dtrip"))]
    assert all(ok)
    z_i.grad = z_j.grad = None
    # the objective's parts and its gradient scale with the upstream gradient
    loss, lc, lt = baseline_objective(z_i, z_j, O.MARGIN, 0.5, 2.0)
    assert loss.dim() == 0 and not lc.requires_grad and not lt.requires_grad
    (loss * up).backward()
    out, dzi, dzj = ops.baseline_objective_fwd_bwd(z_i.detach(), z_j.detach(), O.MARGIN, 0.5, 2.0)
    assert torch.equal(torch.stack([loss.detach(), lc, lt]), out[:3])
    assert torch.equal(z_i.grad, dzi * up) and torch.equal(z_j.grad, dzj * up)
    assert float(loss) == pytest.approx(0.5 * float(lc) + 2.0 * float(lt), rel=2e-7, abs=1e-12)


@pytest.mark.parametrize("name", TRIPLET_CASES)
def test_triplet_with_general_labels(golden, name):
    from neuralsampleid_amd import ops
    e, labels = (t.to(DEV) for t in O.make_case(name))
    out, de, mining = ops.triplet_fwd_bwd(e, labels, O.MARGIN, mining=True)
    out = out.cpu()
    print(f"{name}: trip {float(out[0]):.9f} n_valid {int(out[1])}")
    same = check_decisions(golden, name, mining, out[1])
    if same:
        ref_trip, ref_de = float(golden[f"{name}/trip64"]), stored(golden, name, "de64")
    else:
        r = O.triplet64(*O.make_case(name), O.MARGIN, decisions=(mining["valid"].cpu(), mining["pidx"].cpu(), mining["nidx"].cpu()))
        ref_trip, ref_de = float(r["trip"]), O.compact(r["de"], True)
    ok = [within("trip", out[0], ref_trip, golden[f"{name}/floor_trip"]),
          grad_within("de", de, ref_de, golden[f"{name}/floor_de"])]
    assert all(ok)
    if name == "hand8":          # one valid anchor, inactive hinge: a count of 1, a loss of 0, no gradient
        assert int(out[1]) == 1 and float(out[0]) == 0.0 and float(de.abs().max()) == 0.0 and not bool(mining["active"].any())
    out_f, none = ops.triplet_fwd_bwd(e, labels, O.MARGIN, want_grad=False)
    assert none is None and torch.equal(out_f.cpu(), out)


@pytest.mark.parametrize("name", ["r40x2048", "r72x256", "labels20"])
def test_two_runs_are_bitwise_equal(name):
    from neuralsampleid_amd import ops
    a, b = (t.to(DEV) for t in O.make_case(name))
    if O.CASES[name][0] == "pair":
        runs = [ops.baseline_objective_fwd_bwd(a, b, O.MARGIN, 0.5, 2.0) + ops.pair_ce_fwd_bwd(a, b) for _ in range(2)]
    else:
        runs = [ops.triplet_fwd_bwd(a, b, O.MARGIN) for _ in range(2)]
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_limits_are_refused():
    from neuralsampleid_amd import ops
    for B, D in ((4, 24), (4, 8), (4, 2064), (1025, 16)):
        z = torch.zeros(B, D, device=DEV)
        with pytest.raises((ValueError, RuntimeError)):
            ops.pair_ce_fwd_bwd(z, z.clone())
    with pytest.raises(RuntimeError):
        ops.triplet_fwd_bwd(torch.zeros(8, 16, device=DEV), torch.zeros(8, device=DEV, dtype=torch.int32))


def test_objective_replays_from_a_captured_graph():
    """captured once on a single stream; replayed on the no-valid-anchor input and then on a recipe input copied into the same
    buffers: n_valid, the zero-anchor case and beta / gamma stay on the device"""
    from neuralsampleid_amd import ops
    from neuralsampleid_amd._lib import lib
    B, D = 8, 64
    inputs = {n: tuple(t.to(DEV) for t in O.make_case(n)) for n in ("novalid", "r8x64")}
    eager = {n: ops.baseline_objective_fwd_bwd(zi, zj, O.MARGIN, 0.5, 2.0) for n, (zi, zj) in inputs.items()}
    zi, zj = torch.empty(B, D, device=DEV), torch.empty(B, D, device=DEV)
    ws = torch.empty(lib.nsid_baseline_loss_ws_floats(2 * B, D), device=DEV)
    out, dz = torch.empty(4, device=DEV), (torch.empty(B, D, device=DEV), torch.empty(B, D, device=DEV))
    zi.copy_(inputs["r8x64"][0])
    zj.copy_(inputs["r8x64"][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.baseline_objective_fwd_bwd(zi, zj, O.MARGIN, 0.5, 2.0, ws=ws, out=out, dz=dz)        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.baseline_objective_fwd_bwd(zi, zj, O.MARGIN, 0.5, 2.0, ws=ws, out=out, dz=dz)
    for n in ("novalid", "r8x64"):
        zi.copy_(inputs[n][0])
        zj.copy_(inputs[n][1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[n][0]) and torch.equal(dz[0], eager[n][1]) and torch.equal(dz[1], eager[n][2]), n
    assert int(eager["novalid"][0][3]) == 0 and float(eager["novalid"][0][2]) == 0.0 and int(eager["r8x64"][0][3]) > 0
