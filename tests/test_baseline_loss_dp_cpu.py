"""CPU: the data-parallel form of the baseline's training objective.

* tests/baseline_loss_oracle.py reproduces the numbers the reference's own functions wrote into tests/golden/baseline_loss_dp.npz
  (tests/golden/make_baseline_loss_dp_golden.py): the two pair cases past the row limit of the unsharded kernel.
* world_size = 2 over gloo: parallel.dist_baseline_objective with an fp64 oracle as its rows kernel reproduces the single-process
  gradient of the objective on the concatenated batch after a SUM all-reduce.
* GradReducer.install_param_hooks(): autograd's accumulation hooks fire every bucket during backward, and the buckets sum."""
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:           # spawned ranks re-import this module without conftest.py
        sys.path.insert(0, _p)

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import baseline_loss_oracle as O
from make_baseline_loss_dp_golden import CASES, NEAR_TIE_SHARE_MAX
from synth import synth_randn

GOLDEN = os.path.join(ROOT, "tests", "golden", "baseline_loss_dp.npz")
WORLD = 2
BETA, GAMMA = 0.5, 2.0


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def stored(golden, name, key):
    pre = f"{name}/{key}."
    return {k[len(pre):]: v for k, v in golden.items() if k.startswith(pre)}


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_reproduces_the_reference(golden, name):
    a, b = O.recipe(**CASES[name])
    assert O.input_digest(a, b) == str(golden[f"{name}/sha256"]), "the inputs are not the ones the golden was written from"
    r = O.objective64(a, b)
    for k in ("cls", "trip", "loss"):
        assert abs(float(r[k]) - float(golden[f"{name}/{k}64"])) <= 1e-12, k
    dcls, dtrip = stored(golden, name, "dcls64"), stored(golden, name, "dtrip64")
    assert O.compact_maxerr(r["dcls"], dcls) <= 1e-12
    assert O.compact_maxerr(r["dtrip"], dtrip) <= 1e-12
    assert O.compact_maxerr(r["dz"], {k: dcls[k] + dtrip[k] for k in dcls}) <= 1e-12      # dz64 is not stored: the compact form is linear
    d = r["mining"]
    clear = torch.from_numpy(golden[f"{name}/gap"]) >= O.GAP_MIN      # the golden's decisions are the reference's fp32 ones
    assert bool((d["valid"][clear] == torch.from_numpy(golden[f"{name}/valid"])[clear]).all())
    assert bool((d["pidx"][clear] == torch.from_numpy(golden[f"{name}/pidx"]).long()[clear]).all())
    assert bool((d["nidx"][clear] == torch.from_numpy(golden[f"{name}/nidx"]).long()[clear]).all())
    if bool(clear.all()):
        assert r["n_valid"] == int(golden[f"{name}/valid"].sum())


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_mix_valid_and_invalid_anchors(golden, name):
    valid, gap = golden[f"{name}/valid"], golden[f"{name}/gap"]
    assert valid.shape[0] == 2 * CASES[name]["B"]
    share, near = valid.mean(), (gap < O.GAP_MIN).mean()
    print(f"{name}: valid share {share:.3f}, near-tie share {near:.4f}")
    assert 0.25 <= share <= 0.98
    assert near < NEAR_TIE_SHARE_MAX
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_workspace_query():
    from neuralsampleid_amd._lib import lib
    assert lib.nsid_baseline_loss_rows_ws_floats(4096, 2048) >= 2 * 4096 * 4096 + 4096 * 2048
    assert lib.nsid_baseline_loss_rows_ws_floats(128, 64) == lib.nsid_baseline_loss_ws_floats(128, 64)


def test_public_names_and_no_cpu_path():
    from neuralsampleid_amd import ops, parallel
    z_i, z_j = O.make_case("r8x64")
    with pytest.raises(RuntimeError):
        ops.baseline_objective_rows_fwd_bwd(z_i, z_j)
    with pytest.raises(RuntimeError):                # no process group, no rows_fn: simclr.triplet.baseline_objective, which has no CPU path
        parallel.dist_baseline_objective(z_i, z_j)


# ---- two ranks over gloo -------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def oracle_rows(zi_all, zj_all, p0, n, margin, beta, gamma):
    """the contract of ops.baseline_objective_rows_fwd_bwd in fp64: the GLOBAL losses, the gradient rows of pairs [p0, p0 + n)"""
    with torch.enable_grad():          # called from inside autograd.Function.forward, where grad mode is off
        r = O.objective64(zi_all, zj_all, margin, beta, gamma)
    Bg = zi_all.shape[0]
    out = torch.stack([r["loss"], r["cls"], r["trip"], torch.tensor(float(r["n_valid"]), dtype=torch.float64)]).to(zi_all.dtype)
    dz = r["dz"].to(zi_all.dtype)
    return out, dz[p0:p0 + n].clone(), dz[Bg + p0:Bg + p0 + n].clone()


def tiny_params():
    g = torch.Generator().manual_seed(5)
    return {"w1": torch.randn(24, 16, generator=g) * 0.3, "w2": torch.randn(8, 24, generator=g) * 0.3}


def embed(x, P):
    z = torch.tanh(x @ P["w1"].t()) @ P["w2"].t()
    return z / z.norm(dim=1, keepdim=True).clamp_min(1e-10)


def tiny_inputs(B=6):
    x_i = synth_randn("bldp_xi", B, 16)
    return x_i, x_i + 0.3 * synth_randn("bldp_xj", B, 16)


def _init(rank, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from neuralsampleid_amd import parallel
    assert parallel.init_from_env("gloo")[::2] == (rank, WORLD)
    return parallel


def _objective_worker(rank, port, out):
    parallel = _init(rank, port)
    x_i, x_j = tiny_inputs()
    p0, n = parallel.shard_range(x_i.shape[0], rank, WORLD)
    P = {k: v.clone().requires_grad_(True) for k, v in tiny_params().items()}
    z_i, z_j = embed(x_i[p0:p0 + n], P), embed(x_j[p0:p0 + n], P)
    loss, cls, trip = parallel.dist_baseline_objective(z_i, z_j, O.MARGIN, BETA, GAMMA, rows_fn=oracle_rows)
    assert not cls.requires_grad and not trip.requires_grad
    (1.75 * loss).backward()
    flat = torch.cat([P[k].grad.reshape(-1) for k in sorted(P)]) / 1.75
    parallel.allreduce_gradients(flat)
    out.put((rank, float(loss.detach()), float(cls), float(trip), flat.tolist()))
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(target):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    for p in procs:                    # (each rank puts a few KB: less than a pipe holds, so it can exit before the queue is read)
        p.join(120)
    assert [p.exitcode for p in procs] == [0] * WORLD, f"ranks died or hung: {[p.exitcode for p in procs]}"
    return sorted((q.get() for _ in range(WORLD)), key=lambda t: t[0])


def test_two_rank_objective_matches_single_process():
    got = _run_ranks(_objective_worker)
    x_i, x_j = tiny_inputs()
    P = {k: v.clone().requires_grad_(True) for k, v in tiny_params().items()}
    r = O.objective64(embed(x_i, P).detach(), embed(x_j, P).detach(), O.MARGIN, BETA, GAMMA)
    assert 0 < r["n_valid"], "the tiny batch must exercise the triplet part"
    z_i, z_j = embed(x_i, P), embed(x_j, P)
    B = z_i.shape[0]
    dz = r["dz"].float()
    torch.autograd.backward([z_i, z_j], [dz[:B], dz[B:]])
    flat1 = torch.cat([P[k].grad.reshape(-1) for k in sorted(P)])
    for rank, loss, cls, trip, flat in got:        # every rank reports the global losses
        assert abs(loss - float(r["loss"])) < 1e-5 and abs(cls - float(r["cls"])) < 1e-5 and abs(trip - float(r["trip"])) < 1e-5
        assert torch.allclose(torch.tensor(flat), flat1, atol=1e-5, rtol=1e-4)          # SUM of per-rank grads == global-batch grad
    assert got[0][1:4] == got[1][1:4]
    assert float(flat1.abs().max()) > 1e-3


# ---- GradReducer.install_param_hooks ----------------------------------------------------------------------------------------------
def hooked_model():
    torch.manual_seed(7)
    return torch.nn.Sequential(torch.nn.Linear(16, 24), torch.nn.Tanh(), torch.nn.Linear(24, 24), torch.nn.Tanh(), torch.nn.Linear(24, 8))


def flatten_grads(model):
    """every p.grad a view of one flat buffer, as FusedClipAdam lays them out"""
    params = list(model.parameters())
    offs, tot = [], 0
    for p in params:
        offs.append(tot)
        tot += (p.numel() + 7) // 8 * 8
    flat = torch.zeros(tot)
    for p, o in zip(params, offs):
        p.grad = flat[o:o + p.numel()].view_as(p)
    return params, flat, offs


def hooked_loss(model, rank):
    x_i, x_j = tiny_inputs(4)
    s = float(rank + 1)
    return (model(s * x_i) * model(s * x_j)).sum()          # the encoder runs once per view: every parameter is used twice


def _hooks_worker(rank, port, out):
    parallel = _init(rank, port)
    model = hooked_model()
    params, flat, offs = flatten_grads(model)
    red = parallel.GradReducer(params, flat, offs, bucket_bytes=512, uses_per_step=1).install_param_hooks()
    red.start_step()
    hooked_loss(model, rank).backward()
    fired = list(red.fired)
    red.finish()
    red.remove_param_hooks()
    out.put((rank, fired, red.bounds, flat.tolist()))
    dist.barrier()
    dist.destroy_process_group()


def test_param_hooks_fire_every_bucket_during_backward_and_sum():
    got = _run_ranks(_hooks_worker)
    want = None
    for rank in range(WORLD):
        model = hooked_model()
        _, flat, _ = flatten_grads(model)
        hooked_loss(model, rank).backward()
        want = flat.clone() if want is None else want + flat
    for rank, fired, bounds, flat in got:
        assert len(bounds) >= 3 and bounds[0][1] == want.numel() and bounds[-1][0] == 0
        assert fired == list(range(len(bounds))), "every bucket fires from the hooks, the last parameters' bucket first"
        assert torch.allclose(torch.tensor(flat), want, atol=1e-5, rtol=1e-5)
    assert float(want.abs().max()) > 1e-3


def test_param_hooks_fire_once_per_step_and_come_off():
    from neuralsampleid_amd import parallel
    model = hooked_model()
    params, flat, offs = flatten_grads(model)
    red = parallel.GradReducer(params, flat, offs, bucket_bytes=512, uses_per_step=1).install_param_hooks()
    with pytest.raises(RuntimeError):
        red.install_param_hooks()
    for _ in range(2):
        red.start_step()
        hooked_loss(model, 0).backward()
        assert red.fired == list(range(len(red.bounds))) and red.remaining == [0] * len(red.bounds)
        red.finish()
    # two uses per step is the GNN's count (its own hook reports every view); autograd accumulates once, so nothing would fire
    late = parallel.GradReducer(params, flat, offs, bucket_bytes=512, uses_per_step=2)
    red.remove_param_hooks()
    late.install_param_hooks()
    late.start_step()
    red.start_step()
    hooked_loss(model, 0).backward()
    assert late.fired == [] and red.fired == []
    late.remove_param_hooks()
    assert late._param_hooks == []
