"""GPU: the data-parallel training step of the ResNet-IBN baseline (parallel.dist_baseline_objective, GradReducer.install_param_hooks,
tools/baseline_train_synthetic.py --dp).

One rank with forced collectives (the direct RCCL communicator): the step with the all-gather of the embeddings, the rows kernel and
the bucketed all-reduce launched from autograd's accumulation hooks reproduces the plain step from the same seed. Two real ranks
(skipped on a machine with one GPU): the tool runs, and the replicas end with bitwise equal parameters."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W = 8, 84, 216
MARGIN = 0.2


@pytest.fixture()
def rccl_comm():
    from neuralsampleid_amd import parallel, rccl
    old = os.environ.get("NSID_FORCE_COLLECTIVES")
    os.environ["NSID_FORCE_COLLECTIVES"] = "1"
    comm = rccl.init_comm(0, 1)
    parallel.set_default_comm(comm)
    yield comm
    torch.cuda.synchronize()
    parallel.set_default_comm(None)
    comm.destroy()
    if old is None:
        os.environ.pop("NSID_FORCE_COLLECTIVES", None)
    else:
        os.environ["NSID_FORCE_COLLECTIVES"] = old


def build():
    from synth import synth_state
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    from neuralsampleid_amd.optim import FusedClipAdam
    from neuralsampleid_amd.simclr.triplet import BaselineModel
    enc = ResNetIBN()
    sd = synth_state(enc.state_dict())
    sd["global_pool.p"] = torch.full((1,), 3.0)
    enc.load_state_dict(sd)
    model = BaselineModel({}, enc).to(DEV).train()
    return model, FusedClipAdam(model.parameters(), lr=1e-4, max_norm=1.0, direct_grads=False, ds_prep=False)


def pairs():
    g = torch.Generator(device=DEV).manual_seed(3)
    x_i = torch.randn(B, H, W, device=DEV, generator=g).abs() * 2 + 0.5
    return x_i, (x_i + 0.3 * torch.randn(B, H, W, device=DEV, generator=g)).abs()


def plain_step(x_i, x_j):
    from neuralsampleid_amd.simclr.triplet import baseline_objective
    model, opt = build()
    opt.zero_grad()
    _, _, z_i, z_j = model(x_i, x_j)
    loss, cls, trip = baseline_objective(z_i, z_j, margin=MARGIN)
    loss.backward()
    torch.cuda.synchronize()
    return torch.stack([loss.detach(), cls, trip]).clone(), opt.flat_g.clone()


def test_one_rank_step_equals_the_plain_step(rccl_comm):
    from neuralsampleid_amd import parallel
    x_i, x_j = pairs()
    (l0, g0), (l0b, g0b) = plain_step(x_i, x_j), plain_step(x_i, x_j)
    noise = float((g0b - g0).norm())
    print(f"  two plain steps: |g - g'| = {noise:.3g} (|g| = {float(g0.norm()):.3g}), losses equal: {torch.equal(l0, l0b)}")
    model, opt = build()
    red = parallel.GradReducer(opt.params, opt.flat_g, opt.offsets, bucket_bytes=1 << 20, uses_per_step=1).install_param_hooks()
    try:
        assert len(red.bounds) > 10
        calls0 = rccl_comm.calls
        opt.zero_grad()
        red.start_step()
        _, _, z_i, z_j = model(x_i, x_j)
        loss, cls, trip = parallel.dist_baseline_objective(z_i, z_j, margin=MARGIN)
        assert not cls.requires_grad and not trip.requires_grad
        loss.backward()
        fired_during_backward = len(red.fired)
        red.finish()
        torch.cuda.synchronize()
    finally:
        red.remove_param_hooks()
    dist_g = float((opt.flat_g - g0).norm())
    print(f"  data-parallel step: {fired_during_backward} of {len(red.bounds)} buckets fired during backward, |g_dp - g| = {dist_g:.3g}, "
          f"allowed 4 x {noise:.3g}")
    assert fired_during_backward == len(red.bounds)                   # every bucket fired from the accumulation hooks
    assert rccl_comm.calls - calls0 == len(red.bounds) + 1            # buckets + ONE all-gather of both views; no loss all-reduce
    assert torch.equal(torch.stack([loss.detach(), cls, trip]), l0)
    assert float(g0.norm()) > 0 and dist_g <= 4.0 * noise


def test_two_real_ranks_stay_in_step():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["NSID_HOST_TIMEOUT_S"] = "60"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "baseline_train_synthetic.py"), "--dp", "--gpus", "2", "--batch", "8",
                        "--steps", "2", "--only-ours", "--no-table"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stderr[-4000:]
    rec = json.loads(lines[0])
    assert rec["world"] == 2
    others = [ln.split()[-1] for ln in r.stderr.splitlines() if " param_sha256 " in ln]
    assert others == [rec["param_sha256"]], (others, rec["param_sha256"])          # the replicas stayed in step
    assert rec["loss"] == rec["loss"] and abs(rec["loss"]) < float("inf")
