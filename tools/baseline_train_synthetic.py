"""The ResNet-IBN baseline's training step (baseline/train.py:50-92 of the reference) on synthetic (84, 216) CQT segment pairs, on one
GPU: model.train()(x_i, x_j), baseline_objective, backward, FusedClipAdam(max_norm=1.0); next to a torch-eager restatement of the same
step written here from the state_dict (as tools/resnet_train_bench.py does for the trunk), on the same GPU in the same call.

    python tools/baseline_train_synthetic.py [--batch 256] [--steps 10] [--bf16] [--reps 5] [--only-ours] [--no-table] [--augment [--from-bank]]
    python tools/baseline_train_synthetic.py --dp [--gpus N] [--batch 256] [--steps 10] [--bf16]

--dp runs the data-parallel step instead, one process per GPU, --batch pairs per rank: parallel.dist_baseline_objective (one all-gather
of the embeddings, the objective of the global batch on every rank, the backward for the rank's own pairs) and a GradReducer on
autograd's accumulation hooks (bucketed SUM all-reduce under backward). It runs under the torchrun environment contract
(parallel.init_from_env("rccl")); with --gpus N and no launcher in the environment it starts the N ranks itself as fresh child
processes (at most 16; this process makes no GPU call). NSID_FORCE_COLLECTIVES=1 with one rank is the single-GPU rehearsal of the
collective path. Rank 0 prints one JSON line (ms per step, pairs per second, world, the loss parts, the SHA-256 of the flat parameter
buffer after the last step); every other rank prints its digest on stderr: equal digests mean the replicas stayed in step.

--augment runs the loop of baseline/train.py from raw stems instead: synthetic (B, 110 250) stem pairs on the GPU, a fresh draw of
GPUBaselineWaveAugment per step (the only host work: random numbers and the EQ filter design), GPUTransformCQT(train=True), the step;
it prints the loss parts and the milliseconds of augmentation, front end and step, and stops there (no interleaved timing).

Prints the loss parts of --steps training steps (fp32 activation storage, or bf16 with --bf16) and their ms per step; then times
  hip_fp32 / hip_bf16         the whole step, fp32 / bf16 activation storage
  torch_fp32                  the restatement in fp32, contiguous, torch.optim.Adam + clip_grad_norm_
  torch_bf16_cl               the restatement in bf16, channels-last
  stem_hip_fp32 / _bf16       the stem alone: stem_train + backward (three launch families: stem7_stat + bn_finalize, the folded
                              forward, stem7_bwd)
  stem_torch_fp32 / _bf16_cl  torch-eager on the same four layers (conv 7x7, BatchNorm, ReLU, max-pool), forward + backward
--reps times each, INTERLEAVED (one JSON line: every repetition, medians, min / max); then the per-kernel table of the stem launches
of one step from HIP events around every launch (ops.KernelProfile), under both storages."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from resnet_train_bench import torch_trunk, wall_ms  # noqa: E402
from synth import synth_state  # noqa: E402
from neuralsampleid_amd import functional as F_  # noqa: E402
from neuralsampleid_amd import ops  # noqa: E402
from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN  # noqa: E402
from neuralsampleid_amd.optim import FusedClipAdam  # noqa: E402
from neuralsampleid_amd.simclr.triplet import BaselineModel, baseline_objective  # noqa: E402

MARGIN = 0.2


# ------------------------------------------------------------------------------------------ torch-eager restatement of the step
def torch_stem(sd, x):
    y = F.conv2d(x.unsqueeze(1), sd["conv1.weight"], stride=2, padding=3)
    y = F.batch_norm(y, sd["bn1.running_mean"], sd["bn1.running_var"], sd["bn1.weight"], sd["bn1.bias"], True, 0.1, 1e-5)
    return F.max_pool2d(F.relu(y), 3, 2, 1)


def torch_state(model, dtype, channels_last):
    sd = {}
    for k, v in model.encoder.state_dict().items():
        if not v.is_floating_point():
            continue
        v = v.detach().clone().to(dtype)
        if channels_last and v.dim() == 4:
            v = v.contiguous(memory_format=torch.channels_last)
        if not k.endswith(("running_mean", "running_var")):
            v.requires_grad_(True)
        sd[k] = v
    return sd


def torch_losses(z_i, z_j, margin=MARGIN):
    """simclr/triplet.py of the reference: pair cross-entropy + semi-hard triplet loss, in fp32"""
    z = torch.cat([z_i, z_j]).float()
    M = z.shape[0]
    S = (z @ z.T).masked_fill(torch.eye(M, dtype=torch.bool, device=z.device), -float("inf"))
    cls = F.cross_entropy(S, (torch.arange(M, device=z.device) + M // 2) % M)
    e = F.normalize(z, dim=1)
    sim = e @ e.T
    labels = torch.cat([torch.arange(M // 2), torch.arange(M // 2)]).to(z.device).unsqueeze(1)
    match = labels == labels.T
    pos = sim.masked_fill(~(match & ~torch.eye(M, dtype=torch.bool, device=z.device)), -float("inf")).max(dim=1).values
    neg = sim.masked_fill(match, -float("inf"))
    semi = neg.masked_fill(~(neg > pos.unsqueeze(1) - margin), float("inf")).min(dim=1).values
    valid = ~torch.isinf(semi)
    trip = F.relu(pos[valid] - semi[valid] + margin).mean() if bool(valid.any()) else sim.sum() * 0.0
    return cls, trip


def torch_step(sd, params, opt, x_i, x_j, cl):
    opt.zero_grad(set_to_none=True)
    zs = []
    for x in (x_i, x_j):
        y = torch_stem(sd, x)
        if cl:
            y = y.contiguous(memory_format=torch.channels_last)
        zs.append(F.normalize(torch_trunk(sd, y).float(), p=2, dim=1, eps=1e-10))
    cls, trip = torch_losses(zs[0], zs[1])
    (cls + trip).backward()
    torch.nn.utils.clip_grad_norm_(params, 1.0)
    opt.step()


def torch_stem_step(sd, x, dy):
    for k in ("conv1.weight", "bn1.weight", "bn1.bias"):
        sd[k].grad = None
    torch_stem(sd, x).backward(dy)


# ------------------------------------------------------------------------------------------ the step of this library
def build_model():
    torch.manual_seed(0)
    enc = ResNetIBN()
    sd = synth_state(enc.state_dict())
    sd["global_pool.p"] = torch.full((1,), 3.0)
    enc.load_state_dict(sd)
    return BaselineModel({}, enc).cuda().train()


def hip_step(model, opt, x_i, x_j):
    opt.zero_grad()
    _, _, z_i, z_j = model(x_i, x_j)
    loss, cls, trip = baseline_objective(z_i, z_j, margin=MARGIN)
    loss.backward()
    opt.step()
    return loss, cls, trip


def hip_stem_step(model, x, drows):
    for p in (model.encoder.conv1.weight, model.encoder.bn1.weight, model.encoder.bn1.bias):
        p.grad = None
    rows, _, _ = model.encoder.stem_train(x)
    rows.backward(drows)


def synth_pairs(B, H=84, W=216, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x_i = torch.randn(B, H, W, device="cuda", generator=g).abs() * 2 + 0.5
    x_j = (x_i + 0.3 * torch.randn(B, H, W, device="cuda", generator=g)).abs()
    return x_i, x_j


def stem_table(model, opt, x_i, x_j, label):
    hip_step(model, opt, x_i, x_j)
    torch.cuda.synchronize()
    ops.PROFILE = ops.KernelProfile()
    try:
        ops.KernelProfile.plug()
        hip_step(model, opt, x_i, x_j)
        summ = ops.PROFILE.summary()
    finally:
        ops.PROFILE = None
    total = sum(v["ms"] for v in summ.values())
    print(f"per-kernel table, {label} storage, one training step of {x_i.shape[0]} pairs (sum of the bracketed launches {total:.2f} ms); "
          "the stem's launches:")
    for name, v in sorted(summ.items(), key=lambda kv: -kv[1]["ms"]):
        if name.startswith("stem7_"):
            print(f"  {name:32s} x{v['launches']:3d} {1e3 * v['ms']:10.1f} us {100.0 * v['ms'] / total:5.1f} %")
    print("  every launch family of the step:")
    for name, v in sorted(summ.items(), key=lambda kv: -kv[1]["ms"])[:14]:
        print(f"  {name[:60]:60s} x{v['launches']:4d} {1e3 * v['ms']:10.1f} us {100.0 * v['ms'] / total:5.1f} %")


def run_from_stems(args):
    """baseline/train.py's loop from waveforms: augment -> CQT -> step, nothing of the signal path on the host"""
    from baseline_augment_bench import CFG, L, synth_stems
    from neuralsampleid_amd.modules.transformations import GPUBaselineWaveAugment, GPUTransformCQT
    B = args.batch
    F_.set_activation_dtype(torch.bfloat16 if args.bf16 else torch.float32)
    model = build_model()
    opt = FusedClipAdam(model.parameters(), lr=args.lr, max_norm=1.0, direct_grads=False, ds_prep=False)
    gen = torch.Generator().manual_seed(11)
    augment, front = GPUBaselineWaveAugment(CFG, generator=gen), GPUTransformCQT(CFG, train=True)
    sampler = None
    if args.from_bank:
        from stem_pairs_bench import BASELINE_CFG, synth_bank
        from neuralsampleid_amd.modules.data import GPUStemPairSampler
        sampler = GPUStemPairSampler(BASELINE_CFG, synth_bank(BASELINE_CFG, tracks=4, seconds=30.0))      # built once
        assert sampler.L == L
    else:
        x_i, x_j = synth_stems(B)
    for step in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if sampler is not None:                       # the dataset's __getitem__ for the batch: stems -> (x_i, x_j), on the device
            x_i, x_j, n_ok = sampler.batch(B, generator=gen)
        params = augment.draw(B, generator=gen, device="cuda", L=L)
        t1 = time.perf_counter()
        a_i, a_j = augment(x_i, x_j, params)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        X_i, X_j = front(a_i, a_j)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        loss, cls, trip = hip_step(model, opt, X_i, X_j)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        assert X_i.shape == (B, 84, 216) and bool(torch.isfinite(X_i).all())
        print(f"step {step:3d} | loss {float(loss):.4f} | cls {float(cls):.4f} | triplet {float(trip):.4f} | grad norm "
              f"{float(opt.grad_norm):.3f} | {'sampler.batch + ' if sampler is not None else ''}draw (host) {1e3 * (t1 - t0):7.2f} ms | augment {1e3 * (t2 - t1):7.2f} ms | CQT "
              f"{1e3 * (t3 - t2):6.2f} ms | step {1e3 * (t4 - t3):7.2f} ms", flush=True)
    F_.set_activation_dtype(torch.float32)


# ------------------------------------------------------------------------------------------ the data-parallel step
MAX_RANKS = 16


def spawn_dp_ranks(n):
    """--dp --gpus N without a launcher: N fresh child ranks through torch.distributed.run (this process has made no GPU call); rank
    0's JSON line is relayed; non-zero if a rank fails or the job overruns NSID_BENCH_TIMEOUT_S"""
    import signal
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    deadline = float(os.environ.get("NSID_BENCH_TIMEOUT_S", "900"))
    print(f"[nsid] no launcher in the environment: spawning {n} ranks through torch.distributed.run", file=sys.stderr, flush=True)
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, _ = proc.communicate(timeout=deadline)
    except subprocess.TimeoutExpired:
        print(f"[nsid] the {n}-rank job did not finish within {deadline:.0f} s: terminating its process group", file=sys.stderr, flush=True)
        os.killpg(proc.pid, signal.SIGTERM)
        try:
            proc.wait(timeout=20)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)
            proc.wait()
        return 124
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    if proc.returncode == 0 and len(lines) == 1:
        print(lines[0], flush=True)
        return 0
    sys.stderr.write(out)
    print(f"[nsid] launcher exit code {proc.returncode}, {len(lines)} JSON lines", file=sys.stderr, flush=True)
    return proc.returncode or 1


def dp_step(model, opt, red, x_i, x_j):
    from neuralsampleid_amd import parallel
    opt.zero_grad()
    red.start_step()
    _, _, z_i, z_j = model(x_i, x_j)
    loss, cls, trip = parallel.dist_baseline_objective(z_i, z_j, margin=MARGIN)
    loss.backward()                 # every bucket's all-reduce is launched from the accumulation hooks, under the rest of backward
    early = len(red.fired)
    red.finish()                    # the compute stream waits for the communicator's
    opt.step()
    return loss, cls, trip, early


def run_dp(args):
    import hashlib
    from neuralsampleid_amd import parallel
    rank, local, world = parallel.init_from_env("rccl")
    B = args.batch                                          # pairs per rank
    x_i, x_j = synth_pairs(B, seed=3 + rank)                # every rank owns its own clips
    F_.set_activation_dtype(torch.bfloat16 if args.bf16 else torch.float32)
    model = build_model()                                   # the same seed on every rank: identical replicas, no parameter broadcast
    opt = FusedClipAdam(model.parameters(), lr=args.lr, max_norm=1.0, direct_grads=False, ds_prep=False)
    red = parallel.GradReducer(opt.params, opt.flat_g, opt.offsets, bucket_bytes=16 << 20, uses_per_step=1).install_param_hooks()
    ms, loss = [], None
    for step in range(args.steps):
        parallel.sync_with_deadline(what=f"the work before step {step}")
        t0 = time.perf_counter()
        loss, cls, trip, early = dp_step(model, opt, red, x_i, x_j)
        parallel.sync_with_deadline(what=f"step {step}")
        ms.append(1e3 * (time.perf_counter() - t0))
        loss = loss.detach()
        print(f"[nsid] rank {rank} step {step:3d} | loss {float(loss):.4f} | cls {float(cls):.4f} | triplet {float(trip):.4f} | grad norm "
              f"{float(opt.grad_norm):.3f} | {ms[-1]:8.2f} ms", file=sys.stderr, flush=True)
    red.remove_param_hooks()
    digest = hashlib.sha256(opt.flat_p.cpu().numpy().tobytes()).hexdigest()
    timed = ms[1:] if len(ms) > 1 else ms                   # the first step pays for code objects, the allocator and RCCL's setup
    per_step = float(np.median(timed))
    if rank == 0:
        print(json.dumps({"bench": "baseline data-parallel step", "world": world, "batch_per_rank": B, "segment": [84, 216],
                          "storage": "bf16" if args.bf16 else "fp32", "steps": args.steps, "ms_per_step": round(per_step, 3),
                          "pairs_per_s": round(world * B / (per_step * 1e-3), 1), "ms_all": [round(v, 3) for v in ms],
                          "loss": float(loss), "loss_cls": float(cls), "loss_trip": float(trip), "buckets": len(red.bounds),
                          "buckets_fired_in_backward": early,
                          "collectives": parallel.COMM is not None, "param_sha256": digest}), flush=True)
    else:
        print(f"[nsid] rank {rank} param_sha256 {digest}", file=sys.stderr, flush=True)
    F_.set_activation_dtype(torch.float32)
    parallel.shutdown()


def run(args):
    if args.dp:
        return run_dp(args)
    if args.augment:
        return run_from_stems(args)
    B = args.batch
    x_i, x_j = synth_pairs(B)
    # the training loop itself
    dt = torch.bfloat16 if args.bf16 else torch.float32
    F_.set_activation_dtype(dt)
    model = build_model()
    opt = FusedClipAdam(model.parameters(), lr=args.lr, max_norm=1.0, direct_grads=False, ds_prep=False)
    for step in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss, cls, trip = hip_step(model, opt, x_i, x_j)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        print(f"step {step:3d} | loss {float(loss):.4f} | cls {float(cls):.4f} | triplet {float(trip):.4f} | grad norm "
              f"{float(opt.grad_norm):.3f} | {ms:8.2f} ms", flush=True)
    if args.reps <= 0:
        return
    # interleaved timing
    Hp, Wp = 21, 54
    g = torch.Generator(device="cuda").manual_seed(5)
    runs = {}
    hip = {}
    for name, sdt in (("hip_fp32", torch.float32), ("hip_bf16", torch.bfloat16)):
        m = build_model()
        o = FusedClipAdam(m.parameters(), lr=args.lr, max_norm=1.0, direct_grads=False, ds_prep=False)
        hip[name] = (m, o, sdt)

        def whole(m=m, o=o, sdt=sdt):
            F_.set_activation_dtype(sdt)
            hip_step(m, o, x_i, x_j)
        runs[name] = whole
        drows = torch.randn(B * Hp * Wp, 64, device="cuda", generator=g).to(sdt)

        def stem(m=m, sdt=sdt, drows=drows):
            F_.set_activation_dtype(sdt)
            hip_stem_step(m, x_i, drows)
        runs["stem_" + name] = stem
    if not args.only_ours:
        for name, tdt, cl in (("torch_fp32", torch.float32, False), ("torch_bf16_cl", torch.bfloat16, True)):
            sd = torch_state(hip["hip_fp32"][0], tdt, cl)
            params = [v for v in sd.values() if v.requires_grad]
            topt = torch.optim.Adam(params, lr=args.lr)
            xi, xj = x_i.to(tdt), x_j.to(tdt)
            runs[name] = (lambda sd=sd, params=params, topt=topt, xi=xi, xj=xj, cl=cl: torch_step(sd, params, topt, xi, xj, cl))
            dy = torch.randn(B, 64, Hp, Wp, device="cuda", generator=g).to(tdt)
            if cl:
                dy = dy.contiguous(memory_format=torch.channels_last)
            runs["stem_" + name] = (lambda sd=sd, xi=xi, dy=dy: torch_stem_step(sd, xi, dy))
    for fn in runs.values():                # warm-up: allocator, code objects, cached constants, MIOpen's algorithm search
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            ms[k].append(round(wall_ms(fn), 3))
    rec = {"batch": B, "segment": [84, 216], "reps": args.reps, "ms_all": ms,
           "ms": {k: float(np.median(v)) for k, v in ms.items()}, "min_max": {k: [min(v), max(v)] for k, v in ms.items()}}
    print(json.dumps(rec), flush=True)
    if not args.no_table:
        for name, label in (("hip_bf16", "bf16"), ("hip_fp32", "fp32")):
            m, o, sdt = hip[name]
            F_.set_activation_dtype(sdt)
            stem_table(m, o, x_i, x_j, label)
    F_.set_activation_dtype(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-ours", action="store_true")
    ap.add_argument("--no-table", action="store_true")
    ap.add_argument("--augment", action="store_true", help="run the loop from raw stems: GPUBaselineWaveAugment, GPUTransformCQT, the step")
    ap.add_argument("--from-bank", action="store_true",
                    help="with --augment: cut every batch from a synthetic StemBank with GPUStemPairSampler.batch instead of fixed stems")
    ap.add_argument("--dp", action="store_true", help="the data-parallel step: dist_baseline_objective and a GradReducer on autograd's hooks")
    ap.add_argument("--gpus", type=int, default=1, help="with --dp and no launcher in the environment: start this many ranks")
    args = ap.parse_args()
    if args.from_bank and not args.augment:
        ap.error("--from-bank feeds the augmenter: add --augment")
    if args.dp and args.augment:
        ap.error("--dp runs the step on synthetic CQT segments: drop --augment")
    if args.gpus != 1 and not args.dp:
        ap.error("--gpus starts data-parallel ranks: add --dp")
    if not 1 <= args.gpus <= MAX_RANKS:
        ap.error(f"--gpus: 1 to {MAX_RANKS} ranks")
    if args.dp and args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(spawn_dp_ranks(args.gpus))
    run(args)


if __name__ == "__main__":
    main()
