"""Times the ResNet-IBN baseline's fingerprint extraction (encoder/resnet_ibn.py on csrc/resnet.hip) on one GPU, next to a torch-eager
restatement of the same forward written here from the state_dict, on the same GPU in the same call.

    python tools/resnet_ibn_bench.py [--batches 256,1024] [--clips 2048] [--reps 3] [--frames 216] [--only-ours] [--profile DIR]

Per batch size, clips/s over --clips segments of (84, --frames), wall time of the whole pass ending in a device synchronise:
  hip_fp32 / hip_bf16         extract_fingerprints (eager launches), fp32 / bf16 activation storage
  graph_fp32 / graph_bf16     the same through GraphedFingerprinter(micro_batch = batch)
  torch_fp32                  the restatement in fp32, contiguous (what the reference's own code runs: its arithmetic)
  torch_bf16_cl               the restatement in bf16, channels-last
Every configuration runs --reps times, INTERLEAVED (rep 1 of all, rep 2 of all, ...), so that clock or thermal drift hits all alike;
the JSON line holds every repetition, the median and the ratios. --only-ours skips the torch runs.

--profile DIR: additionally starts ONE child under `rocprofv3 --kernel-trace --stats` (bf16 storage, eager, batch 256, its own process:
counters and traces are never collected inside a timed run) and prints, from its kernel trace, the per-kernel table of one forward and
per convolution launch the achieved FLOP/s (FLOPs counted from the shapes, 2 x MACs) as a share of the dense bf16 MFMA peak, with the
bound that applies to the layer: matrix rate, or HBM bytes where its algorithmic bytes / 6.3 TB/s exceed its FLOPs / peak."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
from synth import synth_state  # noqa: E402
from neuralsampleid_amd import functional as F_  # noqa: E402
from neuralsampleid_amd import ops  # noqa: E402
from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN  # noqa: E402
from neuralsampleid_amd.fingerprint import GraphedFingerprinter, extract_fingerprints  # noqa: E402
from neuralsampleid_amd.simclr.triplet import BaselineModel  # noqa: E402

PEAK_BF16 = 2.5e15          # dense bf16 MFMA, FLOP/s (MI355X)
HBM_BPS = 6.3e12            # achievable HBM bytes/s
PROFILE_BATCH, PROFILE_WARMUP, PROFILE_STEPS = 256, 2, 3


# ------------------------------------------------------------------------------------------ torch-eager restatement
def _bn(x, sd, k):
    return F.batch_norm(x, sd[k + ".running_mean"], sd[k + ".running_var"], sd[k + ".weight"], sd[k + ".bias"], False, 0.0, 1e-5)


def _block(x, sd, k, stride):
    idt = x
    if k + ".downsample.0.weight" in sd:
        idt = _bn(F.conv2d(x, sd[k + ".downsample.0.weight"], stride=stride), sd, k + ".downsample.1")
    y = F.conv2d(x, sd[k + ".conv1.weight"])
    c = y.shape[1] // 2
    y = torch.cat([F.instance_norm(y[:, :c], weight=sd[k + ".bn1.IN.weight"], bias=sd[k + ".bn1.IN.bias"], eps=1e-5),
                   _bn(y[:, c:], sd, k + ".bn1.BN")], 1)
    y = F.relu(y)
    y = _bn(F.conv2d(y, sd[k + ".conv2.weight"], stride=stride, padding=1), sd, k + ".bn2")
    y = _bn(F.conv2d(y, sd[k + ".conv3.weight"]), sd, k + ".bn3")
    return F.relu(y + idt)


@torch.no_grad()
def torch_forward(sd, x, channels_last):
    """BaselineModel(ResNetIBN) in eval mode as plain torch ops on the tensors of `sd` (already in the compute dtype)"""
    x = x.unsqueeze(1)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x = F.max_pool2d(F.relu(_bn(F.conv2d(x, sd["encoder.conv1.weight"], stride=2, padding=3), sd, "encoder.bn1")), 3, 2, 1)
    for li, stride in ((1, 1), (2, 1), (3, 2), (4, 2)):
        x = _block(x, sd, f"encoder.layer{li}.0", stride)
        x = _block(x, sd, f"encoder.layer{li}.1", 1)
    p = sd["encoder.global_pool.p"]
    x = F.adaptive_avg_pool2d(x.clamp(min=1e-6).pow(p), (1, 1)).pow(1.0 / p).flatten(1)
    h = F.linear(x, sd["encoder.embedding_head.weight"], sd["encoder.embedding_head.bias"])
    return F.normalize(h.float(), p=2, eps=1e-10)


def torch_state(model, dtype, channels_last):
    sd = {}
    for k, v in model.state_dict().items():
        if not v.is_floating_point():
            continue
        v = v.detach().to(dtype)
        if channels_last and v.dim() == 4:
            v = v.contiguous(memory_format=torch.channels_last)
        sd[k] = v
    return sd


# ------------------------------------------------------------------------------------------ the model and the timed passes
def build_model(frames):
    torch.manual_seed(0)
    model = BaselineModel({"arch": "resnet-ibn", "n_frames": frames}, ResNetIBN())
    sd = synth_state(model.state_dict())
    sd["encoder.global_pool.p"] = torch.full((1,), 3.0)
    model.load_state_dict(sd)
    return model.cuda().eval()


def clips(n, frames, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, 84, frames, device="cuda", generator=g).abs() * 2


def wall_rate(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def bench(args):
    model = build_model(args.frames)
    specs = clips(args.clips, args.frames)
    for B in [int(b) for b in args.batches.split(",")]:
        runs = {}

        def hip(dt):
            def fn():
                F_.set_activation_dtype(dt)
                extract_fingerprints(model, specs, batch=B)
            return fn

        runs["hip_fp32"], runs["hip_bf16"] = hip(torch.float32), hip(torch.bfloat16)
        for name, dt in (("graph_fp32", torch.float32), ("graph_bf16", torch.bfloat16)):
            F_.set_activation_dtype(dt)
            gf = GraphedFingerprinter(model, micro_batch=B)
            runs[name] = (lambda gf=gf: gf(specs))
        if not args.only_ours:
            for name, dt, cl in (("torch_fp32", torch.float32, False), ("torch_bf16_cl", torch.bfloat16, True)):
                sd = torch_state(model, dt, cl)

                def fn(sd=sd, dt=dt, cl=cl):
                    out = torch.empty((specs.shape[0], 2048), device="cuda")
                    for lo in range(0, specs.shape[0], B):
                        out[lo:lo + B] = torch_forward(sd, specs[lo:lo + B].to(dt), cl)
                    return out
                runs[name] = fn
        for fn in runs.values():            # warm-up: allocator, code objects, cached constants, MIOpen's algorithm search
            fn()
        torch.cuda.synchronize()
        rates = {k: [] for k in runs}
        for _ in range(args.reps):
            for k, fn in runs.items():
                rates[k].append(round(wall_rate(fn, specs.shape[0]), 1))
        rec = {"batch": B, "frames": args.frames, "clips": args.clips, "reps": args.reps, "clips_s_all": rates,
               "clips_s": {k: float(np.median(v)) for k, v in rates.items()}}
        med = rec["clips_s"]
        if not args.only_ours:
            # agreement of the two sides on the first batch (the restatement is the yardstick: it must compute the same thing)
            F_.set_activation_dtype(torch.float32)
            z = extract_fingerprints(model, specs[:B], batch=B)
            zt = torch_forward(torch_state(model, torch.float32, False), specs[:B], False)
            rec["max_dz_hip_fp32_vs_torch_fp32"] = float((z - zt).abs().max())
            rec["ratios"] = {"hip_bf16/torch_fp32": round(med["hip_bf16"] / med["torch_fp32"], 2),
                             "hip_bf16/torch_bf16_cl": round(med["hip_bf16"] / med["torch_bf16_cl"], 2),
                             "graph_bf16/torch_fp32": round(med["graph_bf16"] / med["torch_fp32"], 2),
                             "hip_fp32/torch_fp32": round(med["hip_fp32"] / med["torch_fp32"], 2)}
            # the gate: bf16-storage extraction not slower than torch-eager fp32 beyond the spread of the interleaved repetitions
            rec["gate_hip_bf16_not_slower_than_torch_fp32"] = bool(max(rates["hip_bf16"]) >= min(rates["torch_fp32"]))
        print(json.dumps(rec), flush=True)
        del runs
        torch.cuda.empty_cache()
    F_.set_activation_dtype(torch.float32)


# ------------------------------------------------------------------------------------------ the profiled child and its table
def conv_launches(B, frames):
    """(label, FLOPs, algorithmic bytes in bf16) of the 18 nsid_conv2d_fwd launches of one forward, in launch order"""
    H = ops.conv_out_size(ops.conv_out_size(84, 7, 2), 3, 2)
    W = ops.conv_out_size(ops.conv_out_size(frames, 7, 2), 3, 2)
    out = []

    def add(label, H, W, C, Co, k, s, res):
        Ho, Wo = ops.conv_out_size(H, k, s), ops.conv_out_size(W, k, s)
        M = B * Ho * Wo
        out.append((label, 2.0 * M * Co * k * k * C, 2.0 * (B * H * W * C + Co * k * k * C + M * Co * (2 if res else 1))))
        return Ho, Wo

    for li, (C, s) in enumerate(((128, 1), (256, 1), (512, 2), (1024, 2)), 1):
        for bi in range(2):
            st = s if bi == 0 else 1
            if bi == 0 and st == 2:
                add(f"layer{li}.0.downsample 1x1 s2 {C // 2}->{C}", H, W, C // 2, C, 1, 2, False)
            Ho, Wo = add(f"layer{li}.{bi}.conv2 3x3 s{st} {C}", H, W, C, C, 3, st, False)
            add(f"layer{li}.{bi}.conv3 1x1 +res {C}", Ho, Wo, C, C, 1, 1, True)
            H, W = Ho, Wo
    return out


def profile_child(args):
    F_.set_activation_dtype(torch.bfloat16)
    model = build_model(args.frames)
    specs = clips(PROFILE_BATCH, args.frames)
    for _ in range(PROFILE_WARMUP + PROFILE_STEPS):
        extract_fingerprints(model, specs, batch=PROFILE_BATCH)
    torch.cuda.synchronize()


def profile(args):
    os.makedirs(args.profile, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.profile, "--", sys.executable,
           os.path.abspath(__file__), "--profile-child", "--frames", str(args.frames)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        print("profile: rocprofv3 child failed (per-kernel table not measured):\n" + r.stderr[-2000:])
        return
    rows = []
    for f in glob.glob(args.profile + "/**/*kernel_trace.csv", recursive=True):
        for row in csv.DictReader(open(f)):
            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    convs = [r for r in rows if "conv2d_kernel" in r[2]]          # the forward instantiation conv2d_kernel<T, false>: nothing else runs here
    plan = conv_launches(PROFILE_BATCH, args.frames)
    n = len(plan)
    if len(convs) != n * (PROFILE_WARMUP + PROFILE_STEPS):
        print(f"profile: {len(convs)} convolution launches in the trace, expected {n * (PROFILE_WARMUP + PROFILE_STEPS)}: not measured")
        return
    first = convs[n * PROFILE_WARMUP][0]
    stems = [i for i, r in enumerate(rows) if "stem7_pool_kernel" in r[2]]
    sel = rows[stems[PROFILE_WARMUP]:]
    acc = {}
    for s, e, name in sel:
        m = re.match(r"_ZN\d+_GLOBAL__N_1\d+([a-z0-9_]+_kernel)I(DF16b|f)(?:Lb[01]E)?E", name)        # a mangled anonymous-namespace template
        if m:
            name = f"{m.group(1)}<{'bf16' if m.group(2) == 'DF16b' else 'float'}>"
        name = re.sub(r"\(anonymous namespace\)::|^void ", "", name)
        name = re.sub(r"\(.*\)$", "", name).replace(" ", "")
        a = acc.setdefault(name, [0, 0])
        a[0] += 1
        a[1] += e - s
    tot = sum(t for _, t in acc.values())
    print(f"per forward of {PROFILE_BATCH} clips, bf16 storage, eager (mean of {PROFILE_STEPS}): sum of kernel durations "
          f"{tot / 1e6 / PROFILE_STEPS:.2f} ms = {PROFILE_BATCH * PROFILE_STEPS / (tot / 1e9):.0f} clips/s if back to back")
    for name, (c, t) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
        print(f"  {name[:100]:100s} x{c / PROFILE_STEPS:5.1f}  {t / 1e3 / PROFILE_STEPS:9.1f} us  {100.0 * t / tot:5.1f} %")
    print("convolution launches (nsid_conv2d_fwd), mean over the timed forwards:")
    timed = [r for r in convs if r[0] >= first]
    for i, (label, flops, nbytes) in enumerate(plan):
        us = np.mean([(e - s) / 1e3 for s, e, _ in timed[i::n]])
        bound = "HBM bytes" if nbytes / HBM_BPS > flops / PEAK_BF16 else "matrix rate"
        print(f"  {label:42s} {us:8.1f} us  {flops / us / 1e6:7.1f} TFLOP/s = {100.0 * flops / (us * 1e-6) / PEAK_BF16:4.1f} % of the dense bf16 "
              f"peak  {nbytes / us / 1e3:7.0f} GB/s  bound: {bound}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=216)
    ap.add_argument("--only-ours", action="store_true")
    ap.add_argument("--profile", default=None, metavar="DIR")
    ap.add_argument("--profile-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.profile_child:
        return profile_child(args)
    bench(args)
    if args.profile:
        profile(args)


if __name__ == "__main__":
    main()
