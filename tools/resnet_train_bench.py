"""Times one training-mode forward + backward of the ResNet-IBN trunk (ResNetIBN.trunk_train: the eight residual blocks and the
pooling head, from the stem's output rows) on one GPU, next to a torch-eager restatement of the same layers written here from the
state_dict, on the same GPU in the same call.

    python tools/resnet_train_bench.py [--batch 256] [--map 21,54] [--reps 5] [--only-ours] [--no-table]

Milliseconds per forward + backward (wall time ending in a device synchronise) of
  hip_fp32 / hip_bf16         trunk_train + backward, fp32 / bf16 activation storage
  torch_fp32                  the restatement in fp32, contiguous (the reference's own arithmetic), autograd backward
  torch_bf16_cl               the restatement in bf16, channels-last
Every configuration runs --reps times, INTERLEAVED; the JSON line holds every repetition, the medians and the ratios (torch / hip:
above 1 the kernels of this library are faster).

Then, under bf16 and under fp32 storage, the per-kernel table of one forward + backward from HIP events around every launch
(ops.KernelProfile; the events serialise the launches, so the rows do not add up to the wall time above), and for every convolution
of the trunk that runs on nsid_conv2d_fwd the backward-data and weight-gradient launch next to the forward launch of the same shape,
which does the same FLOPs; likewise nsid_ibn_relu_bwd next to nsid_ibn_relu_fwd."""
import argparse
import json
import os
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

LAYERS = (("layer1.0", 1), ("layer1.1", 1), ("layer2.0", 1), ("layer2.1", 1), ("layer3.0", 2), ("layer3.1", 1), ("layer4.0", 2),
          ("layer4.1", 1))


# ------------------------------------------------------------------------------------------ torch-eager restatement (training mode)
def _bn(x, sd, k):
    # batch statistics; the running statistics of the copy move as they do in training
    return F.batch_norm(x, sd[k + ".running_mean"], sd[k + ".running_var"], sd[k + ".weight"], sd[k + ".bias"], True, 0.1, 1e-5)


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


def torch_trunk(sd, x):
    for k, stride in LAYERS:
        x = _block(x, sd, k, stride)
    p = sd["global_pool.p"]
    x = F.adaptive_avg_pool2d(x.clamp(min=1e-6).pow(p), (1, 1)).pow(1.0 / p).flatten(1)
    return F.linear(x, sd["embedding_head.weight"], sd["embedding_head.bias"])


def torch_state(model, dtype, channels_last):
    sd = {}
    for k, v in model.state_dict().items():
        if not v.is_floating_point():
            continue
        v = v.detach().clone().to(dtype)
        if channels_last and v.dim() == 4:
            v = v.contiguous(memory_format=torch.channels_last)
        if not k.endswith(("running_mean", "running_var")) and not k.startswith(("conv1.", "bn1.")):
            v.requires_grad_(True)
        sd[k] = v
    return sd


# ------------------------------------------------------------------------------------------ the model and the timed passes
def build_model():
    torch.manual_seed(0)
    model = ResNetIBN()
    sd = synth_state(model.state_dict())
    sd["global_pool.p"] = torch.full((1,), 3.0)
    model.load_state_dict(sd)
    return model.cuda().train()


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def hip_step(model, rows, dh, B, H, W):
    for p in model.parameters():
        p.grad = None
    rows.grad = None
    model.trunk_train(rows, B, H, W).backward(dh)


def torch_step(sd, x, dh):
    for v in sd.values():
        v.grad = None
    x.grad = None
    torch_trunk(sd, x).backward(dh)


def conv_plan(B, H, W):
    """(label, H, W, C, Cout, ksize, stride) of the trunk's nsid_conv2d_fwd launches (conv2 of every block, the stride-2 downsamples)"""
    out = []
    for li, (C, s) in enumerate(((128, 1), (256, 1), (512, 2), (1024, 2)), 1):
        for bi in range(2):
            st = s if bi == 0 else 1
            if bi == 0 and st == 2:
                out.append((f"layer{li}.0.downsample 1x1 s2 {C // 2}->{C}", H, W, C // 2, C, 1, 2))
            out.append((f"layer{li}.{bi}.conv2 3x3 s{st} {C}", H, W, C, C, 3, st))
            H, W = ops.conv_out_size(H, 3, st), ops.conv_out_size(W, 3, st)
    return out


def kernel_table(model, rows, dh, B, H, W, label):
    hip_step(model, rows, dh, B, H, W)
    torch.cuda.synchronize()
    ops.PROFILE = ops.KernelProfile()
    try:
        ops.KernelProfile.plug()
        hip_step(model, rows, dh, B, H, W)
        recs = ops.PROFILE.by_shape()
        total = sum(v["ms"] for v in ops.PROFILE.summary().values())
    finally:
        ops.PROFILE = None
    print(f"per-kernel table, {label} storage, one forward + backward of {B} clips on {H}x{W} rows "
          f"(sum of the bracketed launches {total:.2f} ms):")
    agg = {}
    for r in recs:
        a = agg.setdefault(r["kernel"], [0, 0.0])
        a[0] += r["launches"]
        a[1] += r["total_ms"]
    for name, (n, ms) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print(f"  {name[:72]:72s} x{n:4d} {1e3 * ms:10.1f} us {100.0 * ms / total:5.1f} %")
    by = {(r["kernel"], r["M"], r["Nout"], r["K"]): r for r in recs}
    print(f"convolution backward next to the forward of the same shape ({label}; us, TFLOP/s; ratio = backward / forward time):")
    for name, h, w, C, Co, k, s in conv_plan(B, H, W):
        ho, wo = ops.conv_out_size(h, k, s), ops.conv_out_size(w, k, s)
        tag = "<%dx%d,s%d>" % (k, k, s)
        f = by.get(("conv2d_fwd_kernel" + tag, B * ho * wo, Co, k * k * C))
        d = by.get(("conv2d_bwd_data_kernel" + tag, B * h * w, C, k * k * Co))
        g = by.get(("conv2d_wgrad_kernel" + tag, B * ho * wo, Co, k * k * C))
        if not (f and d and g):
            print(f"  {name:40s} not all three launches found in the profile")
            continue
        print(f"  {name:40s} fwd {f['avg_us']:8.1f} ({f['tflops']:6.1f})  bwd-data {d['avg_us']:8.1f} ({d['tflops']:6.1f}) "
              f"x{d['avg_us'] / f['avg_us']:.2f}  bwd-weight {g['avg_us']:8.1f} ({g['tflops']:6.1f}) x{g['avg_us'] / f['avg_us']:.2f}")
    print(f"IBN + ReLU backward next to its forward ({label}; us; the forward also runs once more inside the backward, to recompute y1):")
    for r in recs:
        if r["kernel"] == "ibn_relu_bwd_kernel":
            f = by.get(("ibn_relu_kernel", r["M"], r["Nout"], r["K"]))
            if f:
                print(f"  rows {r['M']:7d} C {r['Nout']:5d}  fwd {f['avg_us']:8.1f}  bwd (3 launches) {r['avg_us']:8.1f}  x{r['avg_us'] / f['avg_us']:.2f}")


def bench(args):
    B = args.batch
    H, W = (int(v) for v in args.map.split(","))
    model = build_model()
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, 64, H, W, device="cuda", generator=g).abs()
    dh = torch.randn(B, 2048, device="cuda", generator=g) / 32
    runs, keep = {}, {}
    for name, dt in (("hip_fp32", torch.float32), ("hip_bf16", torch.bfloat16)):
        rows = x.permute(0, 2, 3, 1).reshape(B * H * W, 64).to(dt).contiguous().requires_grad_(True)
        keep[name] = rows
        runs[name] = (lambda rows=rows: hip_step(model, rows, dh, B, H, W))
    if not args.only_ours:
        for name, dt, cl in (("torch_fp32", torch.float32, False), ("torch_bf16_cl", torch.bfloat16, True)):
            sd = torch_state(model, dt, cl)
            xt = x.to(dt)
            if cl:
                xt = xt.contiguous(memory_format=torch.channels_last)
            xt.requires_grad_(True)
            runs[name] = (lambda sd=sd, xt=xt, dt=dt: torch_step(sd, xt, dh.to(dt)))
    for fn in runs.values():                # warm-up: allocator, code objects, cached constants, MIOpen's algorithm search
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            ms[k].append(round(wall_ms(fn), 3))
    rec = {"batch": B, "map": [H, W], "reps": args.reps, "ms_all": ms, "ms": {k: float(np.median(v)) for k, v in ms.items()}}
    med = rec["ms"]
    if not args.only_ours:
        rec["ratios"] = {"torch_fp32/hip_fp32": round(med["torch_fp32"] / med["hip_fp32"], 2),
                         "torch_fp32/hip_bf16": round(med["torch_fp32"] / med["hip_bf16"], 2),
                         "torch_bf16_cl/hip_bf16": round(med["torch_bf16_cl"] / med["hip_bf16"], 2)}
    print(json.dumps(rec), flush=True)
    if not args.no_table:
        kernel_table(model, keep["hip_bf16"], dh, B, H, W, "bf16")
        kernel_table(model, keep["hip_fp32"], dh, B, H, W, "fp32")
    F_.set_activation_dtype(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--map", default="21,54")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-ours", action="store_true")
    ap.add_argument("--no-table", action="store_true")
    bench(ap.parse_args())


if __name__ == "__main__":
    main()
