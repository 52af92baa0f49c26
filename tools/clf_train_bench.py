"""Times one classifier training step (downstream.train_step: mining, forward, BCE, backward, Adam) from fixed features, next to the
reference's step in torch-eager fp32 on the same GPU with the same pairs and dropout masks, and the encoder forward that supplies the
features.

    python tools/clf_train_bench.py [--sizes 32,256,1024] [--reps 7] [--only-ours] [--in-dim 512|640|768|1024] [--nodes 32] [--kernels]

Per size: ms per step (median of --reps after two warm-up steps, device events around each step), the step's FLOPs from shapes
(per pair 1.05 MFLOP attention forward + 2.2 MFLOP backward: A is stored, not recomputed, plus the per-segment projections and the tail's linears and their
backward) and the speed-up. The eager step is downstream.py:119-134: the per-row argsort mining loop, x_all[hn.view(-1)], two
nn.MultiheadAttention classifier calls with the same keep masks, BCE + BCE, backward, torch.optim.Adam. One JSON line per size.
--only-ours runs just the HIP step (a rocprofv3 --kernel-trace --stats run uses it for the attention kernels' share of the peak).
--nodes N (1 .. 128, default 32): the nodes per segment of both steps; above 32 the HIP step runs the multi-tile attention kernels
(downstream.clf_train_scores_n) and the eager module attends over N nodes, with num_nodes = N in both. The HIP and the eager
repetitions of a size are interleaved in rounds (one warm round first), so a drift of the device reaches both alike. --kernels adds
one more HIP step per size under ops.KernelProfile and prints its classifier kernels (event pairs behind a plug: per-launch
microseconds, TFLOP/s and algorithmic GB/s from the shape formulas of ops.py)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
from neuralsampleid_amd import downstream  # noqa: E402
from neuralsampleid_amd.classifier import CrossAttentionClassifier  # noqa: E402

PEAK_TF = 155.0
N, K = 32, 3


def step_flops(B, C):
    """forward + backward FLOPs of one step at batch B and width C (mining excluded: 2 B 2B d)"""
    P, Sq, Sc = (1 + K) * B, B, 2 * B
    proj = 2.0 * (Sq * N * C * C + Sc * N * 2 * C * C)                  # Q, [K | V]
    tail = 2.0 * P * (C * C + C * 128)                                   # out_proj, fc.0
    attn_f = P * (2.0 * N * N * C + 2.0 * N * C)                         # ~1.05 MFLOP per pair
    attn_b = P * (4.0 * N * N * C + 2.0 * N * C + 2.0 * N * C)          # dQ, dK, da, dV
    return 3.0 * (proj + tail) + attn_f + attn_b                         # proj / tail: forward, backward-data, weight gradient


def timed_interleaved(fns, reps):
    """per fn (median ms, all ms): rounds of one call of each fn in turn, the first two rounds warm-up"""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return [(float(np.median(m)), [round(x, 3) for x in m]) for m in ms]


def kernel_rows(step):
    """one step under ops.KernelProfile: the rows of its classifier kernels"""
    from neuralsampleid_amd import ops
    ops.PROFILE = ops.KernelProfile()
    try:
        ops.KernelProfile.plug(20.0)
        step()
        rows = ops.PROFILE.by_shape()
    finally:
        ops.PROFILE = None
    return [r for r in rows if r["kernel"].startswith("clf_")]


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [round(m, 3) for m in ms]


class EagerClf(nn.Module):
    """downstream.py:59-78 in training mode with an explicit keep mask in place of fc[2]'s own draw"""

    def __init__(self, clf):
        super().__init__()
        self.attn, self.fc, self.pos = clf.attn, clf.fc, clf.positional_embedding

    def forward(self, x_i, x_j, keep):
        x_i, x_j = x_i.permute(0, 2, 1), x_j.permute(0, 2, 1)
        pos = self.pos[:, :x_i.shape[1], :]
        a, _ = self.attn(x_i + pos, x_j + pos, x_j + pos)
        h = self.fc[1](self.fc[0](a.mean(dim=1))) * keep
        return self.fc[4](self.fc[3](h))


def eager_step(model, opt, ni, nj, zi, zj, keep):
    B = ni.shape[0]
    opt.zero_grad()
    x_all = torch.cat((ni, nj), dim=0)
    z_all = torch.cat((zi, zj), dim=0)
    sim = torch.matmul(zi, z_all.T)
    hn = torch.stack([torch.argsort(sim[i], descending=True)[1:K + 1] for i in range(B)])
    negs = x_all[hn.view(-1)]
    pos = model(ni, nj, keep[:B])
    neg = model(ni.repeat(K, 1, 1), negs, keep[B:])
    crit = nn.BCELoss()
    loss = crit(pos, torch.ones(B, 1, device=ni.device)) + crit(neg, torch.zeros(K * B, 1, device=ni.device))
    loss.backward()
    opt.step()
    return loss


def features(B, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    ni = torch.randn(B, C, N, generator=g)
    nj = ni + 0.5 * torch.randn(B, C, N, generator=g)
    zi = torch.nn.functional.normalize(torch.randn(B, 128, generator=g), dim=1)
    zj = torch.nn.functional.normalize(zi + 0.6 * torch.randn(B, 128, generator=g), dim=1)
    return [t.cuda().contiguous() for t in (ni, nj, zi, zj)]


def encoder_ms(B, reps):
    from synth import GRAFP_CFG
    from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
    from neuralsampleid_amd.simclr.simclr import SimCLR
    torch.manual_seed(0)
    model = SimCLR(GRAFP_CFG, GraphEncoder(GRAFP_CFG, in_channels=GRAFP_CFG["n_filters"], k=5, size="t")).cuda().eval()
    x_i = torch.randn(B, GRAFP_CFG["n_mels"], GRAFP_CFG["n_frames"], device="cuda").abs()
    x_j = torch.randn(B, GRAFP_CFG["n_mels"], GRAFP_CFG["n_frames"], device="cuda").abs()
    return timed(lambda: downstream.encode_pairs(model, x_i, x_j), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,256,1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only-ours", action="store_true")
    ap.add_argument("--in-dim", type=int, default=512, choices=(512, 640, 768, 1024), help="the classifier's width C")
    ap.add_argument("--nodes", type=int, default=32, help="nodes per segment, 1 .. 128 (above 32: the multi-tile kernels)")
    ap.add_argument("--kernels", action="store_true", help="one more HIP step per size under ops.KernelProfile: its clf_ kernels")
    args = ap.parse_args()
    C = args.in_dim
    global N
    if not 1 <= args.nodes <= 128:
        ap.error("--nodes must lie in [1, 128]")
    N = args.nodes
    for B in [int(s) for s in args.sizes.split(",")]:
        torch.manual_seed(0)
        clf = CrossAttentionClassifier(in_dim=C, num_nodes=N).cuda()
        ni, nj, zi, zj = features(B, C)
        keep = downstream.draw_keep((1 + K) * B, 0.3, "cuda")
        opt = torch.optim.Adam(clf.parameters(), lr=1e-4)
        hip = lambda: downstream.train_step(clf, opt, None, ni, nj, zi, zj, num_negatives=K, keep=keep)
        if args.only_ours:
            (ours, ours_all), = timed_interleaved([hip], args.reps)
        else:
            torch.manual_seed(0)
            clf_e = CrossAttentionClassifier(in_dim=C, num_nodes=N).cuda().train()
            model = EagerClf(clf_e)
            opt_e = torch.optim.Adam(clf_e.parameters(), lr=1e-4)
            (ours, ours_all), (eager, eager_all) = timed_interleaved([hip, lambda: eager_step(model, opt_e, ni, nj, zi, zj, keep)],
                                                                     args.reps)
        rec = {"in_dim": C, "nodes": N, "B": B, "pairs": (1 + K) * B, "step_gflop": round(step_flops(B, C) / 1e9, 2),
               "hip_ms": round(ours, 3), "hip_all": ours_all, "hip_tflops": round(step_flops(B, C) / ours / 1e9, 2)}
        if not args.only_ours:
            rec.update({"eager_ms": round(eager, 3), "eager_all": eager_all, "speedup": round(eager / ours, 2)})
        print(json.dumps(rec), flush=True)
        if args.kernels:
            for row in kernel_rows(hip):
                print(json.dumps(row), flush=True)
    if not args.only_ours:
        enc, enc_all = encoder_ms(32, args.reps)
        print(json.dumps({"encoder_forward_B32_ms": round(enc, 3), "all": enc_all}), flush=True)


if __name__ == "__main__":
    main()
