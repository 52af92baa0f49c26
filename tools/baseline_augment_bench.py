"""The baseline's waveform augmentations (modules/transformations.GPUBaselineWaveAugment) at the training workload's size, on one GPU:
B = 512 and 256 clips of L = 110 250 samples (5 s at 22 050 Hz) with drawn parameters.

    python tools/baseline_augment_bench.py [--reps 5] [--oracle-clips 4] [--no-step]

Reports, as one JSON line and a table,
  per kernel        nsid_aug_compress, nsid_aug_biquad, nsid_aug_frames on the whole batch and the four launches of the vocoder chain per
                    chunk of 64, from HIP events around each call (milliseconds; the launches are far longer than an event pair's error)
  module            forward() with given params, wall clock around a synchronised call; and draw() on the host
  vocoder_wasted    the share of the vocoder chain spent on the frame-edit clips, whose rows nsid_aug_frames then overwrites
  oracle            tests/baseline_augment_oracle.augment (fp64, numpy / Python) on --oracle-clips clips of the same draw on the host,
                    scaled to the batch
  step              the training step of tools/baseline_train_synthetic.py (bf16 storage, 256 pairs) in the same process, the
                    repetitions of step and module interleaved"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from neuralsampleid_amd import functional as F_  # noqa: E402
from neuralsampleid_amd import ops  # noqa: E402
from neuralsampleid_amd.modules.transformations import BaselineAugmentParams, GPUBaselineWaveAugment  # noqa: E402

CFG = {"arch": "resnet-ibn", "fs": 22050, "dur": 5.0, "hop_len": 512, "n_frames": 216, "overlap": 0.5, "gain": 10, "pitch_shift": 3,
       "min_rate": 0.7, "max_rate": 1.5, "DC_threshold": [-30, 0], "DC_ratio": [2, 4, 8, 20], "DC_attack": [0.001, 0.1],
       "DC_release": [0.05, 1.0]}
L = 110250


def synth_stems(B, L=L, seed=3):
    """x_i: the remaining stem (noise), x_j: the sample stems (two tones under a slow envelope + noise), (B, L) float32 on the GPU"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(L, device="cuda") / CFG["fs"]
    f0 = 110.0 * 2.0 ** (4.0 * torch.rand(B, 1, device="cuda", generator=g))
    env = 0.55 + 0.45 * torch.sin(2 * np.pi * (0.5 + torch.rand(B, 1, device="cuda", generator=g)) * t)
    x_j = env * (0.5 * torch.sin(2 * np.pi * f0 * t) + 0.2 * torch.sin(2 * np.pi * 2.7 * f0 * t))
    x_j = x_j + 0.05 * torch.randn(B, L, device="cuda", generator=g)
    x_i = 0.1 * torch.randn(B, L, device="cuda", generator=g)
    return x_i.contiguous(), x_j.contiguous()


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def kernel_runs(m, x_i, x_j, p):
    B = x_i.shape[0]
    ws = m._workspace(x_i.device, B, L)
    t1, out = ws["t1"], torch.empty_like(x_i)
    lo, hi, n = m.rate_lo, m.rate_hi, ws["chunk"]

    def chain():
        for b0 in range(0, B, n):
            b1 = b0 + n
            ops.aug_stft(x_i[b0:b1], t1[b0:b1], p.gain[b0:b1], ws["window"], ws["twiddle"], ws["spec"])
            ops.aug_vocoder(ws["spec"], n, L, p.rate[b0:b1], lo, hi, ws["voc"])
            ops.aug_istft(ws["voc"], n, L, p.rate[b0:b1], lo, hi, ws["window"], ws["twiddle"], ws["wave"])
            ops.aug_finish(ws["wave"], n, L, p.mode2[b0:b1], p.rate[b0:b1], lo, hi, ws["table"], out[b0:b1])
    return {"copy": lambda: t1.copy_(x_j),
            "aug_compress": lambda: ops.aug_compress(x_j, p.mode1, p.cmp, t1),
            "aug_biquad": lambda: ops.aug_biquad(x_j, p.mode1, p.sos, p.n_sec, t1),
            "vocoder_chain": chain,
            "aug_frames": lambda: ops.aug_frames(x_i, t1, p.gain, p.mode2, p.frame_size, p.frame_ops, out)}


def host_oracle_ms(m, x_i, x_j, p, clips):
    import baseline_augment_oracle as O
    xi, xj = x_i[:clips].cpu().numpy(), x_j[:clips].cpu().numpy()
    ph = [t[:clips].cpu().numpy() for t in p]
    t0 = time.perf_counter()
    for b in range(clips):
        O.augment(xi[b], xj[b], {k: v[b] for k, v in zip(p._fields, ph)})
    return 1e3 * (time.perf_counter() - t0) / clips


def run(args):
    rec = {"L": L, "reps": args.reps, "batches": {}}
    runs = {}
    for B in (512, 256):
        m = GPUBaselineWaveAugment(CFG, generator=torch.Generator().manual_seed(1))
        t0 = time.perf_counter()
        p = m.draw(B, generator=torch.Generator().manual_seed(2), device="cuda", L=L)
        draw_ms = 1e3 * (time.perf_counter() - t0)
        x_i, x_j = synth_stems(B)
        m(x_i, x_j, p)
        m(x_i, x_j, p)
        torch.cuda.synchronize()
        kr = kernel_runs(m, x_i, x_j, p)
        for fn in kr.values():
            fn()
        kern = {k: [round(event_ms(fn), 3) for _ in range(args.reps)] for k, fn in kr.items()}
        frame_share = float(((p.mode2 >= 2) & (p.mode2 <= 4)).float().mean())
        rec["batches"][B] = {"num_bands": m.num_bands, "draw_host_ms": round(draw_ms, 1), "kernel_ms": {k: float(np.median(v)) for k, v in kern.items()},
                             "kernel_ms_all": kern, "clips": {"eq": int((p.mode1 == 0).sum()), "compress": int((p.mode1 == 1).sum()),
                                                              "frames": int((p.mode2 >= 2).sum())},
                             "sections_max": int(p.n_sec.max()), "frame_share": round(frame_share, 3),
                             "vocoder_wasted_ms": round(frame_share * float(np.median(kern["vocoder_chain"])), 3),
                             "workspace_MiB": round(m.workspace_bytes(B, L) / 2 ** 20, 1)}
        runs[f"augment_{B}"] = (lambda m=m, x_i=x_i, x_j=x_j, p=p: m(x_i, x_j, p))
        if B == 512 and args.oracle_clips > 0:
            per_clip = host_oracle_ms(m, x_i, x_j, p, args.oracle_clips)
            rec["oracle_host_ms_per_clip"] = round(per_clip, 1)
            rec["oracle_host_ms_scaled_512"] = round(512 * per_clip, 0)
    if not args.no_step:
        from baseline_train_synthetic import build_model, hip_step, synth_pairs
        from neuralsampleid_amd.optim import FusedClipAdam
        F_.set_activation_dtype(torch.bfloat16)
        model = build_model()
        opt = FusedClipAdam(model.parameters(), lr=1e-4, max_norm=1.0, direct_grads=False, ds_prep=False)
        s_i, s_j = synth_pairs(256)
        runs["step_bf16_256"] = lambda: hip_step(model, opt, s_i, s_j)
    for fn in runs.values():
        fn()
        fn()
    ms = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            ms[k].append(round(wall_ms(fn), 3))
    F_.set_activation_dtype(torch.float32)
    rec["ms_all"] = ms
    rec["ms"] = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps(rec), flush=True)
    for B, r in rec["batches"].items():
        print(f"B = {B}: {r['clips']} clips, {r['num_bands']} bands (<= {r['sections_max']} sections), draw() {r['draw_host_ms']} ms on the host, "
              f"workspaces {r['workspace_MiB']} MiB")
        for k, v in r["kernel_ms"].items():
            print(f"  {k:16s} {v:9.3f} ms")
        print(f"  {'module forward':16s} {rec['ms'][f'augment_{B}']:9.3f} ms; of the vocoder chain {r['vocoder_wasted_ms']} ms "
              f"({100 * r['frame_share']:.0f} % of the clips) is overwritten by the frame edits")
    if "oracle_host_ms_per_clip" in rec:
        print(f"host fp64 oracle: {rec['oracle_host_ms_per_clip']} ms per clip, {rec['oracle_host_ms_scaled_512'] / 1e3:.1f} s for 512 clips on one core")
    if "step_bf16_256" in rec["ms"]:
        print(f"training step, 256 pairs, bf16 storage: {rec['ms']['step_bf16_256']:.2f} ms; augmentation of 256 clips: "
              f"{rec['ms']['augment_256']:.2f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-clips", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
