#!/usr/bin/env python3
"""Stand-alone timing of the log-mel front end in both STFT modes (frontend.LogMelFrontEnd(stft="gemm" | "fft")), and of the
captured training step from waveforms against the captured step from mels. Prints one JSON line.

    python tools/frontend_bench.py [--reps 15] [--no-step]

Method: HIP events around each call on the launch stream; every shape is warmed up; operands are COLD (each repetition takes the
next of a ring of input buffers whose total exceeds the 256 MB Infinity Cache); the modes are interleaved repetition by
repetition and the median is reported. Shapes:
  (a) training    512 x 65 280 samples (two views of 256 clips of 4.08 s): the fused kernel as one launch of 512 clips and as two
                  launches of 256; stft="gemm" has no batched form, so its column is the per-clip loop of 512 logmel() calls
                  (3 launches and 2 temporaries each), which is what a caller could do before
  (b) extraction  one waveform of 1 024 segments (16 496 frames), front(wave) including the segment gather
  (c) one clip    one 4.08 s waveform, logmel(wave)
Floors of the fused kernel are stated from shapes: waveform bytes read once + log-mel bytes stored, over 8 TB/s of HBM."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralsampleid_amd import _lib, functional as F_, ops  # noqa: E402
from neuralsampleid_amd.frontend import LogMelFrontEnd  # noqa: E402

FCFG = {"fs": 16000, "n_fft": 1024, "win_len": 1024, "hop_len": 512, "n_mels": 64, "n_frames": 128, "overlap": 0.875}
CFG = {"arch": "grafp", "n_mels": 64, "n_frames": 128, "patch_bins": 4, "patch_frames": 8, "n_filters": 8,
       "bsz_train": 256, "tau": 0.05, "lr": 8.0e-5, "d": 128, "h": 1024, "u": 32}
L_CLIP = 65280
HBM_GBPS = 8000.0
GEMM_FLOOR_MS = 0.89          # 65 536 frames x 2 x 1024 x 1028 flop at 155 TFLOP/s of f32-input MFMA


def waves(n, L, seed, device):
    """noise plus two tones per clip, generated on the device"""
    g = torch.Generator(device=device).manual_seed(seed)
    t = torch.arange(L, device=device, dtype=torch.float32) / FCFG["fs"]
    f = 200.0 + 3000.0 * torch.rand(n, 2, generator=g, device=device)
    x = 0.05 * torch.randn(n, L, generator=g, device=device)
    x += 0.3 * torch.sin(2 * torch.pi * f[:, :1] * t) + 0.1 * torch.sin(2 * torch.pi * f[:, 1:] * t)
    return x


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved(cases, reps, warmup=2):
    """cases: {name: fn(rep)}; one call of every case per repetition, in turn; medians in ms"""
    for r in range(warmup):
        for fn in cases.values():
            fn(r)
    torch.cuda.synchronize()
    ts = {k: [] for k in cases}
    for r in range(reps):
        for k, fn in cases.items():
            ts[k].append(timed(lambda: fn(warmup + r)))
    return {k: round(statistics.median(v), 4) for k, v in ts.items()}, {k: round(min(v), 4) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--loop-reps", type=int, default=3, help="repetitions of the 512-call per-clip loop of shape (a)")
    ap.add_argument("--no-step", action="store_true", help="skip the captured training steps")
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/frontend_bench.py measures on an MI355X; there is no CPU path")
    dev = torch.device("cuda")
    fft, gemm = LogMelFrontEnd(FCFG, dev, stft="fft"), LogMelFrontEnd(FCFG, dev, stft="gemm")
    res = {"tool": "frontend_bench", "reps": args.reps, "unit": "ms (median of interleaved repetitions, cold operands)"}

    # (a) training shape: a ring of 3 x 512 clips = 401 MB
    ring = [waves(512, L_CLIP, 10 + i, dev) for i in range(3)]
    _lib.launch_counters(reset=True)
    med, mn = interleaved({
        "fft_1x512": lambda r: fft.batch(ring[r % 3]),
        "fft_2x256": lambda r: (fft.batch(ring[r % 3][:256]), fft.batch(ring[r % 3][256:])),
    }, args.reps)
    launches = _lib.launch_counters()["logmel_fft"]
    loop, _ = interleaved({"gemm_loop_512": lambda r: [gemm.logmel(w) for w in ring[r % 3]]}, args.loop_reps, warmup=1)
    bytes_a = 512 * L_CLIP * 4 + 512 * 64 * 128 * 4
    floor_a = bytes_a / HBM_GBPS / 1e6
    res["a_training_512x65280"] = {
        **med, "fft_1x512_min": mn["fft_1x512"], **loop, "gemm_column": "per-clip loop of 512 logmel() calls (no batched form)",
        "speedup_fft_over_gemm_loop": round(loop["gemm_loop_512"] / med["fft_1x512"], 1),
        "fft_hbm_floor_ms": round(floor_a, 4), "fft_fraction_of_hbm": round(floor_a / med["fft_1x512"], 3),
        "gemm_arithmetic_floor_ms": GEMM_FLOOR_MS, "below_gemm_floor": med["fft_1x512"] < GEMM_FLOOR_MS,
        "fft_launches_counted": launches}
    del ring

    # (b) extraction: one waveform of 1 024 segments; ring of 9 x 33.8 MB = 304 MB
    frames = (1024 - 1) * fft.step + FCFG["n_frames"]
    Lb = (frames - 1) * FCFG["hop_len"]
    ring = [waves(1, Lb, 30 + i, dev)[0] for i in range(9)]
    med, _ = interleaved({"fft": lambda r: fft(ring[r % 9]), "gemm": lambda r: gemm(ring[r % 9])}, args.reps)
    bytes_b = Lb * 4 + 64 * frames * 4
    res["b_extraction_1024_segments"] = {**med, "speedup": round(med["gemm"] / med["fft"], 2), "samples": Lb, "frames": frames,
                                         "includes": "segment gather (nsid_unfold_segments)",
                                         "fft_logmel_hbm_floor_ms": round(bytes_b / HBM_GBPS / 1e6, 4)}
    del ring

    # (c) one 4.08 s clip: ring of 1 100 clips = 287 MB
    ring = waves(1100, L_CLIP, 50, dev)
    med, _ = interleaved({"fft": lambda r: fft.logmel(ring[(37 * r) % 1100]), "gemm": lambda r: gemm.logmel(ring[(37 * r) % 1100])},
                         max(args.reps, 31), warmup=3)
    res["c_one_clip_65280"] = {**med, "speedup": round(med["gemm"] / med["fft"], 2)}
    del ring

    if not args.no_step:
        from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
        from neuralsampleid_amd.graphs import GraphedTrainStep
        from neuralsampleid_amd.optim import FusedClipAdam
        from neuralsampleid_amd.simclr.simclr import SimCLR
        ops.set_gemm_precision("bf16")                       # bench.py's headline configuration: bf16 storage, two-stream views
        F_.set_activation_dtype("bf16")
        B = args.batch
        ring = [(waves(B, L_CLIP, 70 + i, dev), waves(B, L_CLIP, 80 + i, dev)) for i in range(3)]
        steps = {}
        for kind in ("mel", "wave"):
            torch.manual_seed(42)
            model = SimCLR(CFG, encoder=GraphEncoder(cfg=CFG, in_channels=CFG["n_filters"], k=3, size="t"), overlap_views=True).to(dev)
            model.train()
            opt = FusedClipAdam(model.parameters(), lr=CFG["lr"], max_norm=1.0)
            if kind == "mel":
                mels = [(fft.batch(a), fft.batch(b)) for a, b in ring]
                step = GraphedTrainStep(model, opt, CFG, *mels[0])
                steps[kind] = (lambda r, step=step, mels=mels: step(*mels[r % 3]))
            else:
                step = GraphedTrainStep(model, opt, CFG, *ring[0], front=fft)
                steps[kind] = (lambda r, step=step: step(*ring[r % 3]))
        med, _ = interleaved({"graphed_step_from_mels": steps["mel"], "graphed_step_from_waveforms": steps["wave"]},
                             max(args.reps, 20), warmup=5)
        res["graphed_step"] = {**med, "batch": B, "from_audio_costs_ms": round(med["graphed_step_from_waveforms"] -
                                                                                med["graphed_step_from_mels"], 4),
                               "note": "both include the copy of the batch into the static buffers (mels 16.8 MB, waveforms 133.7 MB)"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
