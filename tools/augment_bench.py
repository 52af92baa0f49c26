#!/usr/bin/env python3
"""Times the waveform augmentations (modules/transformations.GPUWaveAugment on csrc/augment.hip) on one GPU for the training batch,
B = 256 clips of 65 280 samples with parameters drawn from config/grafp.yaml's ranges (gain 10 dB, rates 0.7 .. 1.5, +-3 semitones),
next to the same algorithm composed from torch-eager ops on the same GPU and to the captured contrastive step the batch feeds.
Prints one JSON line.

    python tools/augment_bench.py [--reps 15] [--no-step] [--no-eager]

Method: HIP events on the launch stream; warm-up first; the cases alternate repetition by repetition and the median is reported.
The inputs rotate through a ring of three batches. The per-stage split times the four stages of every chunk with events of their
own in a separate pass (its sum exceeds the whole call by the event overhead). The torch-eager column is the definition of
DESIGN.md restated with torch.fft, gathers and elementwise ops (fp64 index arithmetic, fp32 values); its result is compared with
the kernels' in the same call ("eager_vs_kernels_rel": max |a - b| / max |b| over the batch)."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralsampleid_amd import _lib, functional as F_, ops  # noqa: E402
from neuralsampleid_amd.modules.transformations import (AUG_PRECISION, AUG_ZEROS, GPUWaveAugment, WaveAugmentParams,  # noqa: E402
                                                        aug_filter_table)

FCFG = {"fs": 16000, "n_fft": 1024, "win_len": 1024, "hop_len": 512, "n_mels": 64, "n_frames": 128, "overlap": 0.875}
ACFG = {"arch": "grafp", "gain": 10, "pitch_shift": 3, "min_rate": 0.7, "max_rate": 1.5}          # config/grafp.yaml:45-50
CFG = {"arch": "grafp", "n_mels": 64, "n_frames": 128, "patch_bins": 4, "patch_frames": 8, "n_filters": 8,
       "bsz_train": 256, "tau": 0.05, "lr": 8.0e-5, "d": 128, "h": 1024, "u": 32}
L_CLIP = 65280
N, HOP, BINS = ops.AUG_N_FFT, ops.AUG_HOP, ops.AUG_BINS


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
    for r in range(warmup):
        for fn in cases.values():
            fn(r)
    torch.cuda.synchronize()
    ts = {k: [] for k in cases}
    for r in range(reps):
        for k, fn in cases.items():
            ts[k].append(timed(lambda: fn(warmup + r)))
    return {k: round(statistics.median(v), 4) for k, v in ts.items()}


class EagerAugment:
    """the same four stages from torch ops, `chunk` clips at a time"""

    def __init__(self, aug, device, chunk=16):
        self.aug, self.chunk = aug, chunk
        self.win = torch.hann_window(N, periodic=True, dtype=torch.float64).to(torch.float32).to(device)
        self.tab = torch.from_numpy(aug_filter_table().astype(np.float32)).to(device)

    def __call__(self, x_i, x_j, p):
        B, L = x_i.shape
        out = torch.empty_like(x_i)
        for b0 in range(0, B, self.chunk):
            sl = slice(b0, min(B, b0 + self.chunk))
            out[sl] = self.some(x_i[sl], x_j[sl], p.gain[sl], p.mode[sl], p.rate[sl])
        return out

    def some(self, x_i, x_j, gain, mode, rate):
        B, L = x_i.shape
        dev = x_i.device
        T_in, T_max, S_max = self.aug.extents(L)
        r = rate.clamp(self.aug.rate_lo, self.aug.rate_hi).double()
        y = F.pad(gain[:, None] * x_j + x_i, (N // 2, N // 2))
        D = torch.fft.rfft(y.unfold(1, N, HOP)[:, :T_in] * self.win, dim=2)                  # (B, T_in, 1025)
        D = torch.cat([D, torch.zeros(B, 2, BINS, dtype=D.dtype, device=dev)], 1)
        mag, ang = D.abs(), D.angle()
        T_out = torch.ceil(T_in / r).long()
        phi = ((torch.arange(BINS, device=dev) % 4) * (math.pi / 2)).float()
        two_pi = 2 * math.pi
        acc = ang[:, 0]
        S = torch.zeros(B, T_max, BINS, dtype=D.dtype, device=dev)
        rows = torch.arange(B, device=dev)
        for t in range(T_max):
            st = t * r
            c = torch.floor(st).long().clamp_max(T_in)
            a = (st - torch.floor(st)).float()[:, None]
            m = (1 - a) * mag[rows, c] + a * mag[rows, c + 1]
            S[:, t] = torch.polar(m, acc) * (t < T_out)[:, None]
            d = ang[rows, c + 1] - ang[rows, c] - phi
            d = d - two_pi * torch.round(d / two_pi)
            acc = acc + phi + d
            acc = acc - two_pi * torch.round(acc / two_pi)
        fr = torch.fft.irfft(S, n=N, dim=2) * self.win                                        # (B, T_max, N)
        full = N + HOP * (T_max - 1)
        ola = F.fold(fr.transpose(1, 2), (1, full), (1, N), stride=(1, HOP)).reshape(B, full)
        w2 = (self.win * self.win)[None, :, None] * (torch.arange(T_max, device=dev)[None, None, :] < T_out[:, None, None])
        wss = F.fold(w2.float(), (1, full), (1, N), stride=(1, HOP)).reshape(B, full)
        s = torch.where(wss > torch.finfo(torch.float32).tiny, ola / wss, ola)[:, N // 2:]
        s = F.pad(s, (0, max(0, S_max - s.shape[1])))[:, :S_max]
        n_s = torch.round(L / r).long()                                                       # ties to even
        s = s * (torch.arange(S_max, device=dev)[None] < n_s[:, None])
        out = s[:, :L] if S_max >= L else F.pad(s, (0, L - S_max))
        pitch = (mode == 1).nonzero().flatten()
        if len(pitch):
            out = out.clone()
            out[pitch] = self.resample(s[pitch], r[pitch], n_s[pitch], L)
        return out

    def resample(self, s, r, n_s, L):
        dev = s.device
        c = r.clamp_max(1.0)
        K = 2 * int(math.ceil(AUG_ZEROS / float(c.min()))) + 3
        out = torch.zeros(s.shape[0], L, device=dev)
        n_out = torch.ceil(n_s.double() * r).long()
        off = torch.arange(K, device=dev) - K // 2
        for m0 in range(0, L, 8192):
            m = torch.arange(m0, min(L, m0 + 8192), device=dev)
            pos = m.double()[None] / r[:, None]                                               # (P, M)
            j = torch.floor(pos).long()[:, :, None] + off
            x = (pos[:, :, None] - j).abs() * (c * AUG_PRECISION)[:, None, None]
            ok = (j >= 0) & (j < n_s[:, None, None]) & (x < AUG_ZEROS * AUG_PRECISION)
            i0 = torch.floor(x).long().clamp_max(AUG_ZEROS * AUG_PRECISION - 1)
            e = (x - i0).float()
            wgt = self.tab[i0] + e * (self.tab[i0 + 1] - self.tab[i0])
            v = torch.gather(s, 1, j.clamp(0, s.shape[1] - 1).reshape(s.shape[0], -1)).reshape(j.shape)
            acc = (torch.where(ok, wgt * v, torch.zeros((), device=dev))).sum(2) * c.float()[:, None]
            out[:, m0:m0 + len(m)] = acc * (m[None] < n_out[:, None])
        return out


def stage_split(aug, x_i, x_j, p, reps):
    """ms per stage over the whole batch: events around every launch of every chunk"""
    B, L = x_i.shape
    ws = aug._workspace(x_i.device, B, L)
    out = torch.empty((B, L), device=x_i.device)
    lo, hi = aug.rate_lo, aug.rate_hi
    acc = {k: [] for k in ("stft", "vocoder", "istft", "finish")}
    for _ in range(reps):
        tot = dict.fromkeys(acc, 0.0)
        for b0 in range(0, B, ws["chunk"]):
            b1 = min(B, b0 + ws["chunk"])
            n, g, m, r = b1 - b0, p.gain[b0:b1], p.mode[b0:b1], p.rate[b0:b1]
            tot["stft"] += timed(lambda: ops.aug_stft(x_i[b0:b1], x_j[b0:b1], g, ws["window"], ws["twiddle"], ws["spec"]))
            tot["vocoder"] += timed(lambda: ops.aug_vocoder(ws["spec"], n, L, r, lo, hi, ws["voc"]))
            tot["istft"] += timed(lambda: ops.aug_istft(ws["voc"], n, L, r, lo, hi, ws["window"], ws["twiddle"], ws["wave"]))
            tot["finish"] += timed(lambda: ops.aug_finish(ws["wave"], n, L, m, r, lo, hi, ws["table"], out[b0:b1]))
        for k, v in tot.items():
            acc[k].append(v)
    return {k: round(statistics.median(v), 4) for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-step", action="store_true", help="skip the captured contrastive step")
    ap.add_argument("--no-eager", action="store_true", help="skip the torch-eager composition")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/augment_bench.py measures on an MI355X; there is no CPU path")
    dev = torch.device("cuda")
    B = args.batch
    aug = GPUWaveAugment({**FCFG, **ACFG})
    p = aug.draw(B, generator=torch.Generator().manual_seed(0), device=dev)
    ring = [(waves(B, L_CLIP, 10 + i, dev), waves(B, L_CLIP, 20 + i, dev)) for i in range(3)]
    res = {"tool": "augment_bench", "batch": B, "samples": L_CLIP, "reps": args.reps,
           "unit": "ms per batch (median of alternating repetitions)", "pitch_clips": int(p.mode.sum()),
           "workspace_mb": round(aug.workspace_bytes(B, L_CLIP) / 2 ** 20, 1)}
    cases = {"kernels": lambda r: aug(*ring[r % 3], p)}
    if not args.no_eager:
        eager = EagerAugment(aug, dev)
        cases["torch_eager"] = lambda r: eager(*ring[r % 3], p)
        a, b = aug(*ring[0], p)[0], eager(*ring[0], p)
        res["eager_vs_kernels_rel"] = float(((a - b).abs().amax(1) / a.abs().amax(1)).max())
    if not args.no_step:
        from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
        from neuralsampleid_amd.frontend import LogMelFrontEnd
        from neuralsampleid_amd.graphs import GraphedTrainStep
        from neuralsampleid_amd.optim import FusedClipAdam
        from neuralsampleid_amd.simclr.simclr import SimCLR
        ops.set_gemm_precision("bf16")                       # bench.py's headline configuration: bf16 storage, two-stream views
        F_.set_activation_dtype("bf16")
        torch.manual_seed(42)
        model = SimCLR(CFG, encoder=GraphEncoder(cfg=CFG, in_channels=CFG["n_filters"], k=3, size="t"), overlap_views=True).to(dev)
        model.train()
        opt = FusedClipAdam(model.parameters(), lr=CFG["lr"], max_norm=1.0)
        step = GraphedTrainStep(model, opt, CFG, *ring[0], front=LogMelFrontEnd(FCFG, dev, stft="fft"))
        cases["graphed_step_from_waveforms"] = lambda r: step(*ring[r % 3])
    _lib.launch_counters(reset=True)
    med = interleaved(cases, args.reps)
    res.update(med)
    res["kernels_clips_per_s"] = round(B / med["kernels"] * 1e3)
    if "torch_eager" in med:
        res["eager_over_kernels"] = round(med["torch_eager"] / med["kernels"], 1)
    if "graphed_step_from_waveforms" in med:
        res["kernels_over_step"] = round(med["kernels"] / med["graphed_step_from_waveforms"], 3)
    c = _lib.launch_counters()
    res["launches_per_call"] = {k: c[k] // (args.reps + 2) for k in ("aug_stft", "aug_vocoder", "aug_istft", "aug_finish")}
    res["stages"] = stage_split(aug, *ring[0], p, args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
