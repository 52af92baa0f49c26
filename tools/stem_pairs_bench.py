"""The stem-pair path (modules/data.py: GPUResample, StemBank, GPUStemPairSampler; csrc/stems.hip) at the training workloads' sizes,
on one GPU in one call:

    python tools/stem_pairs_bench.py [--reps 7] [--no-step]

  sampler     batch(256) (gate + packed build, 320 candidates) and forward() on 256 clips at the encoder's config (16 kHz, 4.08 s +
              0.25 s) and the baseline's (22 050 Hz, 5 s + 2.5 s), per launch from HIP events and as a synchronised wall clock
  resampler   44100 -> 16000 and 44100 -> 22050 of a 4-minute stereo track
  torch       the same arithmetic composed from stock torch ops on the same device: conv1d with the full filter table for the
              resampler; indexing, reductions in fp64, sort and gather for the sampler
  step        the training step each sampler feeds (the encoder's contrastive step, the baseline's bf16 step), same process
The repetitions of everything timed by wall clock are interleaved. Prints one JSON line and a table; where torch wins, the table
says so."""
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
from neuralsampleid_amd.modules.data import GPUResample, GPUStemPairSampler, StemBank  # noqa: E402

ENCODER_CFG = {"arch": "grafp", "fs": 16000, "dur": 4.08, "offset": 0.25, "silence": 1e-5}            # grafp.yaml
BASELINE_CFG = {"arch": "resnet-ibn", "fs": 22050, "dur": 5.0, "offset": 2.5, "silence": 1e-5}       # resnet_ibn.yaml


def synth_bank(cfg, tracks=8, seconds=60.0, seed=3, quiet_every=4):
    """a bank of synthetic tracks at cfg['fs']: tones under slow envelopes plus noise per stem; every `quiet_every`-th track has a
    silent stretch and a near-silent stem, so that some candidates are rejected"""
    bank = StemBank(cfg, "cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    T = int(seconds * cfg["fs"])
    t = torch.arange(T, device="cuda") / cfg["fs"]
    for k in range(tracks):
        f0 = 80.0 * 2.0 ** (4.0 * torch.rand(3, 1, device="cuda", generator=g))
        env = 0.55 + 0.45 * torch.sin(2 * np.pi * (0.1 + torch.rand(3, 1, device="cuda", generator=g)) * t)
        rows = env * (0.3 * torch.sin(2 * np.pi * f0 * t) + 0.1 * torch.sin(2 * np.pi * 2.7 * f0 * t))
        rows = rows + 0.03 * torch.randn(3, T, device="cuda", generator=g)
        if quiet_every and k % quiet_every == quiet_every - 1:
            rows[:, T // 3:T // 2] = 0.0
            rows[1] *= 1e-4
        bank.add_resampled(rows.float().contiguous())
    return bank


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


def torch_resample(x, orig, new):
    """audio.mean(0) + conv1d with the full table, as torchaudio composes it"""
    k = torch.from_numpy(ops.resample_table(orig, new)).to(x.device)
    o, n, width, _ = ops._resample_ratio(orig, new)
    T = x.shape[-1]

    def run():
        m = x.mean(dim=0) if x.dim() == 2 else x
        y = torch.nn.functional.conv1d(torch.nn.functional.pad(m[None, None], (width, width + o)), k[:, None], stride=o)
        return y[0].t().reshape(-1)[:ops.resample_out_len(T, orig, new)]
    return run


def torch_sampler(sampler, params):
    """forward() from stock torch ops: gather the windows, gate with fp64 reductions, order by key, crop, silence test"""
    bank, L, O, W = sampler.bank, sampler.L, sampler.O, sampler.W
    ar_w, ar_l = torch.arange(W, device="cuda"), torch.arange(L, device="cuda")

    def run():
        N = params.track.numel()
        base, ln = bank.base[params.track.long()], bank.length[params.track.long()].long()
        idx = (base + params.start.long())[:, None, None] + torch.arange(3, device="cuda")[None, :, None] * ln[:, None, None] + ar_w
        seg = bank.buf[idx]                                                  # (N, 3, W)
        tot = (seg[:, 0] + seg[:, 1]) + seg[:, 2]
        sig = tot[:, None] - seg
        d = sig - seg
        p_sig, p_n = sig.double().square().sum(-1), d.double().square().sum(-1)
        snr = (10.0 * torch.log10((p_sig / W) / (p_n / W + 1e-8))).float()
        valid = p_sig >= 0.1 * (p_n + 1e-8 * W)
        nv = valid.sum(1)
        key = torch.where(valid, params.key, torch.full_like(params.key, float("inf")))
        order = torch.sort(key, dim=1, stable=True).indices                  # valid stems first, by key, ties to the lower index
        last = torch.gather(order, 1, (nv - 1).clamp(min=0)[:, None])[:, 0]
        rows = torch.arange(N, device="cuda")
        is_i = torch.zeros_like(valid)
        is_i[rows, last] = True
        ci = params.off_i.long()[:, None] + ar_l
        cj = params.off_j.long()[:, None] + ar_l
        x_i = torch.gather(seg[rows, last], 1, ci)
        x_j = torch.gather((seg * (valid & ~is_i)[:, :, None]).sum(1), 1, cj)
        status = torch.where(nv < 2, 1, torch.where((x_i.abs().amax(1) < sampler.silence) | (x_j.abs().amax(1) < sampler.silence), 2, 0))
        keep = (status == 0)[:, None]
        return x_i * keep, x_j * keep, status.int(), snr
    return run


def run(args):
    rec = {"reps": args.reps, "sampler": {}, "resampler": {}}
    runs, kern = {}, {}
    B, N = 256, 320
    for name, cfg in (("encoder", ENCODER_CFG), ("baseline", BASELINE_CFG)):
        bank = synth_bank(cfg)
        sampler = GPUStemPairSampler(cfg, bank)
        gen = torch.Generator().manual_seed(7)
        p_batch, p_fwd = sampler.draw(N, gen), sampler.draw(B, gen)
        x_i, x_j, n_ok = sampler.batch(B, params=p_batch)
        st = sampler(p_fwd)[2]
        ts = torch_sampler(sampler, p_fwd)
        ref = ts()
        ours = sampler(p_fwd)
        same = bool(torch.equal(ours[2], ref[2]) and torch.equal(ours[0], ref[0]) and torch.equal(ours[1], ref[1]))
        rec["sampler"][name] = {"L": sampler.L, "O": sampler.O, "W": sampler.W, "bank_MiB": round(bank.nbytes() / 2 ** 20, 1),
                                "tracks": len(bank), "batch_n_ok": int(n_ok), "batch_candidates": N,
                                "forward_accepted": int((st == 0).sum()), "torch_composition_equal": same}
        runs[f"{name}: batch(256)"] = lambda s=sampler, p=p_batch: s.batch(B, params=p)
        runs[f"{name}: forward 256"] = lambda s=sampler, p=p_fwd: s(p)
        runs[f"{name}: torch forward 256"] = ts
        b = bank

        def gate_only(s=sampler, p=p_batch, b=b):
            st_, pl_, sn_ = (torch.empty(N, device="cuda", dtype=torch.int32), torch.empty(N, device="cuda", dtype=torch.int32),
                             torch.empty((N, 3), device="cuda"))
            return lambda: ops.call("nsid_stem_pairs_gate", ops._p(b.buf), b.buf.numel(), ops._p(b.base), ops._p(b.length), len(b),
                                    ops._p(p.track), ops._p(p.start), ops._p(p.key), ops._p(p.off_i), ops._p(p.off_j), N, s.L, s.O,
                                    s.silence, ops._p(st_), ops._p(sn_), ops._p(pl_), ops._stream())
        kern[f"{name}: gate, 320 candidates"] = gate_only()
    for orig, new in ((44100, 16000), (44100, 22050)):
        g = torch.Generator(device="cuda").manual_seed(orig + new)
        audio = (0.3 * torch.randn(2, 240 * orig, device="cuda", generator=g)).contiguous()
        res = GPUResample(orig, new)
        tr = torch_resample(audio, orig, new)
        y, y_t = res(audio), tr()
        rec["resampler"][f"{orig}->{new}"] = {"T": audio.shape[1], "T_out": y.numel(),
                                              "max_abs_diff_to_torch": float((y - y_t).abs().max())}
        runs[f"resample {orig}->{new}, 4 min stereo"] = lambda r=res, a=audio: r(a)
        runs[f"torch resample {orig}->{new}, 4 min stereo"] = tr
    if not args.no_step:
        from baseline_train_synthetic import build_model, hip_step, synth_pairs
        from neuralsampleid_amd.optim import FusedClipAdam
        F_.set_activation_dtype(torch.bfloat16)
        model = build_model()
        opt = FusedClipAdam(model.parameters(), lr=1e-4, max_norm=1.0, direct_grads=False, ds_prep=False)
        s_i, s_j = synth_pairs(256)
        runs["step: baseline, bf16, 256 pairs"] = lambda: hip_step(model, opt, s_i, s_j)
    for fn in list(runs.values()) + list(kern.values()):
        fn()
        fn()
    ms = {k: [] for k in runs}
    kms = {k: [] for k in kern}
    for _ in range(args.reps):
        for k, fn in runs.items():
            ms[k].append(round(wall_ms(fn), 4))
        for k, fn in kern.items():
            kms[k].append(round(event_ms(fn), 4))
    F_.set_activation_dtype(torch.float32)
    rec["ms_all"], rec["kernel_ms_all"] = ms, kms
    rec["ms"] = {k: float(np.median(v)) for k, v in ms.items()}
    rec["kernel_ms"] = {k: float(np.median(v)) for k, v in kms.items()}
    print(json.dumps(rec), flush=True)
    for k, v in rec["ms"].items():
        print(f"  {k:48s} {v:10.3f} ms   (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})")
    for k, v in rec["kernel_ms"].items():
        print(f"  {k:48s} {v:10.3f} ms   (HIP events)")
    for k, v in rec["ms"].items():
        other = "torch " + k if k.startswith("resample") else k.replace(": forward", ": torch forward")
        t = rec["ms"].get(other) if other != k else None
        if t is not None:
            print(f"  {k}: ours {v:.3f} ms, torch-eager {t:.3f} ms -> " + ("ours faster" if v < t else "TORCH-EAGER WINS"))
    for name, r in rec["sampler"].items():
        print(f"  {name}: L {r['L']}, O {r['O']}; bank {r['bank_MiB']} MiB in {r['tracks']} tracks; batch(256) accepted {r['batch_n_ok']} of "
              f"{r['batch_candidates']} candidates; torch composition equal: {r['torch_composition_equal']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-step", action="store_true")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
