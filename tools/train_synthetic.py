#!/usr/bin/env python3
"""The reference's training loop (train.py:53-81, :117-128) on the MI355X modules, with synthetic log-mel clips instead of
its audio pipeline (audio decoding / augmentation are outside this path). Shows the drop-in: only the import lines differ.

    python tools/train_synthetic.py --steps 50                       # reference-style loop: torch.optim.Adam + clip_grad_norm_
    python tools/train_synthetic.py --steps 50 --fused --bf16        # FusedClipAdam, bf16 activation storage, two-stream views
    python tools/train_synthetic.py --steps 50 --fused --graph --from-wave   # train.py:58 too: waveforms -> log-mel on the GPU
    python tools/train_synthetic.py --steps 50 --fused --from-wave --augment # and the waveform augmentations in front of it
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralsampleid_amd import functional as F_, ops  # noqa: E402
from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder  # noqa: E402  (reference: encoder.graph_encoder)
from neuralsampleid_amd.optim import FusedClipAdam  # noqa: E402
from neuralsampleid_amd.simclr.ntxent import ntxent_loss  # noqa: E402     (reference: simclr.ntxent)
from neuralsampleid_amd.simclr.simclr import SimCLR  # noqa: E402          (reference: simclr.simclr)

CFG = {"arch": "grafp", "n_mels": 64, "n_frames": 128, "patch_bins": 4, "patch_frames": 8, "n_filters": 8,
       "bsz_train": 256, "tau": 0.05, "lr": 8.0e-5, "d": 128, "h": 1024, "u": 32}


def batches(n, batch, device):
    g = torch.Generator().manual_seed(0)
    for _ in range(n):
        x_i = torch.randn(batch, CFG["n_mels"], CFG["n_frames"], generator=g) * 20.0 - 40.0
        yield x_i.to(device), (x_i + 3.0 * torch.randn(x_i.shape, generator=g)).to(device)


FCFG = {"fs": 16000, "n_fft": 1024, "win_len": 1024, "hop_len": 512, "overlap": 0.875, "arch": "grafp"}
ACFG = {"gain": 10, "pitch_shift": 3, "min_rate": 0.7, "max_rate": 1.5}      # grafp.yaml:45-50, the ranges of --augment
N_SAMPLES = 65280                                     # 4.08 s at 16 kHz (grafp.yaml): 128 frames


def wave_batches(n, batch, device):
    """synthetic 16 kHz waveforms: noise plus two tones per clip; view j is view i under a gain and more noise"""
    g = torch.Generator().manual_seed(0)
    t = torch.arange(N_SAMPLES) / FCFG["fs"]
    for _ in range(n):
        f = 200.0 + 3000.0 * torch.rand(batch, 2, generator=g)
        x_i = 0.05 * torch.randn(batch, N_SAMPLES, generator=g)
        x_i += 0.3 * torch.sin(2 * torch.pi * f[:, :1] * t) + 0.1 * torch.sin(2 * torch.pi * f[:, 1:] * t)
        x_j = 0.7 * x_i + 0.05 * torch.randn(batch, N_SAMPLES, generator=g)
        yield x_i.to(device), x_j.to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=CFG["bsz_train"])
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--fused", action="store_true", help="FusedClipAdam instead of clip_grad_norm_ + torch.optim.Adam")
    ap.add_argument("--graph", action="store_true", help="capture the step in a hipGraph (graphs.GraphedTrainStep; needs --fused)")
    ap.add_argument("--bf16", action="store_true", help="bf16 activation storage + bf16 MFMA operands (BASELINE config 2)")
    ap.add_argument("--from-wave", action="store_true",
                    help="start every step from waveforms: GPUTransformSampleID(train=True) as train.py:58 `augment`")
    ap.add_argument("--augment", action="store_true",
                    help="with --from-wave: Gain + TimeStretch / PitchShift of the pair on the GPU (GPUWaveAugment), eagerly in "
                         "front of the step, the reference's GPUTransformSampleID(cpu=True) on its DataLoader workers")
    ap.add_argument("--from-bank", action="store_true",
                    help="with --from-wave --augment: cut every batch from a synthetic StemBank with GPUStemPairSampler.batch "
                         "(the dataset's __getitem__ on the device) instead of ready-made waveform pairs")
    args = ap.parse_args()
    if args.augment and not args.from_wave:
        ap.error("--augment works on waveforms: add --from-wave")
    if args.from_bank and not args.augment:
        ap.error("--from-bank feeds the augmenter: add --from-wave --augment")
    device = torch.device("cuda")
    source, augment, wave_aug = batches, None, None
    if args.from_wave:
        from neuralsampleid_amd.modules.transformations import GPUTransformSampleID   # (reference: modules.transformations)
        augment = GPUTransformSampleID(cfg={**CFG, **FCFG}, train=True).to(device)    # train.py:100
        source = wave_batches
    if args.augment:
        from neuralsampleid_amd.modules.transformations import GPUWaveAugment
        wave_aug = GPUWaveAugment(cfg={**CFG, **FCFG, **ACFG}).to(device)
    if args.from_bank:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from stem_pairs_bench import ENCODER_CFG, synth_bank
        from neuralsampleid_amd.modules.data import GPUStemPairSampler
        sampler = GPUStemPairSampler(ENCODER_CFG, synth_bank(ENCODER_CFG, tracks=4, seconds=30.0))        # built once
        assert sampler.L == N_SAMPLES
        draws = torch.Generator().manual_seed(5)

        def source(n, batch, device):                 # every batch is cut from the bank; n_ok stays on the device
            for _ in range(n):
                yield sampler.batch(batch, generator=draws)[:2]
    if args.bf16:
        ops.set_gemm_precision("bf16")
        F_.set_activation_dtype("bf16")
    torch.manual_seed(42)
    model = SimCLR(CFG, encoder=GraphEncoder(cfg=CFG, in_channels=CFG["n_filters"], k=args.k, size="t"),
                   overlap_views=args.fused).to(device)                                   # train.py:113-116
    model.train()
    if args.fused:
        optimizer = FusedClipAdam(model.parameters(), lr=CFG["lr"], max_norm=1.0)
    else:
        optimizer = torch.optim.Adam(model.parameters(), lr=CFG["lr"])                    # train.py:126
    if args.graph:
        from neuralsampleid_amd.graphs import GraphedTrainStep
        data = list(source(args.steps, args.batch, device))
        step = GraphedTrainStep(model, optimizer, CFG, *data[0], front=augment.front(device) if augment else None)
        torch.cuda.synchronize()
        t0 = time.time()
        for idx, (x_i, x_j) in enumerate(data):
            if wave_aug is not None:
                x_i, x_j = wave_aug(x_i, x_j)                                             # eager, in front of the captured step
            loss = step(x_i, x_j)
            if idx % 10 == 0:
                print(f"Step [{idx}/{args.steps}]\t Loss: {loss.item():.4f}")
        torch.cuda.synchronize()
        print(f"{args.steps} graph replays in {time.time() - t0:.2f} s")
        return
    t0 = time.time()
    for idx, (x_i, x_j) in enumerate(source(args.steps, args.batch, device)):            # train.py:53
        optimizer.zero_grad()                                                             # :58
        if wave_aug is not None:
            x_i, x_j = wave_aug(x_i, x_j)                                                 # the dataset's transform, on the device
        if augment is not None:
            with torch.no_grad():
                x_i, x_j = augment(x_i, x_j)                                              # :58-59
        h_i, h_j, z_i, z_j = model(x_i, x_j)                                              # :61
        loss = ntxent_loss(z_i, z_j, CFG)                                                 # :63
        if torch.isnan(loss):                                                             # :65-68
            print(f"NaN loss at step {idx}, skipping batch")
            continue
        loss.backward()                                                                   # :70
        if not args.fused:
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)              # :73
        optimizer.step()                                                                  # :75
        if idx % 10 == 0:
            print(f"Step [{idx}/{args.steps}]\t Loss: {loss.item():.4f}")                  # :77-78
    torch.cuda.synchronize()
    print(f"{args.steps} steps in {time.time() - t0:.2f} s (eager launches; bench.py replays the step as one hipGraph)")


if __name__ == "__main__":
    main()
