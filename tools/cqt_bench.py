"""Times the constant-Q front end of the ResNet-IBN baseline (frontend.CQTFrontEnd.batch on csrc/cqt.hip) on one GPU, next to the same
transform composed from entry points the library already had and next to torch-eager, all in one run on the same device.

    python tools/cqt_bench.py [--batch 256] [--samples 110250] [--reps 5] [--dense-clips 8] [--eager matmul|conv1d]

  (a) fused        CQTFrontEnd.batch: one launch for the whole batch.
  (b) dense        per clip: nsid_reflect_pad, then nsid_linear_fwd in exact fp32 with lda = hop (overlapping frames of the padded
                   clip) against the dense [re; im] matrix (168 x width), then the magnitude in torch. Timed for --dense-clips clips
                   and EXTRAPOLATED to the batch (x batch / dense-clips): the composition has no batched form, every clip is three
                   launches plus the torch ops.
  (c) torch-eager  reflect pad, unfold into frames and one matmul against the same dense matrix (--eager matmul, the default, in
                   chunks of 32 clips so that the frame matrix stays at 0.45 GB), or F.conv1d with the 168 filters of `width` taps
                   (--eager conv1d: MIOpen has to accept a 16 384-wide filter; not the default because its algorithm search is not
                   bounded in time).

(a) and (b) are captured in a hipGraph and replayed; every replay of (a) runs the batch on each of several input buffers in turn,
together larger than the 256 MB last-level cache, so that no call finds its waveforms cached ("cold operands"); the tables are the
same every call, as in use. Times are device events around --reps replays, after a warm-up replay; the median is reported.
The last figures put (a) next to the extraction it feeds: extract_fingerprints of the same number of (84, T) segments through
tools/resnet_ibn_bench.py's model, wall time ending in a synchronise, fp32 and bf16 activation storage. One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from neuralsampleid_amd import functional as F_  # noqa: E402
from neuralsampleid_amd import ops  # noqa: E402
from neuralsampleid_amd._lib import call  # noqa: E402
from neuralsampleid_amd.fingerprint import extract_fingerprints  # noqa: E402
from neuralsampleid_amd.frontend import CQTFrontEnd, cqt_kernels  # noqa: E402

CFG = {"fs": 22050, "hop_len": 512, "n_frames": 216, "overlap": 0.5, "arch": "resnet-ibn"}
LLC_BYTES = 256 << 20


def dense_matrix(front):
    """[re; im] rows of the dense taps, (168, width) fp32, from the same fp64 evaluation the packed table is made of"""
    _, lengths, starts, width, taps = cqt_kernels(front.fs)
    W = np.zeros((2 * front.n_bins, width), dtype=np.float32)
    for k in range(front.n_bins):
        t = taps[k].astype(np.complex64)
        W[k, starts[k]:starts[k] + lengths[k]] = t.real
        W[front.n_bins + k, starts[k]:starts[k] + lengths[k]] = t.imag
    return torch.from_numpy(W).cuda()


def dense_clip(front, W, wave, padded, spec):
    """(b) for one clip: wave (L,) -> (84, T)"""
    L, pad, T, n = wave.numel(), front.width // 2, spec.shape[0], front.n_bins
    s = ops._stream()
    call("nsid_reflect_pad", ops._p(wave), L, pad, ops._p(padded), s)
    call("nsid_linear_fwd", ops._p(padded), front.hop, ops._p(W), ops.F32, None, ops._p(spec), 2 * n, T, 2 * n, front.width, 1,
         None, None, ops.ACT_NONE, ops.ACT_NONE, None, 1, ops.F32, s)
    re, im = spec[:, :n] * front.scale, spec[:, n:] * front.scale
    return torch.sqrt(re * re + im * im).t()


def eager_batch(front, W, waves, mode):
    """(c): waves (B, L) -> (B, 84, T)"""
    pad, n = front.width // 2, front.n_bins
    outs = []
    for lo in range(0, waves.shape[0], 32):
        xp = F.pad(waves[lo:lo + 32, None, :], (pad, pad), mode="reflect")
        if mode == "conv1d":
            y = F.conv1d(xp, W[:, None, :], stride=front.hop)                     # (b, 168, T)
        else:
            y = torch.matmul(xp[:, 0].unfold(-1, front.width, front.hop), W.t()).transpose(1, 2)
        re, im = y[:, :n] * front.scale[None, :, None], y[:, n:] * front.scale[None, :, None]
        outs.append(torch.sqrt(re * re + im * im))
    return torch.cat(outs)


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def graphed(fn):
    fn()                                                                          # warm-up outside the capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            keep = fn()
    torch.cuda.current_stream().wait_stream(s)
    g.keep = keep
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--samples", type=int, default=110250)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense-clips", type=int, default=8)
    ap.add_argument("--eager", choices=("matmul", "conv1d"), default="matmul")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cqt_bench needs an MI355X"
    B, L = args.batch, args.samples
    ops.set_gemm_precision("fp32")
    front = CQTFrontEnd(CFG, "cuda")
    T = front.n_frames_of(L)
    W = dense_matrix(front)
    nbuf = max(2, -(-2 * LLC_BYTES // (B * L * 4)))                               # buffers that together exceed twice the cache
    gen = torch.Generator(device="cuda").manual_seed(5)
    bufs = [0.1 * torch.randn(B, L, device="cuda", generator=gen) for _ in range(nbuf)]

    # all three compute the same thing (fp32 sums in different orders) on the first clips
    ref = front.batch(bufs[0][:2])
    padded, spec = torch.empty(L + front.width, device="cuda"), torch.empty((T, 2 * front.n_bins), device="cuda")
    d_dense = float((dense_clip(front, W, bufs[0][0], padded, spec) - ref[0]).abs().max())
    d_eager = float((eager_batch(front, W, bufs[0][:2], args.eager) - ref).abs().max())

    g_fused = graphed(lambda: [front.batch(w) for w in bufs])
    fused = [t / nbuf for t in event_ms(g_fused.replay, args.reps)]
    nd = args.dense_clips
    g_dense = graphed(lambda: [dense_clip(front, W, bufs[1 + i % (nbuf - 1)][i], padded, spec) for i in range(nd)])
    dense = [t / nd * B for t in event_ms(g_dense.replay, args.reps)]
    it = iter(range(10 ** 9))
    eager = event_ms(lambda: eager_batch(front, W, bufs[next(it) % nbuf], args.eager), args.reps)

    from resnet_ibn_bench import build_model, clips                               # the extraction the front end feeds
    model, specs, extract = build_model(T), clips(B, T), {}
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        F_.set_activation_dtype(dt)
        extract_fingerprints(model, specs, batch=B)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            extract_fingerprints(model, specs, batch=B)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        extract[name] = ts
    F_.set_activation_dtype(torch.float32)

    med = lambda v: float(np.median(v))                                           # noqa: E731
    rec = {"batch": B, "samples": L, "frames": T, "reps": args.reps, "input_buffers": nbuf,
           "fused_ms_all": [round(t, 4) for t in fused], "fused_ms": round(med(fused), 4),
           "dense_ms_extrapolated_all": [round(t, 3) for t in dense], "dense_ms_extrapolated": round(med(dense), 3),
           "dense_clips_timed": nd, "eager_mode": args.eager, "eager_ms_all": [round(t, 3) for t in eager],
           "eager_ms": round(med(eager), 3), "dense_over_fused": round(med(dense) / med(fused), 2),
           "eager_over_fused": round(med(eager) / med(fused), 2),
           "max_abs_diff_dense_vs_fused": d_dense, "max_abs_diff_eager_vs_fused": d_eager,
           "extract_ms": {k: round(med(v), 3) for k, v in extract.items()},
           "fused_share_of_extract": {k: round(med(fused) / med(v), 4) for k, v in extract.items()},
           "fused_banded_gflop_per_s": round(2.0 * B * T * 16 * float(sum(int(g[3]) for g in front.groups)) / med(fused) / 1e6, 1)}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
