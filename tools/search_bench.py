"""Times FlatL2Index.search (csrc/search.hip) at the issue's shapes and the whole eval_hit_rates on a synthetic emb_dir.

    python tools/search_bench.py [--reps 5] [--quick] [--d 128] [--eager]

--d 2048 times the wide kernel at (4096, 1 << 20) and (19, 1 << 20): the ResNet-IBN baseline's fingerprints, an 8 GB database.
--eager adds a torch-eager fp32 yardstick in the same process: over database chunks, torch.topk(xn[None, :] - 2 * q @ xc.T, k,
largest=False), then a final top-k over the chunk winners.

Rooflines: the fp32 matrix pipe (155 TF measured, MI355X_MICROARCH) for 2 nq nx d flop, and HBM (8 TB/s) for 4 nx d bytes
(one pass over the database). Prints one line per shape: ms (median of --reps after a warm-up), TFLOP/s and its fraction of
155 TF, GB/s and its fraction of 8 TB/s."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralsampleid_amd import fpdb  # noqa: E402
from neuralsampleid_amd.search import FlatL2Index, eval_hit_rates  # noqa: E402

PEAK_TF, PEAK_GBS = 155.0, 8000.0


def _unit(n, d, g):
    x = torch.randn(n, d, device="cuda", generator=g)
    return x / x.norm(dim=1, keepdim=True)


EAGER_SCORES = 1 << 28          # elements of the yardstick's nq x chunk score matrix at most (1 GB)
ADD_ROWS = 1 << 17              # rows per add(): the generator's temporaries stay small next to an 8 GB database


def eager_topk(q, x, xn, k):
    """the torch-eager fp32 yardstick: chunked GEMM + topk, then a top-k over the chunk winners"""
    step = max(k, EAGER_SCORES // max(1, q.shape[0]))
    vals, ids = [], []
    for a in range(0, x.shape[0], step):
        xc = x[a:a + step]
        v, i = torch.topk(xn[None, a:a + step] - 2 * q @ xc.T, min(k, xc.shape[0]), largest=False)
        vals.append(v)
        ids.append(i + a)
    v, pos = torch.topk(torch.cat(vals, 1), k, largest=False)
    return v, torch.cat(ids, 1).gather(1, pos)


def _time(fn, reps):
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
    return ms


def _line(what, ms, nq, nx, d, k):
    t = float(np.median(ms))
    tf = 2.0 * nq * nx * d / t / 1e9
    gbs = 4.0 * nx * d / t / 1e6
    print(f"{what} nq={nq:6d} nx={nx:8d} d={d} k={k}: {t:9.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})  {tf:7.2f} TF/s "
          f"({tf / PEAK_TF:5.3f} of 155)  {gbs:8.1f} GB/s ({gbs / PEAK_GBS:5.3f} of 8 TB/s)", flush=True)


def time_search(nq, nx, d, k, reps, eager=False):
    g = torch.Generator(device="cuda").manual_seed(0)
    idx = FlatL2Index(d)
    for a in range(0, nx, ADD_ROWS):
        idx.add(_unit(min(ADD_ROWS, nx - a), d, g))
    q = _unit(nq, d, g)
    _line("search", _time(lambda: idx.search(q, k), reps), nq, nx, d, k)
    if eager:
        x, xn = idx.xb, idx._norm[:nx]
        _line("eager ", _time(lambda: eager_topk(q, x, xn, k), reps), nq, nx, d, k)
        same = float((eager_topk(q, x, xn, k)[1] == idx.search(q, k)[1]).float().mean())
        print(f"       ids equal to the fused search's: {100 * same:.3f} %", flush=True)
    del idx
    torch.cuda.empty_cache()


def time_eval(n_ref, n_dummy, n_query, d=128):
    rng = np.random.default_rng(0)

    def unit(n):
        x = rng.standard_normal((n, d)).astype(np.float32)
        return x / np.linalg.norm(x, axis=1, keepdims=True)

    with tempfile.TemporaryDirectory() as tmp:
        songs = n_ref // 50
        ref = unit(n_ref)
        fpdb.write_fp_db(tmp, "ref_db", ref, [f"s{i // 50}" for i in range(n_ref)])
        fpdb.write_fp_db(tmp, "dummy_db", unit(n_dummy), ["dummy"] * n_dummy)
        qrows = ref[:n_query] + 0.3 * rng.standard_normal((n_query, d)).astype(np.float32) / np.sqrt(d)
        fpdb.write_fp_db(tmp, "query_db", qrows, [f"q{i // 19}_{i // 19}" for i in range(n_query)])
        gt = {f"s{i}": [f"q{j}" for j in range(n_query // 19 + 1) if (j * 19) // 50 == i] for i in range(songs)}
        eval_hit_rates(tmp, gt, save=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hr = eval_hit_rates(tmp, gt, save=False)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
    print(f"eval_hit_rates ref={n_ref} dummy={n_dummy} query rows={n_query}: {t * 1e3:.1f} ms (top-1 at sl=1: {hr[0, 0]:.1f} %)",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the first two shapes only, and a small evaluation")
    ap.add_argument("--d", type=int, default=128, help="fingerprint width; above 256 the wide kernel and its two shapes")
    ap.add_argument("--eager", action="store_true", help="also time the torch-eager fp32 yardstick on every shape")
    a = ap.parse_args()
    if a.d > 256:                                   # 8 GB of database at d = 2048; the evaluation is timed at GraFP's width only
        shapes = [(4096, 1 << 20), (19, 1 << 20)]
    else:
        shapes = [(16384, 1 << 20), (19, 1 << 20)] + ([] if a.quick else [(4096, 5 << 20)])
    for nq, nx in shapes:
        time_search(nq, nx, a.d, 20, a.reps, a.eager)
    if a.d <= 256:
        time_eval(50_000, 200_000, 19 * 200, a.d) if a.quick else time_eval(200_000, 1 << 20, 19 * 1000, a.d)


if __name__ == "__main__":
    main()
