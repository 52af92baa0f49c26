"""Times FlatL2Index.search (csrc/search.hip) at the issue's shapes and the whole eval_hit_rates on a synthetic emb_dir.

    python tools/search_bench.py [--reps 5] [--quick]

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


def time_search(nq, nx, d, k, reps):
    g = torch.Generator(device="cuda").manual_seed(0)
    idx = FlatL2Index(d)
    idx.add(_unit(nx, d, g))
    q = _unit(nq, d, g)
    idx.search(q, k)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        idx.search(q, k)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    t = float(np.median(ms))
    tf = 2.0 * nq * nx * d / t / 1e9
    gbs = 4.0 * nx * d / t / 1e6
    print(f"search nq={nq:6d} nx={nx:8d} d={d} k={k}: {t:9.3f} ms  {tf:7.2f} TF/s ({tf / PEAK_TF:5.3f} of 155)  "
          f"{gbs:8.1f} GB/s ({gbs / PEAK_GBS:5.3f} of 8 TB/s)", flush=True)
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
    a = ap.parse_args()
    shapes = [(16384, 1 << 20), (19, 1 << 20)] + ([] if a.quick else [(4096, 5 << 20)])
    for nq, nx in shapes:
        time_search(nq, nx, 128, 20, a.reps)
    time_eval(50_000, 200_000, 19 * 200) if a.quick else time_eval(200_000, 1 << 20, 19 * 1000)


if __name__ == "__main__":
    main()
