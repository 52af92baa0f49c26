"""Times the normalised candidate search against the exact search on the same operands, and one scan with and without norm_search.

    python tools/norm_search_bench.py [--reps 10] [--k 20] [--cohort 4096] [--quick] [--no-scan]

One JSON line with
  search:  per shape (nq x nx at d; 19 x 100 000 and 16 384 x 2^20 at d = 128, 8 192 x 262 144 at d = 2048: identify_bench's and
           links_bench's shapes) ops.flat_norm_topk against ops.flat_l2_topk of the same library, the statistics and the norms made
           before the clock starts; device events around the call, repetitions interleaved (A B A B ...), median / min / max in ms. The
           expectation is the exact search's time plus five flops and two loads per cell's column; "plain_spread" = (max - min) /
           median of the exact search's own runs is what a ratio has to exceed to mean anything.
  scan:    SampleIndex.scan(vote="diagonal", normalize=True) of a recording of --scan-rows rows over a catalogue of --songs songs of
           --seg rows behind --dummy dummy rows, with and without norm_search=True, host clock, interleaved; the statistics of the index
           rows are cached by a first call outside the clock, as they are in a resident index."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralsampleid_amd import ops  # noqa: E402
from neuralsampleid_amd.identify import SampleIndex  # noqa: E402

DEV = "cuda"
SHAPES = [(19, 100_000, 128), (16_384, 1 << 20, 128), (8_192, 262_144, 2048)]
QUICK = [(19, 20_000, 128), (1_024, 1 << 16, 128), (512, 1 << 14, 2048)]
THETA, MIN_SCORE = 2.5, 10.0


def _st(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4)}


def _unit(g, n, d, slab=1 << 16):
    """rows that correlate with their neighbours (a sum of 8 consecutive frames), unit length, made in slabs"""
    out = torch.empty((n, d), device=DEV)
    for a in range(0, n, slab):
        m = min(slab, n - a)
        f = torch.randn(m + 7, d, device=DEV, generator=g)
        x = sum(f[t:t + m] for t in range(8))
        out[a:a + m] = x / x.norm(dim=1, keepdim=True)
    return out


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def search_case(g, nq, nx, d, k, M, reps):
    x = _unit(g, nx, d)
    pick = torch.randperm(nx, device=DEV, generator=g)[:nq]
    q = x[pick] + 0.5 * torch.randn(nq, d, device=DEV, generator=g) / d ** 0.5
    q = (q / q.norm(dim=1, keepdim=True)).contiguous()
    cohort = x[torch.arange(M, device=DEV) * (nx // M)].contiguous()
    xn, qn = ops.row_sqnorm(x), ops.row_sqnorm(q)
    slabs = [ops.cohort_stats(x[a:a + (1 << 18)], cohort) for a in range(0, nx, 1 << 18)]       # the workspace grows with the rows
    x_stats = tuple(torch.cat(parts) for parts in zip(*slabs))
    norm = ops.cohort_stats(q, cohort) + x_stats
    plain = lambda: ops.flat_l2_topk(q, x, xn, k, qn)
    normed = lambda: ops.flat_norm_topk(q, x, norm, k)
    (_, Ip), (Z, In) = plain(), normed()
    torch.cuda.synchronize()
    assert (In >= 0).all() and (Z[:, :-1] >= Z[:, 1:]).all()
    tp, tn = [], []
    for _ in range(reps):
        tp.append(_event_ms(plain))
        tn.append(_event_ms(normed))
    med = float(np.median(tp))
    return {"nq": nq, "nx": nx, "d": d, "k": k, "cohort": M, "plain": _st(tp), "norm": _st(tn),
            "norm_over_plain": round(float(np.median(tn)) / med, 4), "plain_spread": round((max(tp) - min(tp)) / med, 4),
            "first_hit_shared": round(float((Ip[:, 0] == In[:, 0]).float().mean()), 4),
            "tflops_plain": round(2.0 * nq * nx * d / med / 1e9, 2), "tflops_norm": round(2.0 * nq * nx * d / float(np.median(tn)) / 1e9, 2)}


def scan_case(g, dummy, songs, seg, rows, d, k, M, reps):
    idx = SampleIndex(None, device=DEV)
    idx.add_dummy(_unit(g, dummy, d))
    cat = _unit(g, songs * seg, d).view(songs, seg, d)
    for s in range(songs):
        idx.add_rows(f"s{s}", cat[s])
    idx.set_cohort(size=M)
    rec = _unit(g, rows, d)
    for n, a in enumerate(range(50, rows - 40, 400)):                 # an excerpt of a song every 400 rows
        v = cat[n % songs, 30:62] + 0.5 * torch.randn(32, d, device=DEV, generator=g) / d ** 0.5
        rec[a:a + 32] = v / v.norm(dim=1, keepdim=True)
    kw = dict(fp=rec, threshold=THETA, min_score=MIN_SCORE, k_probe=k, vote="diagonal", normalize=True)
    runs = {"l2": lambda: idx.scan(**kw), "norm": lambda: idx.scan(norm_search=True, **kw)}
    found = {name: len(fn()) for name, fn in runs.items()}            # also fills the cached statistics
    t = {name: [] for name in runs}
    for _ in range(reps):
        for name, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append(1e3 * (time.perf_counter() - t0))
    return {"dummy_rows": dummy, "songs": songs, "rows_per_song": seg, "recording_rows": rows, "d": d, "k": k, "cohort": M,
            "planted": len(range(50, rows - 40, 400)), "occurrences": found, "scan_l2_search": _st(t["l2"]),
            "scan_norm_search": _st(t["norm"]), "norm_over_l2": round(float(np.median(t["norm"]) / np.median(t["l2"])), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--cohort", type=int, default=4096)
    ap.add_argument("--dummy", type=int, default=100_000)
    ap.add_argument("--songs", type=int, default=200)
    ap.add_argument("--seg", type=int, default=300)
    ap.add_argument("--scan-rows", type=int, default=4000)
    ap.add_argument("--no-scan", action="store_true", help="the search comparison alone")
    ap.add_argument("--quick", action="store_true", help="small shapes, 3 repetitions")
    a = ap.parse_args()
    shapes = SHAPES
    if a.quick:
        shapes, a.reps, a.dummy, a.songs, a.scan_rows = QUICK, min(a.reps, 3), min(a.dummy, 8192), min(a.songs, 24), min(a.scan_rows, 800)
    g = torch.Generator(device=DEV).manual_seed(0)
    out = {"tool": "norm_search_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "search": []}
    with torch.no_grad():
        for nq, nx, d in shapes:
            out["search"].append(search_case(g, nq, nx, d, a.k, a.cohort, a.reps))
            torch.cuda.empty_cache()
        if not a.no_scan:
            out["scan"] = scan_case(g, a.dummy, a.songs, a.seg, a.scan_rows, 128, a.k, a.cohort, a.reps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
