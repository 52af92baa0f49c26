"""Times the leave-one-out search and the catalogue self-join (SampleIndex.links) on a synthetic catalogue: unit rows that correlate with
their neighbours (overlapping segments) plus plants between songs.

    python tools/links_bench.py [--reps 10] [--nq 65536] [--nx 1048576] [--d 128] [--k 20] [--songs 200] [--seg 300] [--quick]

One JSON line with
  search:  ops.flat_l2_topk_excl against ops.flat_l2_topk of the same library at the same (nq, nx, d, k): the queries are database
           rows, every query row leaves out the --seg rows of its own "song"; device events around the call, repetitions interleaved
           (A B A B ...), median / min / max in ms.
  links:   SampleIndex.links over --songs songs of --seg rows (every third song samples its neighbour), host clock, results on the
           host, in songs/s; and the per-song loop of locate(fp=rows, leave_out=name) over the same songs, whose results are checked
           equal to links' before anything is timed."""
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
THETA, MIN_SCORE = 0.6, 2.0


def _st(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4)}


def _unit(g, n, d, slab=1 << 18):
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


def search_case(g, nq, nx, d, k, seg, reps):
    x = _unit(g, nx, d)
    xn = ops.row_sqnorm(x)
    pick = torch.randperm(nx, device=DEV, generator=g)[:nq].sort().values
    q = x[pick].contiguous()
    qn = ops.row_sqnorm(q)
    lo = (pick // seg * seg).to(torch.int32)
    hi = (lo + seg).clamp(max=nx).to(torch.int32)
    plain = lambda: ops.flat_l2_topk(q, x, xn, k, qn)
    excl = lambda: ops.flat_l2_topk_excl(q, x, xn, k, lo, hi, qn)
    (_, Ip), (_, Ie) = plain(), excl()
    torch.cuda.synchronize()
    own = float(((Ip >= lo[:, None]) & (Ip < hi[:, None])).float().mean())
    assert not ((Ie >= lo[:, None]) & (Ie < hi[:, None])).any()
    tp, te = [], []
    for _ in range(reps):
        tp.append(_event_ms(plain))
        te.append(_event_ms(excl))
    return {"nq": nq, "nx": nx, "d": d, "k": k, "range_rows": seg, "plain": _st(tp), "excl": _st(te),
            "excl_over_plain": round(float(np.median(te) / np.median(tp)), 4),
            "plain_slots_taken_by_own_song": round(own, 4), "tflops_excl": round(2.0 * nq * nx * d / np.median(te) / 1e9, 2)}


def links_case(g, songs, seg, d, reps):
    idx = SampleIndex(None, device=DEV)
    idx.add_dummy(_unit(g, 2000, d))
    rows = _unit(g, songs * seg, d).view(songs, seg, d)
    for s in range(0, songs - 1, 3):                                 # song s samples song s + 1: 24 rows at rates 0.75 / 1.0 / 1.5 in turn
        rate = (0.75, 1.0, 1.5)[(s // 3) % 3]
        t = torch.arange(24, device=DEV)
        v = rows[s + 1, 30 + torch.round(t * rate).long()] + 0.5 * torch.randn(24, d, device=DEV, generator=g) / d ** 0.5
        rows[s, 100:124] = v / v.norm(dim=1, keepdim=True)
    for s in range(songs):
        idx.add_rows(f"s{s}", rows[s])
    kw = dict(k_probe=20, n_songs=5, threshold=THETA, min_score=MIN_SCORE)
    fps = {n: idx.fingerprints[lo:lo + m] for n, (lo, m, _) in zip(idx.names, idx._song_rows)}
    run_links = lambda: idx.links(**kw)
    run_loop = lambda: {n: idx.locate(fp=fps[n], leave_out=n, **kw) for n in idx.names}
    res, loop = run_links(), run_loop()
    assert res.skipped == [] and res.occurrences == loop, "links and the loop of locate disagree"
    ops.launch_counters(reset=True)
    run_links()
    c = ops.launch_counters()
    tl, tp = [], []
    for _ in range(reps):
        for fn, dst in ((run_links, tl), (run_loop, tp)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dst.append(1e3 * (time.perf_counter() - t0))
    found = sum(1 for v in res.occurrences.values() if v)
    return {"songs": songs, "rows_per_song": seg, "d": d, "dummy_rows": idx.n_dummy, "songs_with_a_link": found,
            "planted_pairs": len(range(0, songs - 1, 3)), "links": _st(tl), "loop_of_locate": _st(tp),
            "links_songs_per_s": round(1e3 * songs / float(np.median(tl)), 1),
            "loop_songs_per_s": round(1e3 * songs / float(np.median(tp)), 1),
            "loop_over_links": round(float(np.median(tp) / np.median(tl)), 3),
            "links_launches": {k: c[k] for k in ("flat_l2_topk_excl", "seq_scores", "song_vote", "pair_sim", "local_align")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--nq", type=int, default=65536)
    ap.add_argument("--nx", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--songs", type=int, default=200)
    ap.add_argument("--seg", type=int, default=300)
    ap.add_argument("--no-links", action="store_true", help="the search comparison alone")
    ap.add_argument("--quick", action="store_true", help="a small database, a small catalogue, 3 repetitions")
    a = ap.parse_args()
    if a.quick:
        a.reps, a.nq, a.nx, a.songs = min(a.reps, 3), min(a.nq, 4096), min(a.nx, 1 << 16), min(a.songs, 24)
    g = torch.Generator(device=DEV).manual_seed(0)
    out = {"tool": "links_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps}
    with torch.no_grad():
        out["search"] = search_case(g, a.nq, a.nx, a.d, a.k, a.seg, a.reps)
        if not a.no_links:
            out["links"] = links_case(g, a.songs, a.seg, 128, a.reps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
