"""Times the exact search with and without the certified bf16 pre-filter (FlatL2Index.search(prefilter=...)) in one process.

    python tools/search_prefilter_bench.py [--reps 5] [--nx 1048576] [--d 128] [--k 20] [--quick] [--only NAME ...]

One JSON line. Per shape: the plain search (A) against the pre-filtered search with its fallback (B), repetitions interleaved
A B A B, device events around the whole call, median / min / max in ms, and the fraction of rows the pre-filter certified. The two
results are checked bitwise equal before anything is timed. Shapes, all at d = 128, k = 20:
  random_16k:  16 384 queries near database rows over 2^20 unit random rows
  loo_64k:     65 536 x 2^20 leave-one-out on tools/links_bench.py's correlated rows (every query leaves out its own 300 rows)
  rows_19:     19 x 2^20
  links_small / links_large: SampleIndex.links over 200 x 300 and over 2000 x 300 rows (host clock, songs/s)
The catalogues are synthetic; the certified fraction on real fingerprints is not known from this tool."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from neuralsampleid_amd import ops  # noqa: E402
from neuralsampleid_amd.identify import SampleIndex  # noqa: E402
from neuralsampleid_amd.search import FlatL2Index  # noqa: E402
from links_bench import DEV, MIN_SCORE, THETA, _event_ms, _st, _unit  # noqa: E402


def _same(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def search_case(name, idx, q, k, exclude, reps):
    plain = lambda: idx.search(q, k, exclude=exclude, prefilter=False)
    pre = lambda: idx.search(q, k, exclude=exclude, prefilter=True)
    idx.prefilter_stats.update(rows=0, certified=0, fell_back=0, bypassed=0)
    a, b = plain(), pre()
    assert _same(a, b), f"{name}: the pre-filtered search differs from the plain search"
    stats = dict(idx.prefilter_stats)
    # the pre-filter's own launches, once, on the first query block
    prof = {}
    ta, tb = [], []
    for _ in range(reps):
        ta.append(_event_ms(plain))
        tb.append(_event_ms(pre))
    ops.PROFILE = ops.KernelProfile()
    pre()
    for kname, v in ops.PROFILE.summary().items():
        prof[kname] = round(v["ms"], 3)
    ops.PROFILE = None
    return {"nq": int(q.shape[0]), "nx": idx.ntotal, "d": idx.d, "k": k, "leave_one_out": exclude is not None,
            "plain": _st(ta), "prefilter": _st(tb), "plain_over_prefilter": round(float(np.median(ta) / np.median(tb)), 3),
            "certified_fraction": round(stats["certified"] / max(1, stats["rows"]), 5), "fell_back_rows": stats["fell_back"],
            "prefilter_kernels_ms": prof}


def links_case(g, songs, seg, d, reps):
    dummy = _unit(g, 2000, d)
    rows = _unit(g, songs * seg, d).view(songs, seg, d)
    for s in range(0, songs - 1, 3):
        rate = (0.75, 1.0, 1.5)[(s // 3) % 3]
        t = torch.arange(24, device=DEV)
        v = rows[s + 1, 30 + torch.round(t * rate).long()] + 0.5 * torch.randn(24, d, device=DEV, generator=g) / d ** 0.5
        rows[s, 100:124] = v / v.norm(dim=1, keepdim=True)
    idxs = []
    for pre in (False, True):
        idx = SampleIndex(None, device=DEV, prefilter=pre)
        idx.add_dummy(dummy)
        for s in range(songs):
            idx.add_rows(f"s{s}", rows[s])
        idxs.append(idx)
    kw = dict(k_probe=20, n_songs=5, threshold=THETA, min_score=MIN_SCORE)
    ra, rb = idxs[0].links(**kw), idxs[1].links(**kw)
    assert ra.skipped == rb.skipped == [] and ra.occurrences == rb.occurrences, "links differ with the pre-filter"
    stats = dict(idxs[1]._index.prefilter_stats)
    ta, tb = [], []
    for _ in range(reps):
        for idx, dst in ((idxs[0], ta), (idxs[1], tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            idx.links(**kw)
            torch.cuda.synchronize()
            dst.append(1e3 * (time.perf_counter() - t0))
    return {"songs": songs, "rows_per_song": seg, "d": d, "plain": _st(ta), "prefilter": _st(tb),
            "plain_songs_per_s": round(1e3 * songs / float(np.median(ta)), 1),
            "prefilter_songs_per_s": round(1e3 * songs / float(np.median(tb)), 1),
            "plain_over_prefilter": round(float(np.median(ta) / np.median(tb)), 3),
            "certified_fraction": round(stats["certified"] / max(1, stats["rows"]), 5), "fell_back_rows": stats["fell_back"]}


def main():
    names = ["random_16k", "loo_64k", "rows_19", "links_small", "links_large"]
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nx", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--seg", type=int, default=300)
    ap.add_argument("--only", nargs="*", default=names, choices=names)
    ap.add_argument("--quick", action="store_true", help="a small database and small catalogues, 2 repetitions")
    a = ap.parse_args()
    scale = 16 if a.quick else 1
    if a.quick:
        a.reps, a.nx = min(a.reps, 2), min(a.nx, 1 << 16)
    g = torch.Generator(device=DEV).manual_seed(0)
    out = {"tool": "search_prefilter_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps}
    with torch.no_grad():
        if "random_16k" in a.only or "rows_19" in a.only:
            x = torch.randn(a.nx, a.d, device=DEV, generator=g)
            x /= x.norm(dim=1, keepdim=True)
            idx = FlatL2Index(a.d, DEV, prefilter=True)
            idx.add(x)
            for name, nq in (("random_16k", 16384 // scale), ("rows_19", 19)):
                if name in a.only:
                    pick = torch.randint(0, a.nx, (nq,), device=DEV, generator=g)
                    q = x[pick] + 0.3 * torch.randn(nq, a.d, device=DEV, generator=g) / a.d ** 0.5
                    out[name] = search_case(name, idx, q.contiguous(), a.k, None, a.reps)
            del idx, x
        if "loo_64k" in a.only:
            x = _unit(g, a.nx, a.d)
            idx = FlatL2Index(a.d, DEV, prefilter=True)
            idx.add(x)
            pick = torch.randperm(a.nx, device=DEV, generator=g)[:65536 // scale].sort().values
            lo = pick // a.seg * a.seg
            hi = (lo + a.seg).clamp(max=a.nx)
            out["loo_64k"] = search_case("loo_64k", idx, x[pick].contiguous(), a.k, (lo.cpu(), hi.cpu()), a.reps)
            del idx, x
        if "links_small" in a.only:
            out["links_small"] = links_case(g, 200 // (8 if a.quick else 1), a.seg, 128, a.reps)
        if "links_large" in a.only:
            out["links_large"] = links_case(g, 2000 // (8 if a.quick else 1), a.seg, 128, max(1, a.reps // 2))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
