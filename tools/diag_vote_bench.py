"""Times ops.diag_vote against the sequence path it replaces (ops.seq_scores + ops.song_vote) on the same search result.

    python tools/diag_vote_bench.py [--reps 20] [--dummy 90000] [--songs 250] [--segs 40] [--tests 1000] [--quick]

(a) tools/identify_bench.py's vote shape: --tests tests x 6 lengths (1 .. 19 rows) at k_probe = 20 on a synthetic index at d = 128.
(b) The windows of locate / scan / links: 1 and 64 windows of 204 rows at k_probe = 20 (4080 candidates each).
Device events around each call (the per-pair tables are uploaded inside, on both sides); the repetitions of the three calls are
interleaved in one process after a warm-up; medians with min and max; the profiler is off."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralsampleid_amd import ops  # noqa: E402
from neuralsampleid_amd.identify import SampleIndex  # noqa: E402
from neuralsampleid_amd.search import extract_test_ids, make_pairs  # noqa: E402

DEV = "cuda"
D = 128
SEQ = (1, 3, 5, 9, 11, 19)


def _unit(g, n):
    x = torch.randn(n, D, device=DEV, generator=g)
    return x / x.norm(dim=1, keepdim=True)


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _fmt(v):
    return f"{np.median(v):9.3f} ms (min {np.min(v):.3f}, max {np.max(v):.3f})"


def compare(idx, q, starts, lens, reps, what):
    k = 20
    _, I = idx._index.search(q, k)
    song_of, ldo = idx._song_of[: idx.n_ref], int(np.max(lens)) * k
    scores = ops.seq_scores(q, idx._index.xb, I, starts, lens, ldo)
    calls = {"ops.seq_scores": lambda: ops.seq_scores(q, idx._index.xb, I, starts, lens, ldo),
             "ops.song_vote": lambda: ops.song_vote(I, scores, starts, lens, song_of, idx.n_dummy, None, 10),
             "ops.diag_vote": lambda: ops.diag_vote(I, starts, lens, song_of, idx.n_dummy, None, 16, 10)}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    t = {name: [] for name in calls}
    for _ in range(reps):                          # interleaved: A B C A B C ...
        for name, fn in calls.items():
            t[name].append(_event_ms(fn))
    print(f"{what}: {len(starts)} pairs, {int((np.asarray(lens) * k).sum())} candidates")
    for name in calls:
        print(f"  {name:16s} {_fmt(t[name])}")
    seq = np.asarray(t["ops.seq_scores"]) + np.asarray(t["ops.song_vote"])
    print(f"  seq_scores + song_vote {_fmt(seq)}; diag_vote / that = {np.median(t['ops.diag_vote']) / np.median(seq):.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dummy", type=int, default=90000)
    ap.add_argument("--songs", type=int, default=250)
    ap.add_argument("--segs", type=int, default=40)
    ap.add_argument("--tests", type=int, default=1000)
    ap.add_argument("--quick", action="store_true", help="a small index and 100 tests")
    a = ap.parse_args()
    if a.quick:
        a.dummy, a.songs, a.tests, a.reps = 9000, 25, 100, min(a.reps, 5)
    g = torch.Generator(device=DEV).manual_seed(0)
    with torch.no_grad():
        idx = SampleIndex(None, device=DEV)
        idx.add_dummy(_unit(g, a.dummy))
        for s in range(a.songs):
            idx.add_rows(f"s{s}", _unit(g, a.segs))
        print(f"index: {idx.n_dummy} dummy + {idx.n_ref} ref rows ({a.songs} songs x {a.segs}), d {D}, k_probe 20", flush=True)
        L = SEQ[-1]
        rng = np.random.default_rng(1)
        firsts = rng.integers(0, idx.n_ref - L, size=a.tests)
        ref = idx.fingerprints
        q = torch.cat([ref[int(f): int(f) + L] for f in firsts])
        q = q + 0.5 * torch.randn(q.shape, device=DEV, generator=g) / D ** 0.5
        q = (q / q.norm(dim=1, keepdim=True)).contiguous()
        starts, lens = extract_test_ids([f"q{t}_{t}" for t in range(a.tests) for _ in range(L)])
        _, _, ps, pl = make_pairs(starts, lens, SEQ)
        compare(idx, q, ps, pl, a.reps, "(a) evaluation form")
        W = ops.VOTE_MAX_CAND // 20
        for n in (1, 64):
            rows = _unit(g, n * W).contiguous()
            compare(idx, rows, [w * W for w in range(n)], [W] * n, a.reps, f"(b) windows of {W} rows")


if __name__ == "__main__":
    main()
