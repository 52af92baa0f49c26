"""Times neuralsampleid_amd.identify on a synthetic index: (a) one query of 19 segments against about 100 k rows at d = 128, per
stage and in total, with and without the classifier re-rank; (b) the evaluation's form, about 1 000 tests x 6 lengths at
k_probe = 20 on the same I and scores: ops.song_vote against the file-based path's vote (copy I and the scores to the host, then
search.aggregate_hit_rates), interleaved repetitions in one process.

    python tools/identify_bench.py [--reps 20] [--dummy 90000] [--songs 250] [--segs 40] [--tests 1000] [--quick]

Stage times: device events around the stage's launches, median of --reps after a warm-up (an event pair on an idle GPU also sees
the launch latency: these stages are a few launches each, so that is part of what a caller waits for). Totals: host clock around
the call, which ends with the results on the host. Only rows with node matrices (the --songs x --segs reference rows) keep a
[K | P] block; the dummy rows cost 4 d bytes each."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralsampleid_amd import ops  # noqa: E402
from neuralsampleid_amd.classifier import CrossAttentionClassifier  # noqa: E402
from neuralsampleid_amd.identify import SampleIndex  # noqa: E402
from neuralsampleid_amd.search import aggregate_hit_rates, extract_test_ids, make_pairs  # noqa: E402

DEV = "cuda"
D, C, N = 128, 512, 32
SEQ = (1, 3, 5, 9, 11, 19)


def _events_ms(fn, reps):
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
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def _host_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def _fmt(t):
    return f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def _unit(g, n):
    x = torch.randn(n, D, device=DEV, generator=g)
    return x / x.norm(dim=1, keepdim=True)


def build_index(a, g):
    torch.manual_seed(0)
    clf = CrossAttentionClassifier(in_dim=C, num_nodes=N).to(DEV).eval()
    idx = SampleIndex(None, classifier=clf, device=DEV)
    idx.add_dummy(_unit(g, a.dummy))
    t0 = time.perf_counter()
    for s in range(a.songs):
        idx.add_rows(f"s{s}", _unit(g, a.segs), torch.randn(a.segs, C, N, device=DEV, generator=g))
    torch.cuda.synchronize()
    print(f"index: {idx.n_dummy} dummy + {idx.n_ref} ref rows ({a.songs} songs x {a.segs}), d {D}; [K | P] {idx.kp_bytes_per_segment} B per "
          f"ref segment = {idx.kp_bytes_per_segment * idx.n_ref / 2 ** 30:.2f} GiB; add_rows of all songs {time.perf_counter() - t0:.2f} s",
          flush=True)
    return idx, clf


def noisy_rows(idx, g, first, n, sigma=0.5):
    """n consecutive reference rows from `first` on, with noise, re-normalised: a query that samples them"""
    rows = idx.fingerprints[first: first + n]
    x = rows + sigma * torch.randn(n, D, device=DEV, generator=g) / D ** 0.5
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def one_query(idx, clf, a, g):
    L, k = 19, 20
    fp = noisy_rows(idx, g, 7 * a.segs + 3, L)
    nodes = torch.randn(L, C, N, device=DEV, generator=g)
    xb, song_of, song_of_nodes = idx._index.xb, idx._song_of[: idx.n_ref], idx._song_of_nodes[: idx.n_ref]
    kp, tail = idx._kp[: idx.n_ref * N], clf.folded()[4]
    with torch.no_grad():
        _, I = idx._index.search(fp, k)
        scores = ops.seq_scores(fp, xb, I, [0], [L], L * k)
        cidx = ops.vote_candidates(I, idx.n_dummy, idx.n_ref).reshape(-1)
        q = clf.project_queries(nodes)
        S, _ = ops.clf_pair_scores_dev(q, kp, N, tail, [0], [L], [L * k], cidx)
        print(f"(a) one query: {L} segments, k_probe {k}: {L * k} candidates, {L} x {L * k} = {L * L * k} classifier pairs", flush=True)
        r = a.reps
        print(f"  search                {_fmt(_events_ms(lambda: idx._index.search(fp, k), r))}")
        print(f"  seq_scores            {_fmt(_events_ms(lambda: ops.seq_scores(fp, xb, I, [0], [L], L * k), r))}")
        print(f"  song_vote             {_fmt(_events_ms(lambda: ops.song_vote(I, scores, [0], [L], song_of, idx.n_dummy, None, 10), r))}")
        print(f"  identify, total        {_fmt(_host_ms(lambda: idx.identify(fp=fp, k_probe=k, top=10), r))}")
        print(f"  vote_candidates       {_fmt(_events_ms(lambda: ops.vote_candidates(I, idx.n_dummy, idx.n_ref), r))}")
        print(f"  project_queries       {_fmt(_events_ms(lambda: clf.project_queries(nodes), r))}")
        print(f"  clf_pair_scores_dev   {_fmt(_events_ms(lambda: ops.clf_pair_scores_dev(q, kp, N, tail, [0], [L], [L * k], cidx), r))}")
        print(f"  song_vote_clf         "
              f"{_fmt(_events_ms(lambda: ops.song_vote_clf(I, S, [0], [L * k], [0], [L], song_of_nodes, idx.n_dummy, None, 0.5, 10), r))}")
        print(f"  identify rerank, total {_fmt(_host_ms(lambda: idx.identify(fp=fp, nodes=nodes, k_probe=k, top=10, rerank=True), r))}",
              flush=True)


def evaluation_form(idx, a, g):
    k, L = 20, 19
    T = a.tests
    rng = np.random.default_rng(1)
    firsts = rng.integers(0, idx.n_ref - L, size=T)
    q = torch.cat([noisy_rows(idx, g, int(f), L) for f in firsts])
    query_lookup = [f"q{t}_{t}" for t in range(T) for _ in range(L)]
    ref_lookup = [idx.names[c] for c in idx._song_of[: idx.n_ref].cpu().tolist()]
    gt = {}
    for t, f in enumerate(firsts.tolist()):
        gt.setdefault(ref_lookup[f], []).append(f"q{t}")
    starts, lens = extract_test_ids(query_lookup)
    _, _, ps, pl = make_pairs(starts, lens, SEQ)
    _, I = idx._index.search(q, k)
    scores = ops.seq_scores(q, idx._index.xb, I, ps, pl, L * k)
    song_of = idx._song_of[: idx.n_ref]
    torch.cuda.synchronize()
    print(f"(b) evaluation form: {T} tests x {len(SEQ)} lengths = {ps.size} pairs, k_probe {k}: I {tuple(I.shape)}, scores "
          f"{tuple(scores.shape)}, {int((pl * k).sum())} candidates", flush=True)

    def device_vote():
        songs, totals, n = ops.song_vote(I, scores, ps, pl, song_of, idx.n_dummy, None, 10)
        return songs.cpu(), totals.cpu(), n.cpu()

    def host_copy():
        return I.cpu().numpy(), scores.cpu().numpy()

    def host_vote():
        Ih, sh = host_copy()
        return aggregate_hit_rates(Ih, sh, query_lookup, ref_lookup, idx.n_dummy, gt, SEQ)

    # the two sides agree on top-1 before anything is timed
    songs, _, _ = device_vote()
    _, raw, _ = host_vote()
    ti, si, _, _ = make_pairs(starts, lens, SEQ)
    qid_hit = np.array([ref_lookup[firsts[t]] == (idx.names[c] if c >= 0 else None) for t, c in zip(ti, songs[:, 0].tolist())])
    top1 = np.zeros((T, len(SEQ)), dtype=bool)
    top1[ti, si] = qid_hit
    assert np.array_equal(top1, raw[:, :len(SEQ)].astype(bool)), "device and host votes disagree on top-1"
    dev, host, copy, kern = [], [], [], []
    for _ in range(a.reps):                        # interleaved: A B A B ...
        for fn, out in ((device_vote, dev), (host_vote, host), (host_copy, copy)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
    kern = _events_ms(lambda: ops.song_vote(I, scores, ps, pl, song_of, idx.n_dummy, None, 10), a.reps)
    st = lambda v: (float(np.median(v)), float(np.min(v)), float(np.max(v)))
    print(f"  ops.song_vote, launch alone (events; starts / lens uploaded inside)   {_fmt(kern)}")
    print(f"  ops.song_vote + top-10 songs, totals and n_songs on the host           {_fmt(st(dev))}")
    print(f"  file-based path: I and scores to the host + aggregate_hit_rates        {_fmt(st(host))}")
    print(f"    of which the two copies                                              {_fmt(st(copy))}")
    print(f"  top-1 hit rate per length (both sides): {np.round(100 * top1.mean(0), 1).tolist()}", flush=True)


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
        a.dummy, a.songs, a.tests = 9000, 25, 100
    g = torch.Generator(device=DEV).manual_seed(0)
    idx, clf = build_index(a, g)
    one_query(idx, clf, a, g)
    evaluation_form(idx, a, g)


if __name__ == "__main__":
    main()
