"""Times the scan of a long recording (SampleIndex.scanner, ops.local_align_strip) on synthetic rows at d = 128.

    python tools/scan_bench.py [--reps 9] [--quick] [--vote diagonal] [--no-walk]

(a) The walk. 32 pairs of 4096 x 4096 through nsid_local_align in one launch, against the same S through nsid_local_align_strip in
    strips of 204 rows (the scanner's window at k_probe = 20) with the carry chained: 21 launches. Device events around the launches
    alone (tables on the device before), us per query row, and nsid_align_occurrences over the strips' rows (the one launch forms its
    occurrences itself). The strips' row results and the occurrences are checked equal to the one launch's before anything is timed.
    The difference is what the strips cost: per strip one launch, the LDS fill from the carry and its store
    (2 rows x 12 bytes x the song's rows, read and written), and a walk that starts with an empty pipeline.
(b) End to end. A 2-hour recording (14 063 rows at 0.512 s per row) with planted excerpts against a catalogue of the size
    tools/identify_bench.py uses (90 000 dummy rows + 250 songs x 40 rows): scan(fp=...) at the defaults, host clock, results on the
    host: ms per window, the total, and the multiple of real time. The excerpts are planted at a window's second row and 100 rows
    inside a window. With --vote diagonal the same scan is also timed with vote="diagonal" (ops.diag_vote instead of seq_scores +
    song_vote per window), the two votes' repetitions interleaved, and the found / planted counts are printed for both votes.

The repetitions of the two sides of (a) are interleaved; medians with min and max; the profiler is off."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralsampleid_amd import ops  # noqa: E402
from neuralsampleid_amd._lib import call  # noqa: E402
from neuralsampleid_amd.identify import SampleIndex  # noqa: E402

DEV = "cuda"
D = 128
THETA, MIN_SCORE = 0.6, 2.0
ROW_S = 0.512


def _st(v):
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def _fmt(t, unit="ms"):
    return f"{t[0]:9.3f} {unit} (min {t[1]:.3f}, max {t[2]:.3f})"


def _unit(g, n):
    """rows that correlate with their neighbours (overlapping segments), unit length"""
    f = torch.randn(n + 7, D, device=DEV, generator=g)
    x = sum(f[t:t + n] for t in range(8))
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def _plant(g, q, ref, a, b, n, rate, sigma=0.5):
    t = torch.arange(n, device=DEV)
    src = ref[b + torch.round(t * rate).long()]
    v = src + sigma * torch.randn(n, D, device=DEV, generator=g) / D ** 0.5
    q[a:a + n] = v / v.norm(dim=1, keepdim=True)


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def walk_case(g, P, L, strip, reps):
    p, st = (lambda t: t.data_ptr()), (lambda: torch.cuda.current_stream().cuda_stream)
    q = _unit(g, L)
    x = torch.cat([_unit(g, L) for _ in range(P)])
    for s in range(P):
        _plant(g, q, x[s * L:(s + 1) * L], (97 * s) % (L - 64), 40 + 11 * s, 48, (0.75, 1.0, 1.5)[s % 3])
    ones = np.full(P, L, np.int64)
    S, s_off, s_ld = ops.pair_sim(q, x, np.zeros(P, np.int64), ones, np.arange(P) * L, ones)
    top = 16
    i32 = torch.from_numpy(np.stack([s_ld, ones, ones]).astype(np.int32)).to(DEV)
    i64 = torch.from_numpy(np.stack([s_off, np.arange(P) * L])).to(DEV)
    occ = torch.empty((P, top, 4), device=DEV, dtype=torch.int32)
    occ_score = torch.empty((P, top), device=DEV)
    n_occ = torch.empty(P, device=DEV, dtype=torch.int32)
    row_h = torch.empty(P * L, device=DEV)
    row_j, row_org = (torch.empty(P * L, device=DEV, dtype=torch.int32) for _ in range(2))
    whole = lambda: call("nsid_local_align", p(S), p(i64[0]), p(i32[0]), p(i32[1]), p(i32[2]), P, L, L, THETA, MIN_SCORE, top, p(i64[1]),
                         p(row_h), p(row_j), p(row_org), p(occ), p(occ_score), p(n_occ), st())
    # the strips: per strip the tables of all pairs, uploaded before
    carry, carry_off = ops.align_carry(ones, DEV)
    c_off = torch.from_numpy(carry_off).to(DEV)
    s_rows = tuple(torch.empty(P * L, device=DEV, dtype=dt) for dt in (torch.float32, torch.int32, torch.int32, torch.int32))
    open_h = torch.empty(P, device=DEV)
    tables = []
    for lo in range(0, L, strip):
        n = min(strip, L - lo)
        t32 = torch.from_numpy(np.stack([np.full(P, n), np.full(P, lo), np.full(P, 1 if lo == 0 else 0)]).astype(np.int32)).to(DEV)
        t64 = torch.from_numpy(np.stack([s_off + lo * L, np.arange(P) * L + lo])).to(DEV)
        tables.append((n, t32, t64))

    def strips():
        for n, t32, t64 in tables:
            call("nsid_local_align_strip", p(S), p(t64[0]), p(i32[0]), p(t32[0]), p(i32[2]), p(t32[1]), p(t32[2]), P, n, L, THETA,
                 p(c_off), p(carry[0]), p(carry[1]), p(carry[2]), p(t64[1]), p(s_rows[0]), p(s_rows[1]), p(s_rows[2]), p(s_rows[3]),
                 p(open_h), st())

    n32 = torch.from_numpy(np.stack([ones, np.zeros(P, np.int64)]).astype(np.int32)).to(DEV)
    occ2, occ2_score, n_occ2 = torch.empty_like(occ), torch.empty_like(occ_score), torch.empty_like(n_occ)
    occs = lambda: call("nsid_align_occurrences", p(s_rows[0]), p(s_rows[1]), p(s_rows[2]), p(s_rows[3]), p(i64[1]), p(n32[0]), p(n32[1]),
                        P, L, MIN_SCORE, top, p(occ2), p(occ2_score), p(n_occ2), st())
    whole(), strips(), occs()
    torch.cuda.synchronize()
    assert torch.equal(occ2, occ) and torch.equal(occ2_score.view(torch.int32), occ_score.view(torch.int32)) and \
        torch.equal(n_occ2, n_occ), "align_occurrences and the one launch disagree on the occurrences"
    packed = torch.where(s_rows[2] >= 0, (s_rows[2] << 16) | s_rows[3], -1)
    assert torch.equal(s_rows[0].view(torch.int32), row_h.view(torch.int32)) and torch.equal(s_rows[1], row_j) and \
        torch.equal(packed, row_org), "the chained strips and the one launch disagree on the row results"
    t_whole, t_strips, t_occ = [], [], []
    for _ in range(reps):                                        # interleaved: A B C A B C ...
        t_whole.append(_event_ms(whole))
        t_strips.append(_event_ms(strips))
        t_occ.append(_event_ms(occs))
    a, b, c = _st(t_whole), _st(t_strips), _st(t_occ)
    ns = len(tables)
    carry_bytes = 2 * 2 * 12 * L * P * ns                         # two rows of 12-byte cells per pair and strip, read and written
    print(f"(a) the walk: {P} pairs of {L} x {L}, S {4.0 * P * L * L / 2 ** 30:.2f} GiB; occurrences per pair: min {int(n_occ.min())}, "
          f"max {int(n_occ.max())}")
    print(f"  nsid_local_align, one launch (walk + occurrences)   {_fmt(a)}   = {1e3 * a[0] / L:.3f} us per row")
    print(f"  nsid_local_align_strip, {ns} launches of {strip} rows       {_fmt(b)}   = {1e3 * b[0] / L:.3f} us per row")
    print(f"  nsid_align_occurrences, one launch, {P} runs of {L} rows  {_fmt(c)}")
    print(f"  strips + occurrences against the one launch: {b[0] + c[0] - a[0]:+.3f} ms = {1e3 * (b[0] + c[0] - a[0]) / ns:+.1f} us per strip")
    print(f"  strips alone against the one launch: {b[0] - a[0]:+.3f} ms = {1e3 * (b[0] - a[0]) / ns:+.1f} us per strip; carry traffic "
          f"{carry_bytes / 2 ** 20:.1f} MiB in all ({carry_bytes / ns / P / 1024:.0f} KiB per pair and strip)", flush=True)


def scan_case(g, a):
    rows = 1200 if a.quick else 14063
    n_songs, seg, dummy = (40, 40, 2000) if a.quick else (250, 40, 90000)
    idx = SampleIndex(None, device=DEV)
    idx.add_dummy(_unit(g, dummy))
    for s in range(n_songs):
        idx.add_rows(f"s{s}", _unit(g, seg))
    q = _unit(g, rows)
    ref = idx.fingerprints
    W = ops.VOTE_MAX_CAND // 20
    windows = -(-rows // W)
    # excerpts of 20 rows: at a window's second row (where the vote's sequence score sees them) and deep inside a window (where it
    # does not: such an excerpt is found only if its song is active for another reason)
    plants = []
    for n, w in enumerate(range(2, windows - 1, max(1, windows // 8))):
        plants.append((w * W + 1, 7 + 3 * n, 4, 20, (1.0, 0.75, 1.5)[n % 3], "start"))
        plants.append(((w + 1) * W + 100, 11 + 3 * n, 4, 20, (1.0, 0.75, 1.5)[n % 3], "inside"))
    for a0, song, b, n, rate, _ in plants:
        _plant(g, q, ref[song * seg:(song + 1) * seg], a0, b, n, rate)
    kw = dict(threshold=THETA, min_score=MIN_SCORE, row_hop_s=ROW_S, row_len_s=2 * ROW_S)
    votes = ("sequence", "diagonal") if a.vote == "diagonal" else ("sequence",)
    run = lambda vote: idx.scan(fp=q, vote=vote, **kw)
    occs = {v: run(v) for v in votes}
    torch.cuda.synchronize()
    t = {v: [] for v in votes}
    for _ in range(a.reps):                                      # interleaved: A B A B ...
        for v in votes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(v)
            torch.cuda.synchronize()
            t[v].append(1e3 * (time.perf_counter() - t0))
    print(f"(b) scan end to end: {rows} rows ({rows * ROW_S / 3600:.2f} h) against {n_songs} songs x {seg} rows + {dummy} dummy rows; "
          f"k_probe 20, n_songs 5, windows of {W} rows")
    for v in votes:
        sc = idx.scanner(vote=v, **kw)
        sc.push(q)
        sc.finish()
        m = _st(t[v])
        found = {"start": 0, "inside": 0}
        for a0, song, b, n, rate, kind in plants:
            want = (a0, a0 + n - 1)
            found[kind] += any(o.song == f"s{song}" and abs(o.q_rows[0] - want[0]) <= 1 and abs(o.q_rows[1] - want[1]) <= 1
                               for o in occs[v])
        print(f"  vote = {v}: {sc.stats['windows']} windows, {sc.stats['strips']} strips, {sc.stats['runs']} runs")
        print(f"  scan, total (host clock, results on the host)      {_fmt(m)}")
        print(f"  per window {m[0] / sc.stats['windows']:.3f} ms; {rows * ROW_S / (m[0] / 1e3):.0f} x real time")
        print(f"  {len(occs[v])} occurrences; planted at a window's second row: {found['start']} of {len(plants) // 2} found within one "
              f"row; planted 100 rows inside a window: {found['inside']} of {len(plants) // 2}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions, 4 pairs of 1024 x 1024, a 10-minute recording, a small index")
    ap.add_argument("--vote", choices=("sequence", "diagonal"), default="sequence",
                    help="diagonal: part (b) also with vote='diagonal', interleaved with the sequence vote")
    ap.add_argument("--no-walk", action="store_true", help="skip part (a)")
    a = ap.parse_args()
    if a.quick:
        a.reps = min(a.reps, 3)
    g = torch.Generator(device=DEV).manual_seed(0)
    with torch.no_grad():
        if not a.no_walk:
            walk_case(g, *((4, 1024) if a.quick else (32, 4096)), 204, a.reps)
        scan_case(g, a)


if __name__ == "__main__":
    main()
