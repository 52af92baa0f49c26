"""Times the alignment against songs past 4096 rows (ops.local_align_panels, SampleIndex(long_songs=True)) on synthetic rows at d = 128.

    python tools/long_song_bench.py [--reps 9] [--pairs 8] [--quick]

(a) The walk in panels against the strip walk. `pairs` pairs of 204 x 4096 (the scanner's window at k_probe = 20 against the longest
    song the strip kernel takes) through nsid_local_align_strip and through nsid_local_align_panels at panel_cols = 4096 (one panel)
    and 1024 (four panels), the same S, every launch fresh. The outputs are checked equal before anything is timed. For information:
    the default path does not use the panels kernel at this shape.
(b) The panels entry at 204 x 8192, 204 x 16384 and 4096 x 16384 (panel_cols = 4096: 2, 4 and 4 panels), one workgroup per pair.
(c) A scanner window with one long song active: scanner(songs=[a song of 16384 rows]) over a recording of 10 windows of 204 rows, host
    clock per window (pair_sim, the panels launch, the round trip of open_h), beside the same with a song of 4096 rows in a default
    index (the strip launch).
(d) nsid_align_occurrences_span on one run of 2^20 rows at span 32766 (a song of 16384 rows), every row in a group of 64 rows, beside
    nsid_align_occurrences (its window is 8190 rows) on the same rows.

Device events around the launches alone in (a), (b) and (d), tables on the device before; the repetitions of the sides of a comparison
are interleaved; medians with min and max; the profiler is off."""
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


def _st(v):
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def _fmt(t, unit="ms"):
    return f"{t[0]:9.3f} {unit} (min {t[1]:.3f}, max {t[2]:.3f})"


def _unit(g, n):
    """rows that correlate with their neighbours (overlapping segments), unit length"""
    f = torch.randn(n + 7, D, device=DEV, generator=g)
    x = sum(f[t:t + n] for t in range(8))
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


class Walk:
    """P fresh pairs of Lq x Lr over one S; strip() and panels(panel_cols) are one launch each, with their own outputs"""

    def __init__(self, g, P, Lq, Lr):
        self.P, self.Lq, self.Lr = P, Lq, Lr
        q = _unit(g, Lq)
        x = torch.cat([_unit(g, Lr) for _ in range(P)])
        for s in range(P):                                          # an excerpt per pair, across column 4096 where the song has one
            n = min(48, Lq)
            b = min(4096, Lr - n) - 20 - 3 * s
            v = x[s * Lr + b: s * Lr + b + n] + 0.5 * torch.randn(n, D, device=DEV, generator=g) / D ** 0.5
            q[(7 * s) % (Lq - n + 1):][:n] = v / v.norm(dim=1, keepdim=True)
        ql, xl = np.full(P, Lq, np.int64), np.full(P, Lr, np.int64)
        self.S, s_off, s_ld = ops.pair_sim(q, x, np.zeros(P, np.int64), ql, np.arange(P) * Lr, xl, long_songs=True)
        self.i32 = torch.from_numpy(np.stack([s_ld, ql, xl, np.zeros(P), np.ones(P)]).astype(np.int32)).to(DEV)   # .., row_base, fresh
        hsize = 2 * (Lq + 2)
        self.i64 = torch.from_numpy(np.stack([s_off, np.arange(P) * 2 * Lr, np.arange(P) * Lq, np.arange(P) * hsize])).to(DEV)
        self.halo = (torch.empty(P * hsize, device=DEV),) + tuple(torch.empty(P * hsize, device=DEV, dtype=torch.int32) for _ in range(2))
        self.out = {}

    def _outputs(self, key):
        if key not in self.out:
            P, Lq, Lr = self.P, self.Lq, self.Lr
            ints = lambda n: torch.empty(n, device=DEV, dtype=torch.int32)
            self.out[key] = ((torch.empty(2 * P * Lr, device=DEV), ints(2 * P * Lr), ints(2 * P * Lr)),
                             (torch.empty(P * Lq, device=DEV), ints(P * Lq), ints(P * Lq), ints(P * Lq)), torch.empty(P, device=DEV))
        return self.out[key]

    def strip(self):
        p, i32, i64 = (lambda t: t.data_ptr()), self.i32, self.i64
        carry, rows, open_h = self._outputs("strip")
        call("nsid_local_align_strip", p(self.S), p(i64[0]), p(i32[0]), p(i32[1]), p(i32[2]), p(i32[3]), p(i32[4]), self.P, self.Lq,
             self.Lr, THETA, p(i64[1]), p(carry[0]), p(carry[1]), p(carry[2]), p(i64[2]), p(rows[0]), p(rows[1]), p(rows[2]), p(rows[3]),
             p(open_h), torch.cuda.current_stream().cuda_stream)

    def panels(self, panel_cols):
        p, i32, i64, halo = (lambda t: t.data_ptr()), self.i32, self.i64, self.halo
        carry, rows, open_h = self._outputs(panel_cols)
        call("nsid_local_align_panels", p(self.S), p(i64[0]), p(i32[0]), p(i32[1]), p(i32[2]), p(i32[3]), p(i32[4]), self.P, self.Lq,
             self.Lr, panel_cols, THETA, p(i64[1]), p(carry[0]), p(carry[1]), p(carry[2]), p(i64[3]), p(halo[0]), p(halo[1]), p(halo[2]),
             p(i64[2]), p(rows[0]), p(rows[1]), p(rows[2]), p(rows[3]), p(open_h), torch.cuda.current_stream().cuda_stream)

    def same(self, a, b):
        flat = lambda o: [t.view(torch.int32) for t in o[0] + o[1]] + [o[2].view(torch.int32)]
        return all(torch.equal(u, v) for u, v in zip(flat(self.out[a]), flat(self.out[b])))


def _line(name, t, Lq, Lr, P):
    print(f"  {name:58s}{_fmt(t)}   = {1e3 * t[0] / Lq:7.3f} us per row, {1e6 * t[0] / (Lq * Lr * P):6.3f} ns per cell", flush=True)


def walk_cases(g, a):
    P = a.pairs
    w = Walk(g, P, 204, 4096)
    w.strip(), w.panels(4096), w.panels(1024)
    torch.cuda.synchronize()
    assert w.same("strip", 4096) and w.same("strip", 1024), "the panels and the strip kernel disagree"
    t = ([], [], [])
    for _ in range(a.reps):                                          # interleaved: A B C A B C ...
        t[0].append(_event_ms(w.strip))
        t[1].append(_event_ms(lambda: w.panels(4096)))
        t[2].append(_event_ms(lambda: w.panels(1024)))
    print(f"(a) {P} pairs of 204 x 4096, one launch, fresh")
    _line("nsid_local_align_strip", _st(t[0]), 204, 4096, P)
    _line("nsid_local_align_panels, panel_cols 4096 (1 panel)", _st(t[1]), 204, 4096, P)
    _line("nsid_local_align_panels, panel_cols 1024 (4 panels)", _st(t[2]), 204, 4096, P)
    print(f"  panels (1 panel) / strip = {np.median(t[1]) / np.median(t[0]):.3f}", flush=True)
    del w
    print(f"(b) {P} pairs, nsid_local_align_panels at panel_cols 4096, one launch, fresh")
    for Lq, Lr in ((204, 8192), (204, 16384), (4096, 16384)):
        if a.quick and Lq > 204:
            continue
        w = Walk(g, P, Lq, Lr)
        w.panels(4096)
        torch.cuda.synchronize()
        _line(f"{Lq} x {Lr} ({-(-Lr // 4096)} panels), S {4.0 * P * Lq * Lr / 2 ** 30:.2f} GiB",
              _st([_event_ms(lambda: w.panels(4096)) for _ in range(a.reps)]), Lq, Lr, P)
        del w


def window_case(g, a):
    W = ops.VOTE_MAX_CAND // 20
    rec = _unit(g, 10 * W)
    kw = dict(threshold=THETA, min_score=MIN_SCORE)
    sides = []
    for rows, long_songs in ((16384, True), (4096, False)):
        idx = SampleIndex(None, device=DEV, long_songs=long_songs)
        idx.add_dummy(_unit(g, 2000 if a.quick else 90000))
        for s in range(40 if a.quick else 250):
            idx.add_rows(f"s{s}", _unit(g, 40))
        idx.add_rows("song", _unit(g, rows))
        sides.append((rows, idx))

    def run(idx):
        sc = idx.scanner(songs=["song"], **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.push(rec)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / 10
    for _, idx in sides:
        run(idx)
    t = [[], []]
    for _ in range(a.reps):
        for n, (_, idx) in enumerate(sides):
            t[n].append(run(idx))
    print(f"(c) a scanner window of {W} rows with one song active (songs=[...], nothing voted), host clock per window over 10 windows")
    for n, (rows, idx) in enumerate(sides):
        print(f"  a song of {rows:5d} rows, long_songs={idx.long_songs!s:5s}                          {_fmt(_st(t[n]))}", flush=True)


def occurrences_case(a):
    n = 1 << (16 if a.quick else 20)
    rng = np.random.default_rng(0)
    i = np.arange(n)
    rows = [torch.from_numpy(v).to(DEV) for v in (rng.random(n, dtype=np.float32) + 2.0, (i % 64).astype(np.int32),
                                                   (i // 64 * 64).astype(np.int32), np.full(n, 5, np.int32))]
    p = lambda t: t.data_ptr()
    i32 = torch.tensor([n, 0, 32766], device=DEV, dtype=torch.int32)
    off = torch.zeros(1, device=DEV, dtype=torch.int64)
    outs = [(torch.empty((1, 16, 4), device=DEV, dtype=torch.int32), torch.empty((1, 16), device=DEV), torch.empty(1, device=DEV, dtype=torch.int32))
            for _ in range(2)]
    st = lambda: torch.cuda.current_stream().cuda_stream
    span = lambda: call("nsid_align_occurrences_span", p(rows[0]), p(rows[1]), p(rows[2]), p(rows[3]), p(off), p(i32[0:]), p(i32[1:]),
                        p(i32[2:]), 1, n, MIN_SCORE, 16, p(outs[0][0]), p(outs[0][1]), p(outs[0][2]), st())
    plain = lambda: call("nsid_align_occurrences", p(rows[0]), p(rows[1]), p(rows[2]), p(rows[3]), p(off), p(i32[0:]), p(i32[1:]), 1, n,
                         MIN_SCORE, 16, p(outs[1][0]), p(outs[1][1]), p(outs[1][2]), st())
    span(), plain()
    torch.cuda.synchronize()
    assert int(outs[0][2]) == n // 64 and all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(*outs))
    t = ([], [])
    for _ in range(a.reps):
        t[0].append(_event_ms(span))
        t[1].append(_event_ms(plain))
    print(f"(d) one run of {n} rows in groups of 64 rows ({n // 64} occurrences), one workgroup")
    print(f"  nsid_align_occurrences_span, span 32766                   {_fmt(_st(t[0]))}")
    print(f"  nsid_align_occurrences (window 8190)                      {_fmt(_st(t[1]))}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions, no 4096 x 16384 walk, a small index, a run of 2^16 rows")
    a = ap.parse_args()
    if a.quick:
        a.reps = min(a.reps, 3)
    g = torch.Generator(device=DEV).manual_seed(0)
    with torch.no_grad():
        walk_cases(g, a)
        window_case(g, a)
        occurrences_case(a)


if __name__ == "__main__":
    main()
