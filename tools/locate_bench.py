"""Times the time-localised matching of neuralsampleid_amd.identify on synthetic rows at d = 128: (a) ops.pair_sim + ops.local_align for
one 480-row query against 1, 5 and 32 songs of 480 rows; (b) the evaluation-sized case, 76 queries x 5 songs as 380 pairs of one call;
(c) SampleIndex.locate end to end (windows, search, vote, align, the occurrences on the host).

    python tools/locate_bench.py [--reps 20] [--quick]

The yardstick is a torch composition of the same rule on the same device in the same process: one batched matrix product gives S, then
a Python loop over the rows with elementwise torch.where / comparisons over all pairs at once gives the row results (it stops there:
the occurrences are not formed). Its row results are checked equal to the kernel's on its own S before anything is timed. The
repetitions of the two sides are interleaved; the profiler is off.

Kernel times: device events around the launch alone (tables uploaded before), median of --reps after a warm-up; an event pair on an
idle GPU also sees the launch latency. "ops" times: host clock around the ops call, tables uploaded inside, synchronised after."""
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


def _fmt(t):
    return f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


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


def torch_rule(S, theta):
    """the yardstick's row walk: S (P, Lq, Lr) -> the row results (row_h, row_j, row_org), each (P, Lq)"""
    P, Lq, Lr = S.shape
    cols = torch.arange(Lr, device=S.device, dtype=torch.int32)
    zero = torch.zeros((P, Lr), device=S.device)
    none = torch.full((P, Lr), -1, device=S.device, dtype=torch.int32)
    pad_h = lambda h: torch.nn.functional.pad(h, (2, 0))
    pad_o = lambda o: torch.nn.functional.pad(o, (2, 0), value=-1)
    h1, o1, h2, o2 = pad_h(zero), pad_o(none), pad_h(zero), pad_o(none)
    row_h = torch.zeros((P, Lq), device=S.device)
    row_j = torch.full((P, Lq), -1, device=S.device, dtype=torch.int32)
    row_org = torch.full((P, Lq), -1, device=S.device, dtype=torch.int32)
    theta = torch.tensor(theta, device=S.device, dtype=torch.float32)
    for i in range(Lq):
        e = S[:, i] - theta
        best, frm = zero, none
        for hp, op in ((h1[:, 1:-1], o1[:, 1:-1]), (h1[:, :-2], o1[:, :-2]), (h2[:, 1:-1], o2[:, 1:-1])):
            take = hp > best
            best = torch.where(take, hp, best)
            frm = torch.where(take, op, frm)
        v = best + e
        pos = v > 0
        h = torch.where(pos, v, zero)
        o = torch.where(pos, torch.where(frm >= 0, frm, (i << 16) | cols), none)
        hv = torch.where(e > 0, h, -1.0)
        m = hv.max(dim=1).values
        j = torch.where(hv == m[:, None], cols, Lr).min(dim=1).values           # ties to the smallest j
        has = m > 0
        jc = j.clamp(max=Lr - 1).long()
        row_h[:, i] = torch.where(has, m, 0.0)
        row_j[:, i] = torch.where(has, j, -1)
        row_org[:, i] = torch.where(has, o.gather(1, jc[:, None])[:, 0], -1)
        h2, o2, h1, o1 = h1, o1, pad_h(h), pad_o(o)
    return row_h, row_j, row_org


def torch_yardstick(qb, xb, theta):
    """one batched matrix product gives S, the row loop the rest"""
    return torch_rule(torch.bmm(qb, xb.transpose(1, 2)), theta)


def kernel_launchers(q, x, P, Lq, Lr, top):
    """the two launches alone, their tables on the device: (pair_sim, local_align, S)"""
    dev = q.device
    q_len, x_len = np.full(P, Lq, np.int64), np.full(P, Lr, np.int64)
    q_start, x_start = np.arange(P) * Lq, np.arange(P) * Lr
    s_off, s_ld = np.arange(P) * Lq * Lr, x_len
    tiles = torch.from_numpy(ops.pair_sim_tiles(q_len, x_len)).to(dev)
    i32 = torch.from_numpy(np.stack([q_start, q_len, x_len, s_ld]).astype(np.int32)).to(dev)
    i64 = torch.from_numpy(np.stack([x_start, s_off, np.arange(P) * Lq])).to(dev)
    S = torch.empty(P * Lq * Lr, device=dev)
    occ = torch.empty((P, top, 4), device=dev, dtype=torch.int32)
    occ_score = torch.empty((P, top), device=dev)
    n_occ = torch.empty(P, device=dev, dtype=torch.int32)
    row_h = torch.empty(P * Lq, device=dev)
    row_j, row_org = (torch.empty(P * Lq, device=dev, dtype=torch.int32) for _ in range(2))
    p, st = (lambda t: t.data_ptr()), (lambda: torch.cuda.current_stream().cuda_stream)
    sim = lambda: call("nsid_pair_sim", p(q), D, q.shape[0], p(x), D, x.shape[0], D, p(i32[0]), p(i32[1]), p(i64[0]), p(i32[2]), p(i64[1]),
                       p(i32[3]), P, p(tiles), tiles.shape[0], p(S), S.numel(), st())
    align = lambda: call("nsid_local_align", p(S), p(i64[1]), p(i32[3]), p(i32[1]), p(i32[2]), P, Lq, Lr, THETA, MIN_SCORE, top, p(i64[2]),
                         p(row_h), p(row_j), p(row_org), p(occ), p(occ_score), p(n_occ), st())
    return sim, align, S


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def pairs_case(label, g, nq, ns, Lq, Lr, reps, top=16):
    """nq queries x ns songs each, as nq ns pairs of one call"""
    P = nq * ns
    q = torch.cat([_unit(g, Lq) for _ in range(nq)])
    x = torch.cat([_unit(g, Lr) for _ in range(P)])
    for p in range(P):                                           # one occurrence per pair, at rates 0.75, 1.0 and 1.5 in turn
        rate = (0.75, 1.0, 1.5)[p % 3]
        _plant(g, q[(p // ns) * Lq:(p // ns + 1) * Lq], x[p * Lr:(p + 1) * Lr], (20 + 13 * (p % ns)) % (Lq - 30), 30, 24, rate)
    q_len, x_len = [Lq] * P, [Lr] * P
    q_start, x_start = [(p // ns) * Lq for p in range(P)], [p * Lr for p in range(P)]
    sim, align, S_k = kernel_launchers(q, x, P, Lq, Lr, top)
    # the same pairs for the yardstick: (P, Lq, d) and (P, Lr, d)
    qb = q.view(nq, 1, Lq, D).expand(nq, ns, Lq, D).reshape(P, Lq, D).contiguous()
    xb = x.view(P, Lr, D)

    def ops_both():
        S, s_off, s_ld = ops.pair_sim(q, x, q_start, q_len, x_start, x_len)
        return ops.local_align(S, s_off, s_ld, q_len, x_len, THETA, MIN_SCORE, top)

    # agreement before anything is timed: the yardstick's rule on the kernel's own S gives the kernel's row results
    S, s_off, s_ld = ops.pair_sim(q, x, q_start, q_len, x_start, x_len)
    got = ops.local_align(S, s_off, s_ld, q_len, x_len, THETA, MIN_SCORE, top)
    S_t = torch.bmm(qb, xb.transpose(1, 2))
    assert float((S_t.reshape(-1) - S).abs().max()) < 1e-5, "the matrix product and pair_sim disagree"
    rh, rj, ro = torch_rule(S.view(P, Lq, Lr), THETA)
    assert torch.equal(rh.reshape(-1), got[3]) and torch.equal(rj.reshape(-1), got[4]) and torch.equal(ro.reshape(-1), got[5]), \
        "the torch rule and local_align disagree on the row results"
    n_occ = got[2].cpu().numpy()

    t_sim, t_align, t_ops, t_torch = [], [], [], []
    sim(), align(), ops_both(), torch_yardstick(qb, xb, THETA)
    torch.cuda.synchronize()
    for _ in range(reps):                                        # interleaved: A B A B ...
        t_sim.append(_event_ms(sim))
        t_align.append(_event_ms(align))
        t_ops.append(_host_ms(ops_both))
        t_torch.append(_host_ms(lambda: torch_yardstick(qb, xb, THETA)))
    sbytes = 4.0 * P * Lq * Lr
    print(f"{label}: {P} pairs of {Lq} x {Lr} rows, d {D}; S {sbytes / 2 ** 20:.1f} MiB written by pair_sim and read once by local_align; "
          f"{Lq} row barriers per pair (the latency floor of the walk); occurrences per pair: min {n_occ.min()}, max {n_occ.max()}")
    print(f"  pair_sim, launch alone (events)                 {_fmt(_st(t_sim))}")
    print(f"  local_align, launch alone (events)              {_fmt(_st(t_align))}   = {1e3 * np.median(t_align) / Lq:.3f} us per row")
    print(f"  ops.pair_sim + ops.local_align (host clock)     {_fmt(_st(t_ops))}")
    print(f"  torch yardstick: bmm + row loop (host clock)    {_fmt(_st(t_torch))}", flush=True)


def locate_case(g, a):
    n_songs, seg, Lq = (40, 120, 300) if a.quick else (250, 480, 480)
    idx = SampleIndex(None, device=DEV)
    idx.add_dummy(_unit(g, 2000 if a.quick else 20000))
    for s in range(n_songs):
        idx.add_rows(f"s{s}", _unit(g, seg))
    q = _unit(g, Lq)
    ref = idx.fingerprints
    plants = [(20, 7, 40, 24, 1.0), (120, 7, 10, 30, 0.75), (220, 19, 60, 20, 1.5)]
    for a0, song, b, n, rate in plants:
        _plant(g, q, ref[song * seg:(song + 1) * seg], a0, b, n, rate)
    run = lambda: idx.locate(fp=q, k_probe=20, n_songs=5, threshold=THETA, min_score=MIN_SCORE, row_hop_s=0.512, row_len_s=1.024)
    occs = run()
    t = [_host_ms(run) for _ in range(a.reps)]
    W = min(Lq, ops.VOTE_MAX_CAND // 20)
    print(f"(c) locate end to end: a {Lq}-row query against {n_songs} songs x {seg} rows + {idx.n_dummy} dummy rows, k_probe 20 "
          f"({-(-Lq // W)} windows of {W} rows), 5 candidates aligned")
    print(f"  locate, total (host clock, results on the host) {_fmt(_st(t))}")
    for o in occs:
        print(f"    {o.song}: score {o.score:.2f}, query rows {o.q_rows} = {o.q_time[0]:.1f}-{o.q_time[1]:.1f} s, song rows {o.r_rows} = "
              f"{o.r_time[0]:.1f}-{o.r_time[1]:.1f} s, stretch {o.stretch:.2f}")
    print(f"  planted: {[(f's{s}', (a0, a0 + n - 1), rate) for a0, s, b, n, rate in plants]}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions, shorter rows, a small index")
    a = ap.parse_args()
    if a.quick:
        a.reps = min(a.reps, 3)
    L = 96 if a.quick else 480
    g = torch.Generator(device=DEV).manual_seed(0)
    with torch.no_grad():
        for ns in (1, 5, 32):
            pairs_case(f"(a) one query, {ns} song{'s' if ns > 1 else ''}", g, 1, ns, L, L, a.reps)
        pairs_case("(b) evaluation-sized", g, 8 if a.quick else 76, 5, L, L, a.reps)
        locate_case(g, a)


if __name__ == "__main__":
    main()
