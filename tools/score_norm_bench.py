"""Times the cohort score normalisation of neuralsampleid_amd.identify on synthetic rows at d = 128: (a) ops.cohort_stats for a
scanner window (204 rows) and for resident rows (100 000) against a cohort of 4096 rows; (b) nsid_pair_sim against nsid_pair_sim_norm,
the launches alone, on the pairs cases of tools/locate_bench.py; (c) a scanner window with and without normalize=True.

    python tools/score_norm_bench.py [--reps 20] [--quick]

Device events around the launch (a, b) or a host clock around a synchronised call (c); a warm-up, then --reps repetitions, the two
sides of (b) and (c) alternated in one process; the profiler is off. cohort_stats is also given as a share of the fp32-MFMA bound
2 n M d / 155 TFLOP/s; its operand bytes (4 d (n + M) + 8 n) are printed beside it, so that which of the two bounds it can be read off."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from locate_bench import D, DEV, _event_ms, _fmt, _host_ms, _plant, _st, _unit  # noqa: E402
from neuralsampleid_amd import ops  # noqa: E402
from neuralsampleid_amd._lib import call  # noqa: E402
from neuralsampleid_amd.identify import SampleIndex  # noqa: E402

MFMA_F32_TFLOPS = 155.0          # fp32-input MFMA peak of one MI355X
HBM_TBPS = 8.0
THETA, MIN_SCORE = 7.0, 10.0     # sigmas: synthetic rows, nothing measured on real audio


def stats_case(g, n, M, reps):
    x, c = _unit(g, n), _unit(g, M)
    ops.cohort_stats(x, c)
    torch.cuda.synchronize()
    t = _st([_event_ms(lambda: ops.cohort_stats(x, c)) for _ in range(reps)])
    flop, nbytes = 2.0 * n * M * D, 4.0 * D * (n + M) + 8.0 * n
    t_mfma, t_mem = flop / (MFMA_F32_TFLOPS * 1e12) * 1e3, nbytes / (HBM_TBPS * 1e12) * 1e3
    print(f"(a) cohort_stats {n} x {M} x {D} (both launches, workspace allocated inside): {_fmt(t)}")
    print(f"    {flop / t[0] / 1e9:.1f} TFLOP/s = {100 * t_mfma / t[0]:.1f} % of the fp32-MFMA bound ({t_mfma:.4f} ms); operand bytes "
          f"{nbytes / 2 ** 20:.1f} MiB = {t_mem:.4f} ms at {HBM_TBPS:.0f} TB/s: the {'matrix rate' if t_mfma > t_mem else 'operand bytes'} "
          "bound it", flush=True)


def sim_launchers(q, x, P, Lq, Lr, norm):
    """nsid_pair_sim and nsid_pair_sim_norm alone, their tables on the device"""
    dev = q.device
    q_len, x_len = np.full(P, Lq, np.int64), np.full(P, Lr, np.int64)
    q_start, x_start = (np.arange(P) // (P // (q.shape[0] // Lq))) * Lq, np.arange(P) * Lr
    tiles = torch.from_numpy(ops.pair_sim_tiles(q_len, x_len)).to(dev)
    i32 = torch.from_numpy(np.stack([q_start, q_len, x_len, x_len]).astype(np.int32)).to(dev)
    i64 = torch.from_numpy(np.stack([x_start, np.arange(P) * Lq * Lr])).to(dev)
    S = torch.empty(P * Lq * Lr, device=dev)
    p, st = (lambda t: t.data_ptr()), (lambda: torch.cuda.current_stream().cuda_stream)
    args = lambda: (p(q), D, q.shape[0], p(x), D, x.shape[0], D, p(i32[0]), p(i32[1]), p(i64[0]), p(i32[2]), p(i64[1]), p(i32[3]), P,
                    p(tiles), tiles.shape[0], p(S), S.numel())
    raw = lambda: call("nsid_pair_sim", *args(), st())
    nrm = lambda: call("nsid_pair_sim_norm", *args(), *(p(t) for t in norm), st())
    return raw, nrm


def pairs_case(label, g, nq, ns, L, reps):
    P = nq * ns
    q = torch.cat([_unit(g, L) for _ in range(nq)])
    x = torch.cat([_unit(g, L) for _ in range(P)])
    cohort = _unit(g, 4096)
    norm = ops.cohort_stats(q, cohort) + ops.cohort_stats(x, cohort)
    raw, nrm = sim_launchers(q, x, P, L, L, norm)
    raw(), nrm()
    torch.cuda.synchronize()
    t_raw, t_nrm = [], []
    for _ in range(reps):                                        # alternated: A B A B ...
        t_raw.append(_event_ms(raw))
        t_nrm.append(_event_ms(nrm))
    a, b = _st(t_raw), _st(t_nrm)
    print(f"(b) {label}: {P} pairs of {L} x {L} rows, launches alone (events)")
    print(f"    pair_sim       {_fmt(a)}")
    print(f"    pair_sim_norm  {_fmt(b)}   = {b[0] / a[0]:.3f} x", flush=True)


def scanner_case(g, a):
    n_songs, seg, n_dummy, W = (40, 120, 2000, 100) if a.quick else (250, 480, 20000, 204)
    idx = SampleIndex(None, device=DEV)
    idx.add_dummy(_unit(g, n_dummy))
    for s in range(n_songs):
        idx.add_rows(f"s{s}", _unit(g, seg))
    idx.set_cohort()
    rec = _unit(g, 4 * W)
    for w, (song, b, rate) in enumerate(((7, 40, 1.0), (19, 60, 0.75), (3, 20, 1.5), (11, 10, 1.0))):
        _plant(g, rec[w * W:(w + 1) * W], idx.fingerprints[song * seg:(song + 1) * seg], 20, b, 30, rate)

    def run(normalize):
        kw = dict(threshold=THETA, min_score=MIN_SCORE) if normalize else dict(threshold=0.6, min_score=2.0)
        return idx.scan(fp=rec, k_probe=20, n_songs=5, window_rows=W, normalize=normalize, **kw)

    found = {n: len(run(n)) for n in (False, True)}
    t = {False: [], True: []}
    for _ in range(a.reps):
        for n in (False, True):
            t[n].append(_host_ms(lambda: run(n)) / 4)
    print(f"(c) scanner: 4 windows of {W} rows against {n_songs} songs x {seg} rows + {idx.n_dummy} dummy rows, cohort {idx._cohort.shape[0]}, "
          f"5 voted songs a window; per window (host clock around scan() / 4, results on the host, resident statistics cached)")
    print(f"    raw cells        {_fmt(_st(t[False]))}   {found[False]} occurrences")
    print(f"    normalize=True   {_fmt(_st(t[True]))}   {found[True]} occurrences   = {np.median(t[True]) / np.median(t[False]):.3f} x",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions, shorter rows, a small index")
    a = ap.parse_args()
    if a.quick:
        a.reps = min(a.reps, 3)
    g = torch.Generator(device=DEV).manual_seed(0)
    with torch.no_grad():
        stats_case(g, 204, 4096, a.reps)
        stats_case(g, 10000 if a.quick else 100000, 4096, a.reps)
        L = 96 if a.quick else 480
        for ns in (1, 5, 32):
            pairs_case(f"one query, {ns} song{'s' if ns > 1 else ''}", g, 1, ns, L, a.reps)
        pairs_case("evaluation-sized", g, 8 if a.quick else 76, 5, L, a.reps)
        scanner_case(g, a)


if __name__ == "__main__":
    main()
