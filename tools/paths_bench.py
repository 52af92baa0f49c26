"""Times SampleIndex.paths on the occurrences of tools/locate_bench.py's case: synthetic rows at d = 128, one 480-row query against songs
of 480 rows, an excerpt of every song planted in the query at rates 0.75, 1.0 and 1.5 in turn.

    python tools/paths_bench.py [--reps 20] [--quick]

Per number of songs (1, 5, 32): SampleIndex.align (the call that produces the occurrences: one pair_sim and one local_align over the
whole 480 x 480 matrices) next to SampleIndex.paths on its occurrences (one pair_sim and one align_paths over the occurrences' boxes,
one copy to the host, the statistics on the host), both on the host clock with the results on the host, interleaved; then the
align_paths launch alone (device events, tables uploaded before) and the time per path cell. The paths are checked before anything is
timed: every one starts and ends at its occurrence's corners, and paths() itself refuses a last H that differs from the score in any
bit. The profiler is off."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from locate_bench import D, DEV, MIN_SCORE, THETA, _event_ms, _fmt, _host_ms, _plant, _st, _unit  # noqa: E402
from neuralsampleid_amd import ops  # noqa: E402
from neuralsampleid_amd._lib import call  # noqa: E402
from neuralsampleid_amd.identify import SampleIndex  # noqa: E402


def paths_launcher(idx, q, occs):
    """the align_paths launch alone on the boxes of `occs`, S and the tables on the device"""
    first = {n: idx._song_rows[idx.code(n)][0] for n in {o.song for o in occs}}
    b = np.asarray([(o.q_rows[0], o.q_rows[1] - o.q_rows[0] + 1, first[o.song] + o.r_rows[0], o.r_rows[1] - o.r_rows[0] + 1, o.r_rows[0])
                    for o in occs], dtype=np.int64)
    S, s_off, s_ld = ops.pair_sim(q, idx.fingerprints, b[:, 0], b[:, 1], b[:, 2], b[:, 3])
    slots = np.minimum(b[:, 1], b[:, 3])
    dsize = b[:, 1] * ((b[:, 3] + 3) // 4)
    dev = q.device
    i32 = torch.from_numpy(np.stack([s_ld, b[:, 1], b[:, 3], b[:, 0], b[:, 4]]).astype(np.int32)).to(dev)
    i64 = torch.from_numpy(np.stack([s_off, np.cumsum(slots) - slots, np.cumsum(dsize) - dsize])).to(dev)
    n = int(slots.sum())
    path_len = torch.empty(len(occs), device=dev, dtype=torch.int32)
    end_h = torch.empty(len(occs), device=dev)
    path_i, path_j = (torch.empty(n, device=dev, dtype=torch.int32) for _ in range(2))
    path_s = torch.empty(n, device=dev)
    dirs = torch.empty(int(dsize.sum()), device=dev, dtype=torch.uint8)
    p, st = (lambda t: t.data_ptr()), (lambda: torch.cuda.current_stream().cuda_stream)
    launch = lambda: call("nsid_align_paths", p(S), p(i64[0]), p(i32[0]), p(i32[1]), p(i32[2]), p(i32[3]), p(i32[4]), len(occs),
                          int(b[:, 3].max()), THETA, p(i64[1]), p(i64[2]), p(dirs), p(path_len), p(path_i), p(path_j), p(path_s), p(end_h),
                          st())
    return launch, path_len, int((b[:, 1] * b[:, 3]).sum())


def songs_case(g, ns, L, reps):
    idx = SampleIndex(None, device=DEV)
    for s in range(ns):
        idx.add_rows(f"s{s}", _unit(g, L))
    names = [f"s{s}" for s in range(ns)]
    q = _unit(g, L)
    ref = idx.fingerprints
    n = min(24, max(4, (L - 40) // max(ns, 1)))                     # the excerpts follow one another in the query
    for s in range(ns):
        _plant(g, q, ref[s * L:(s + 1) * L], 10 + s * n, 30, n, (0.75, 1.0, 1.5)[s % 3])
    align = lambda: idx.align(q, names, threshold=THETA, min_score=MIN_SCORE, row_hop_s=0.512, row_len_s=1.024)
    occs = [o for per_song in align() for o in per_song]
    assert occs, "the planted excerpts were not found"
    paths = lambda: idx.paths(q, occs, THETA, row_hop_s=0.512, row_len_s=1.024)
    got = paths()
    for pth, o in zip(got, occs):
        assert (pth.q_rows[0], pth.q_rows[-1]) == o.q_rows and (pth.r_rows[0], pth.r_rows[-1]) == o.r_rows
    cells = sum(pth.q_rows.size for pth in got)
    launch, path_len, box_cells = paths_launcher(idx, q, occs)
    launch()
    torch.cuda.synchronize()
    assert int(path_len.sum()) == cells
    t_align, t_paths, t_launch = [], [], []
    for _ in range(reps):                                        # interleaved
        t_align.append(_host_ms(align))
        t_paths.append(_host_ms(paths))
        t_launch.append(_event_ms(launch))
    slopes = ", ".join(f"{pth.slope:.3f}" for pth in got[:6] if pth.slope is not None)
    print(f"{ns} song{'s' if ns > 1 else ''} x {L} rows, a {L}-row query: {len(occs)} occurrences, {box_cells} box cells "
          f"({100.0 * box_cells / (ns * L * L):.2f} % of the matrices), {cells} path cells; slopes {slopes}{' ...' if len(got) > 6 else ''}")
    print(f"  SampleIndex.align (host clock, results on the host)   {_fmt(_st(t_align))}")
    print(f"  SampleIndex.paths (host clock, results on the host)   {_fmt(_st(t_paths))}   = "
          f"{1e3 * np.median(t_paths) / cells:.2f} us per path cell")
    print(f"  align_paths, launch alone (events)                    {_fmt(_st(t_launch))}   = "
          f"{1e3 * np.median(t_launch) / cells:.2f} us per path cell", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions, shorter rows")
    a = ap.parse_args()
    if a.quick:
        a.reps = min(a.reps, 3)
    L = 160 if a.quick else 480
    g = torch.Generator(device=DEV).manual_seed(0)
    with torch.no_grad():
        for ns in (1, 5, 32):
            songs_case(g, ns, L, a.reps)


if __name__ == "__main__":
    main()
