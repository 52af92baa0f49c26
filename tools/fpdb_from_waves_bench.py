#!/usr/bin/env python3
"""Database build from waveforms: the per-file path against the packed one (fpdb.build_fp_db_from_waves). Prints one JSON line.

    python tools/fpdb_from_waves_bench.py [--songs 2000] [--reps 3] [--batch 1024]

Workload: `--songs` synthetic noise songs of 30 s at 16 kHz on the HOST (fp32; at most 256 distinct waveforms, handed out in turn),
51 segments each, the 't' encoder in bf16 storage, one MI355X. Every path starts from the host waveforms and ends with the
database files on disk, so each includes its uploads, its device-to-host copies and the file writes:
  per_file_gemm / per_file_fft   the path a caller had before: per song `front(wave.to(device))` (one front-end pass and one segment
                                 gather per file), extract_fingerprints on that file's segments, a blocking host copy per file;
                                 with the default stft="gemm" front end and with stft="fft" (the arithmetic the packed path uses)
  packed_eager                   build_fp_db_from_waves, extract_fingerprints per micro-batch
  packed_graphed                 build_fp_db_from_waves with a GraphedFingerprinter
Method: a host clock around each whole build, ending in a device synchronise; one warm-up of every path, then the paths take turns
repetition by repetition (the box is shared: a drift hits all of them); median, minimum and maximum are reported, and a speed-up
counts only if it exceeds the spread. `front_end_share_of_pack`: device-event time of the ragged front-end launch over one pack of
the default size (warm, median of 5), over the packed_graphed wall time per pack. Peak device memory is torch's allocator peak over a
packed build (model, pack buffers, micro-batch activations)."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralsampleid_amd import fpdb, functional as F_, ops  # noqa: E402
from neuralsampleid_amd.fingerprint import GraphedFingerprinter, extract_fingerprints  # noqa: E402
from neuralsampleid_amd.frontend import LogMelFrontEnd  # noqa: E402
from neuralsampleid_amd.packs import WavePack, plan_pack  # noqa: E402

FCFG = {"fs": 16000, "n_fft": 1024, "win_len": 1024, "hop_len": 512, "n_mels": 64, "n_frames": 128, "overlap": 0.875}
CFG = {"arch": "grafp", "n_mels": 64, "n_frames": 128, "patch_bins": 4, "patch_frames": 8, "n_filters": 8,
       "bsz_train": 256, "tau": 0.05, "lr": 8.0e-5, "d": 128, "h": 1024, "u": 32}
L_SONG = 30 * 16000
DISTINCT = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--pack-samples", type=int, default=1 << 26)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/fpdb_from_waves_bench.py measures on an MI355X; there is no CPU path")
    from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
    from neuralsampleid_amd.simclr.simclr import SimCLR
    dev = torch.device("cuda")
    ops.set_gemm_precision("bf16")
    F_.set_activation_dtype("bf16")
    torch.manual_seed(42)
    model = SimCLR(CFG, encoder=GraphEncoder(cfg=CFG, in_channels=CFG["n_filters"], k=3, size="t")).to(dev).eval()
    gemm, fft = LogMelFrontEnd(FCFG, dev), LogMelFrontEnd(FCFG, dev, stft="fft")
    g = torch.Generator().manual_seed(7)
    distinct = [0.1 * torch.randn(L_SONG, generator=g) for _ in range(min(args.songs, DISTINCT))]

    def songs():
        return ((f"s{i}", distinct[i % len(distinct)]) for i in range(args.songs))

    tmp = tempfile.mkdtemp(prefix="fpdb_bench_")

    def per_file(front, tag):
        w = fpdb.FpDbAppender(tmp, tag, 128)
        for nm, wave in songs():
            segs = front(wave.to(dev))
            if segs.shape[0]:
                w.append(extract_fingerprints(model, segs, args.batch), [nm] * segs.shape[0])
        return w.close()[0]

    graphed = GraphedFingerprinter(model, micro_batch=args.batch)
    paths = {
        "per_file_gemm": lambda: per_file(gemm, "a_gemm"),
        "per_file_fft": lambda: per_file(fft, "a_fft"),
        "packed_eager": lambda: fpdb.build_fp_db_from_waves(model, gemm, songs(), tmp, "b", batch=args.batch,
                                                            pack_samples=args.pack_samples)[0],
        "packed_graphed": lambda: fpdb.build_fp_db_from_waves(model, gemm, songs(), tmp, "c", batch=args.batch,
                                                              pack_samples=args.pack_samples, extract=graphed)[0],
    }

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, n

    clips = {k: timed(fn)[1] for k, fn in paths.items()}                     # warm-up of every path
    assert len(set(clips.values())) == 1, clips
    n_clips = clips["packed_eager"]
    ts = {k: [] for k in paths}
    for r in range(args.reps):
        for k, fn in paths.items():
            ts[k].append(timed(fn)[0])
            print(f"repetition {r} {k}: {ts[k][-1]:.3f} s", file=sys.stderr, flush=True)
    res = {"tool": "fpdb_from_waves_bench", "songs": args.songs, "clips": n_clips, "reps": args.reps, "batch": args.batch,
           "pack_samples": args.pack_samples, "unit": "seconds per build, host clock, interleaved repetitions"}
    for k, v in ts.items():
        med = statistics.median(v)
        res[k] = {"median_s": round(med, 3), "min_s": round(min(v), 3), "max_s": round(max(v), 3),
                  "songs_per_s": round(args.songs / med, 1), "clips_per_s": round(n_clips / med, 1)}
    for k in ("packed_eager", "packed_graphed"):
        for base in ("per_file_gemm", "per_file_fft"):
            res[k][f"speedup_over_{base}"] = round(res[base]["median_s"] / res[k]["median_s"], 2)
            # beyond the spread: the slowest packed repetition against the fastest per-file one
            res[k][f"worst_case_speedup_over_{base}"] = round(res[base]["min_s"] / res[k]["max_s"], 2)

    # the files of the per-file fft path and of the packed path hold the same fingerprints up to the micro-batch composition
    a, _ = fpdb.load_memmap_data(tmp, "a_fft")
    b, _ = fpdb.load_memmap_data(tmp, "b")
    c, _ = fpdb.load_memmap_data(tmp, "c")
    res["max_abs_diff_packed_eager_vs_per_file_fft"] = float(np.abs(np.asarray(a) - np.asarray(b)).max())
    res["max_abs_diff_packed_graphed_vs_packed_eager"] = float(np.abs(np.asarray(c) - np.asarray(b)).max())
    assert fpdb.load_lookup(tmp, "a_fft") == fpdb.load_lookup(tmp, "b") == fpdb.load_lookup(tmp, "c")

    # one pack of the default size: the front end's share, the buffers, the allocator's peak
    per_pack = max(1, min(args.songs, args.pack_samples // L_SONG))
    plan = plan_pack([L_SONG] * per_pack, gemm)
    pack = WavePack(plan, [distinct[i % len(distinct)] for i in range(per_pack)], dev)
    torch.cuda.synchronize()
    ev = []
    for _ in range(6):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ops.logmel_fft_ragged(pack, gemm.n_fft, gemm.window, gemm.twiddle, gemm.fb, gemm.band, pack.spec)
        e.record()
        e.synchronize()
        ev.append(s.elapsed_time(e))
    front_ms = statistics.median(ev[1:])
    n_packs = -(-args.songs // per_pack)
    pack_ms = 1e3 * res["packed_graphed"]["median_s"] / n_packs
    res["pack"] = {"songs": per_pack, "segments": plan.total_segs, "front_end_ms": round(front_ms, 3),
                   "wall_ms_per_pack_graphed": round(pack_ms, 1), "front_end_share_of_pack": round(front_ms / pack_ms, 4),
                   "waveform_and_table_bytes": 4 * plan.total_samples + 8 * (4 * plan.n_songs + plan.total_segs),
                   "spectrogram_bytes": 4 * plan.n_rows * plan.ld, "micro_batch_bytes": 4 * args.batch * 64 * 128,
                   "fingerprint_bytes": 4 * plan.total_segs * 128}
    del pack
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    paths["packed_graphed"]()
    torch.cuda.synchronize()
    res["pack"]["peak_device_bytes_allocated_during_build"] = int(torch.cuda.max_memory_allocated())
    res["pack"]["device_bytes_allocated_before_build"] = int(base)
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
