"""Fingerprint database files — the on-disk format the reference's retrieval/evaluation code reads.

Reference writer: test_fp.py:120-133 (`create_fp_db` / `create_ref_db` / `create_dummy_db`): for a database `fname`
  {fname}.mm            raw float32, C order, shape (n_segments, d)     (np.memmap mode 'w+')
  {fname}_shape.npy     np.save of the tuple (n_segments, d)            (loads as an int64 array of 2)
  {fname}_lookup.json   list of n_segments strings (song name per segment; queries: "<name>_<index>")
Reference reader: eval.py:154-196 (`load_memmap_data`: memmap 'r+', NaN -> 0 in place, optional extra rows).
Node-matrix dumps: test_fp.py:244-246 — one `{song_id}.npy` per song holding (num_segments, C, N) float32.

The fingerprints themselves come from `fingerprint.extract_fingerprints` (HIP kernels, eval-mode BN); `build_fp_db` streams
them straight into the memmap, and with several ranks every rank writes its contiguous row range of ONE shared file
(`shard_bounds`), so no gather is needed: the file is complete when all ranks have flushed."""
import json
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .fingerprint import shard_bounds


def write_fp_db(output_root_dir: str, fname: str, fp, lookup_table: Sequence[str]) -> Tuple[int, int]:
    """fp: (n, d) float32 array-like (numpy or a CPU/GPU torch tensor). Byte-identical to the reference writer."""
    fp = _to_numpy(fp)
    if fp.ndim != 2:
        raise ValueError("fingerprints must be (n_segments, d)")
    if len(lookup_table) != fp.shape[0]:
        raise ValueError(f"lookup table has {len(lookup_table)} entries for {fp.shape[0]} fingerprints")
    os.makedirs(output_root_dir, exist_ok=True)
    arr_shape = (int(fp.shape[0]), int(fp.shape[1]))
    arr = np.memmap(os.path.join(output_root_dir, f"{fname}.mm"), dtype="float32", mode="w+", shape=arr_shape)
    arr[:] = fp[:]
    arr.flush()
    del arr
    np.save(os.path.join(output_root_dir, f"{fname}_shape.npy"), arr_shape)
    with open(os.path.join(output_root_dir, f"{fname}_lookup.json"), "w") as f:
        json.dump(list(lookup_table), f)
    return arr_shape


def load_memmap_data(source_dir: str, fname: str, append_extra_length: Optional[int] = None, shape_only: bool = False,
                     display: bool = False):
    """Mirror of eval.py:154-196: returns (memmap 'r+', shape array); NaNs are zeroed in place like the reference does."""
    data_shape = np.load(os.path.join(source_dir, fname + "_shape.npy"))
    if shape_only:
        return data_shape
    if append_extra_length:
        data_shape[0] += append_extra_length
    data = np.memmap(os.path.join(source_dir, fname + ".mm"), dtype="float32", mode="r+",
                     shape=(int(data_shape[0]), int(data_shape[1])))
    data[np.isnan(data)] = 0.0
    if display:
        print(f"Load {data_shape[0]:,} items from {os.path.join(source_dir, fname + '.mm')}.")
    return data, data_shape


def load_lookup(source_dir: str, fname: str) -> List[str]:
    with open(os.path.join(source_dir, f"{fname}_lookup.json")) as f:
        return json.load(f)


def write_node_matrices(save_dir: str, matrices: Dict[str, np.ndarray]) -> None:
    """test_fp.py:244-246: one `{song_id}.npy` per song with the pre-projection node matrices (num_segments, C, N)."""
    os.makedirs(save_dir, exist_ok=True)
    for song_id, nm in matrices.items():
        np.save(os.path.join(save_dir, f"{song_id}.npy"), _to_numpy(nm))


def build_fp_db(model, songs: Iterable[Tuple[str, "object"]], output_root_dir: str, fname: str = "ref_db",
                query_style: bool = False, batch: int = 1024, rank: int = 0, world: int = 1,
                barrier=None) -> Tuple[int, int]:
    """songs: iterable of (name, specs) with specs (S, n_mels, n_frames) fp32 on the GPU (the log-mel segments of one
    audio file). Fingerprints are extracted on the HIP path and written in the reference's format.

    world > 1: every rank is handed the SAME `songs` sequence, extracts only its contiguous share of the segment rows and
    writes them into the shared memmap; rank 0 writes the shape and lookup files (`barrier`: torch.distributed's by
    default). Call a barrier before reading."""
    import torch
    from .fingerprint import embedding_dim, extract_fingerprints
    songs = list(songs)
    counts = [int(s.shape[0]) for _, s in songs]
    n = sum(counts)
    d = embedding_dim(model)
    lookup: List[str] = []
    for idx, ((nm, _), c) in enumerate(zip(songs, counts)):
        lookup.extend([f"{nm}_{idx}" if query_style else nm] * c)          # test_fp.py:110-115
    os.makedirs(output_root_dir, exist_ok=True)
    path = os.path.join(output_root_dir, f"{fname}.mm")
    if rank == 0:
        arr = np.memmap(path, dtype="float32", mode="w+", shape=(n, d))     # creates / sizes the file
        del arr
        np.save(os.path.join(output_root_dir, f"{fname}_shape.npy"), (n, d))
        with open(os.path.join(output_root_dir, f"{fname}_lookup.json"), "w") as f:
            json.dump(lookup, f)
    if world > 1:                                                           # the file exists before anyone maps it
        if barrier is None:
            import torch.distributed as dist
            barrier = dist.barrier
        barrier()
    lo, hi = shard_bounds(n, rank, world)
    arr = np.memmap(path, dtype="float32", mode="r+", shape=(n, d))
    row = 0
    for (_, specs), c in zip(songs, counts):
        a, b = max(lo, row), min(hi, row + c)
        if a < b:
            z = extract_fingerprints(model, specs[a - row:b - row], batch)
            arr[a:b] = z.detach().cpu().numpy()
        row += c
    arr.flush()
    del arr
    return n, d


class FpDbAppender:
    """the same three files written a block of rows at a time: `{fname}.mm` is a raw float32 array, so appending rows keeps
    the format; the shape and lookup files are written by close(). Byte-identical to write_fp_db on the same rows."""

    def __init__(self, output_root_dir: str, fname: str, d: int):
        os.makedirs(output_root_dir, exist_ok=True)
        self.dir, self.fname, self.d, self.n = output_root_dir, fname, int(d), 0
        self.lookup: List[str] = []
        self._f = open(os.path.join(output_root_dir, f"{fname}.mm"), "wb")

    def append(self, rows, names: Sequence[str]) -> None:
        rows = _to_numpy(rows)
        if rows.ndim != 2 or rows.shape[1] != self.d:
            raise ValueError(f"fingerprints must be (rows, {self.d})")
        if len(names) != rows.shape[0]:
            raise ValueError(f"{len(names)} lookup entries for {rows.shape[0]} fingerprints")
        rows.tofile(self._f)
        self.lookup.extend(names)
        self.n += int(rows.shape[0])

    def close(self) -> Tuple[int, int]:
        self._f.close()
        np.save(os.path.join(self.dir, f"{self.fname}_shape.npy"), (self.n, self.d))
        with open(os.path.join(self.dir, f"{self.fname}_lookup.json"), "w") as f:
            json.dump(self.lookup, f)
        return self.n, self.d


def build_fp_db_from_waves(model, front, songs: Iterable[Tuple[str, "object"]], output_root_dir: str, fname: str = "ref_db",
                           query_style: bool = False, batch: int = 1024, pack_samples: int = 1 << 26,
                           extract=None) -> Tuple[int, int, dict]:
    """The database of test_fp.py:92-216 (create_ref_db / create_query_db / create_dummy_db) straight from waveforms, without a
    launch, an unfolded tensor and a host copy per audio file (packs.py).

    songs: any iterable of (name, wave) with wave a mono fp32 1-D tensor on the CPU or the GPU, already at the front end's sample
    rate; it is consumed once, a pack at a time. front: a LogMelFrontEnd (SimCLR models) or a CQTFrontEnd (the ResNet-IBN
    baseline). Consecutive songs are grouped into packs of at most `pack_samples` samples (a longer song is a pack of its own); per
    pack there is one upload, one front-end launch, micro-batches of `batch` segments gathered into one reused buffer and handed
    to `extract`, and ONE device-to-host copy of the pack's fingerprints, whose rows are appended to `{fname}.mm`. Micro-batches do
    not cross packs. extract: `extract(specs, out)` -> fingerprints of specs written into out, e.g. a GraphedFingerprinter; by
    default extract_fingerprints on `model`.

    Songs at or below the front end's reflect-pad minimum, or shorter than one segment, are skipped (the reference's unfold raises
    and create_dummy_db skips the file). Lookup strings are `name`, or f"{name}_{idx}" with query_style, idx being the song's
    position in `songs`, skipped songs included (test_fp.py:110-115).

    The packed front end always uses the fused-FFT arithmetic (`front.batch`), whatever `stft` a LogMelFrontEnd was built with:
    a database and its queries must come from the same form.

    Returns (n, d, report): report["skipped"] = [(idx, name, reason)], report["packs"] = [{"songs": (first idx, last idx + 1),
    "rows": (first row, last row + 1)}] in file order."""
    import torch
    from .fingerprint import embedding_dim, extract_fingerprints
    from .packs import PackArena, WavePack, check_wave, plan_pack
    batch, pack_samples = int(batch), int(pack_samples)
    if batch < 1 or pack_samples < 1:
        raise ValueError("batch and pack_samples must be positive")
    d = embedding_dim(model)
    dev = next(model.parameters()).device
    if extract is None:
        def extract(specs, out):
            return extract_fingerprints(model, specs, batch, out)
    writer = FpDbAppender(output_root_dir, fname, d)
    report = {"skipped": [], "packs": []}
    arena = PackArena(dev)
    bufs = {}

    def flush(group, first_idx, end_idx):
        plan = plan_pack([w.numel() for _, _, w in group], front)
        for j, reason in plan.skipped:
            report["skipped"].append((group[j][0], group[j][1], reason))
        row0 = writer.n
        if plan.n_songs:
            pack = WavePack(plan, [group[j][2] for j in plan.index], dev, arena)
            n = plan.total_segs
            if "x" not in bufs:
                bufs["x"] = torch.empty((batch, plan.n_rows, plan.n_frames), device=dev, dtype=torch.float32)
            if "z" not in bufs or bufs["z"].shape[0] < n:
                bufs["z"] = torch.empty((n, d), device=dev, dtype=torch.float32)
            z = bufs["z"][:n]
            with torch.no_grad():
                for s0 in range(0, n, batch):
                    k = min(batch, n - s0)
                    extract(pack.segments(s0, k, bufs["x"]), z[s0:s0 + k])
            names = []
            for j, c in zip(plan.index, plan.segs):
                idx, nm, _ = group[j]
                names.extend([f"{nm}_{idx}" if query_style else nm] * int(c))
            writer.append(z.cpu().numpy(), names)                          # the pack's one device-to-host copy (blocking)
        report["packs"].append({"songs": (first_idx, end_idx), "rows": (row0, writer.n)})

    group, held, first = [], 0, 0
    idx = -1
    try:
        for idx, (nm, wave) in enumerate(songs):
            check_wave(wave)
            L = wave.numel()
            if group and held + L > pack_samples:
                flush(group, first, idx)
                group, held, first = [], 0, idx
            group.append((idx, nm, wave))
            held += L
        if group:
            flush(group, first, idx + 1)
    finally:
        n, d = writer.close()
    return n, d, report


def _to_numpy(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ node matrices (classifier re-rank)
def extract_node_matrices(model, specs, batch: int = 1024):
    """specs (S, n_mels, n_frames) fp32 on the GPU -> (S, C, N) fp32 pre-projection node matrices of the eval-mode encoder
    (the reference's model.encoder(p, return_pre_proj=True)[0], test_fp.py:233-236), on the HIP path"""
    import torch
    from . import functional, ops
    was_training = model.training
    model.eval()
    if functional.ACT_DTYPE == torch.bfloat16:
        ops.register_weight_shadows(model)
    try:
        pe = model.peak_extractor
        out = []
        with torch.no_grad():
            for lo in range(0, specs.shape[0], batch):
                x = specs[lo:lo + batch].contiguous()
                B, H, W = x.shape
                N = (H // pe.patch_bins) * (W // pe.patch_frames)
                rows, n_last, _ = model.encoder.forward_rows(pe.forward_rows(x), B, N, return_nodes=True)
                out.append(functional.from_rows(rows, B, n_last).float())
        if not out:
            return None
        return torch.cat(out, 0)
    finally:
        model.train(was_training)


def build_node_matrices(model, songs: Iterable[Tuple[str, "object"]], save_dir: str, batch: int = 1024) -> Dict[str, Tuple[int, ...]]:
    """test_fp.py:219-248 create_ref_nmatrix: `{save_dir}/{song}.npy` = (S, C, N) float32 per song (the eval_hr / eval_map
    ref_nmatrix directory). songs: iterable of (name, specs (S, n_mels, n_frames) on the GPU). Returns the shapes written."""
    os.makedirs(save_dir, exist_ok=True)
    shapes = {}
    for nm, specs in songs:
        m = extract_node_matrices(model, specs, batch)
        a = _to_numpy(m)
        np.save(os.path.join(save_dir, f"{nm}.npy"), a)
        shapes[nm] = a.shape
    return shapes


def build_query_node_matrices(model, songs: Iterable[Tuple[str, "object"]], save_path: str, batch: int = 1024) -> Dict[str, Tuple[int, ...]]:
    """test_fp.py:252-277 create_query_nmatrix: np.save of {song: (S, C, N) float32} to save_path (query_nmatrix.npy /
    query_full_nmatrix.npy; read back with np.load(..., allow_pickle=True).item())"""
    d = {nm: _to_numpy(extract_node_matrices(model, specs, batch)) for nm, specs in songs}
    parent = os.path.dirname(save_path)
    if parent:
        os.makedirs(parent, exist_ok=True)
    np.save(save_path, d)
    return {k: v.shape for k, v in d.items()}
