"""Packs: many songs of different lengths through the front end in ONE launch (include/nsid.h nsid_logmel_fft_ragged /
nsid_cqt_ragged), and their segments one micro-batch at a time (nsid_unfold_segments_ragged) — the database build of the
reference's test_fp.py:92-216 (create_query_db / create_ref_db / create_dummy_db) without a launch, an unfolded tensor and a host
copy per audio file. fpdb.build_fp_db_from_waves is the driver.

    plan = plan_pack([w.numel() for w in waves], front)      # host only: every table, every bound
    pack = WavePack(plan, [waves[i] for i in plan.index], "cuda")    # one upload, one front-end launch
    x = pack.segments(s0, nseg, buf)                         # (nseg, rows, n_frames) of the pack's segment list

The kernels take their per-song tables from device memory and cannot check them, so everything that would otherwise become an
out-of-bounds access is checked here, on the host, before anything is uploaded: `PackPlan.validate` re-derives every table from
the lengths, and the ops wrappers take their tables from a WavePack (built from a validated plan) only.

A song's spectrogram columns, and therefore its segments, are bit-equal to `front.batch(wave[None])[0]` — the fused-FFT
arithmetic for the log-mel front end, whatever `stft` the front end uses for single waveforms."""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import DEFINES

MAX_PACK_SAMPLES = 1 << 30           # the kernels index a song's samples with ints, the entries refuse more
MAX_CQT_SONG = 1 << 28               # nsid_cqt's limit for one clip
LOGMEL_RUN, CQT_TILE = DEFINES["NSID_LOGMEL_RUN"], DEFINES["NSID_CQT_TILE"]      # frames per work item (include/nsid.h)
TABLE_COLS = DEFINES["NSID_PACK_COLS"]                 # {first sample, samples, first column, items before}


def front_kind(front) -> str:
    from .frontend import CQTFrontEnd, LogMelFrontEnd
    if isinstance(front, LogMelFrontEnd):
        return "logmel"
    if isinstance(front, CQTFrontEnd):
        return "cqt"
    raise TypeError(f"plan_pack takes a LogMelFrontEnd or a CQTFrontEnd, got {type(front).__name__}")


def _tables(lengths: np.ndarray, hop: int, n_frames: int, step: int, item: int, gap: int):
    """every table of a pack from the song lengths alone (int64 arrays; the plain loops of tests/test_packs_cpu.py restate it)"""
    n = lengths.size
    frames = 1 + lengths // hop
    segs = np.where(frames >= n_frames, (frames - n_frames) // step + 1, 0)
    offsets = np.zeros(n, np.int64)
    cols = np.zeros(n, np.int64)
    prefix = np.zeros(n, np.int64)
    seg_start = np.zeros(n + 1, np.int64)
    if n:
        np.cumsum(lengths[:-1] + gap, out=offsets[1:])
        np.cumsum(frames[:-1], out=cols[1:])
        np.cumsum((frames[:-1] + item - 1) // item, out=prefix[1:])
        np.cumsum(segs, out=seg_start[1:])
    total = int(seg_start[-1])
    seg_col = np.repeat(cols, segs) + (np.arange(total, dtype=np.int64) - np.repeat(seg_start[:-1], segs)) * step
    return frames, segs, offsets, cols, prefix, seg_start, seg_col


@dataclass
class PackPlan:
    """the host-side description of one pack. `index[j]` is the position of the pack's song j among the candidates `plan_pack`
    was given; `skipped` lists (position, reason) of the candidates left out."""
    kind: str                        # "logmel" | "cqt"
    hop: int
    n_frames: int
    step: int
    n_rows: int                      # n_mels, or 84 CQT bins
    min_len: int                     # songs need L > min_len (torch's reflect pad raises at or below n_fft/2, width/2)
    item: int                        # frames per work item
    gap: int                         # unused samples between two songs
    ld: int                          # row stride of the packed spectrogram, >= total_cols
    index: np.ndarray
    lengths: np.ndarray
    frames: np.ndarray               # T_i
    segs: np.ndarray                 # S_i
    offsets: np.ndarray              # first sample of song i in the pack
    cols: np.ndarray                 # first output column of song i
    prefix: np.ndarray               # work items of the songs before song i
    seg_start: np.ndarray            # (n + 1,): segments of the songs before song i; [-1] = total
    seg_col: np.ndarray              # (total_segs,): first column of every segment
    skipped: List[Tuple[int, str]] = field(default_factory=list)
    front: object = field(default=None, repr=False, compare=False)     # the front end the plan was made for (its device tables)

    @property
    def n_songs(self) -> int:
        return int(self.lengths.size)

    @property
    def total_samples(self) -> int:
        return int(self.offsets[-1] + self.lengths[-1]) if self.n_songs else 0

    @property
    def total_cols(self) -> int:
        return int(self.frames.sum())

    @property
    def total_items(self) -> int:
        return int(((self.frames + self.item - 1) // self.item).sum())

    @property
    def total_segs(self) -> int:
        return int(self.seg_col.size)

    @property
    def max_len(self) -> int:
        return int(self.lengths.max()) if self.n_songs else 0

    def table(self) -> np.ndarray:
        """(n_songs, 4) int64: the device table of the ragged front-end entries"""
        return np.ascontiguousarray(np.stack((self.offsets, self.lengths, self.cols, self.prefix), 1).astype(np.int64))

    def validate(self) -> "PackPlan":
        """re-derives every table from the lengths and compares; raises ValueError on any difference or any broken bound"""
        arrays = (self.index, self.lengths, self.frames, self.segs, self.offsets, self.cols, self.prefix, self.seg_start,
                  self.seg_col)
        if any(not isinstance(a, np.ndarray) or a.dtype != np.int64 or a.ndim != 1 for a in arrays):
            raise ValueError("pack tables must be 1-D int64 arrays")
        n = self.n_songs
        if n < 1:
            raise ValueError("a pack needs at least one song")
        if self.kind not in ("logmel", "cqt") or self.item != (LOGMEL_RUN if self.kind == "logmel" else CQT_TILE):
            raise ValueError("unknown pack kind or work-item size")
        if min(self.hop, self.n_frames, self.step, self.n_rows) < 1 or self.min_len < 0 or self.gap < 0:
            raise ValueError("hop, n_frames, step and n_rows must be positive")
        if any(a.size != n for a in (self.index, self.frames, self.segs, self.offsets, self.cols, self.prefix)) \
                or self.seg_start.size != n + 1:
            raise ValueError("pack tables disagree about the number of songs")
        if int(self.lengths.min()) <= self.min_len:
            raise ValueError(f"a song of {int(self.lengths.min())} samples is at or below the reflect-pad minimum {self.min_len}")
        if self.kind == "cqt" and self.max_len >= MAX_CQT_SONG:
            raise ValueError(f"a song of {self.max_len} samples exceeds the constant-Q kernel's limit of 2^28")
        want = _tables(self.lengths, self.hop, self.n_frames, self.step, self.item, self.gap)
        have = (self.frames, self.segs, self.offsets, self.cols, self.prefix, self.seg_start, self.seg_col)
        for name, a, b in zip(("frames", "segs", "offsets", "cols", "prefix", "seg_start", "seg_col"), have, want):
            if a.shape != b.shape or not np.array_equal(a, b):
                raise ValueError(f"pack table `{name}` does not follow from the song lengths")
        if self.total_samples >= MAX_PACK_SAMPLES:
            raise ValueError(f"a pack of {self.total_samples} samples: the limit is 2^30 - 1")
        if self.total_cols > self.ld:
            raise ValueError(f"{self.total_cols} columns do not fit the row stride {self.ld}")
        if self.total_items >= 1 << 31:
            raise ValueError("too many work items for one launch")
        # every segment inside its own song's columns (follows from the above; stated on its own because it is the bound the
        # gather kernel relies on)
        owner = np.repeat(np.arange(n), self.segs)
        if self.seg_col.size and (np.any(self.seg_col < self.cols[owner])
                                  or np.any(self.seg_col + self.n_frames > self.cols[owner] + self.frames[owner])):
            raise ValueError("a segment leaves its song's columns")
        return self

    def freeze(self) -> "PackPlan":
        for a in (self.index, self.lengths, self.frames, self.segs, self.offsets, self.cols, self.prefix, self.seg_start,
                  self.seg_col):
            a.flags.writeable = False
        return self


def plan_pack(lengths: Sequence[int], front, gap: int = 0, spare_cols: int = 0, require_segment: bool = True) -> PackPlan:
    """lengths: the sample counts of the candidate songs, in pack order; front: the LogMelFrontEnd or CQTFrontEnd the pack will
    run through. Candidates at or below the reflect-pad minimum, and (require_segment) those shorter than one segment, are left
    out and reported in `plan.skipped` — the reference's unfold raises for them and create_dummy_db skips the file
    (transformations.py:101-104). gap: unused samples between songs; spare_cols: columns of the row stride beyond the songs'.
    Raises ValueError when the remaining songs do not fit one pack (2^30 samples). A plan may come back empty (n_songs == 0)."""
    kind = front_kind(front)
    hop, n_frames, step = int(front.hop), int(front.n_frames), int(front.step)
    n_rows = int(front.n_mels) if kind == "logmel" else int(front.n_bins)
    min_len = int(front.n_fft) // 2 if kind == "logmel" else int(front.width) // 2
    item = LOGMEL_RUN if kind == "logmel" else CQT_TILE
    gap, spare_cols = int(gap), int(spare_cols)
    if gap < 0 or spare_cols < 0:
        raise ValueError("gap and spare_cols must not be negative")
    if step < 1:
        raise ValueError("the front end's segment step must be at least one frame")
    cand = [int(v) for v in lengths]
    keep, skipped = [], []
    for j, L in enumerate(cand):
        T = 1 + max(L, 0) // hop
        if L <= min_len:
            skipped.append((j, f"{L} samples: at or below the reflect-pad minimum of {min_len}"))
        elif require_segment and T < n_frames:
            skipped.append((j, f"{T} frames: shorter than one segment of {n_frames}"))
        else:
            keep.append(j)
    L = np.array([cand[j] for j in keep], dtype=np.int64)
    if L.size:
        total = int(L.sum()) + gap * (L.size - 1)
        if total >= MAX_PACK_SAMPLES:
            raise ValueError(f"a pack of {total} samples: the limit is 2^30 - 1; split the songs over several packs")
        if kind == "cqt" and int(L.max()) >= MAX_CQT_SONG:
            raise ValueError(f"a song of {int(L.max())} samples exceeds the constant-Q kernel's limit of 2^28")
    frames, segs, offsets, cols, prefix, seg_start, seg_col = _tables(L, hop, n_frames, step, item, gap)
    plan = PackPlan(kind, hop, n_frames, step, n_rows, min_len, item, gap, int(frames.sum()) + spare_cols,
                    np.array(keep, dtype=np.int64), L, frames, segs, offsets, cols, prefix, seg_start, seg_col, skipped, front)
    if plan.n_songs:
        plan.validate()
    return plan.freeze()


def check_wave(wave, length: Optional[int] = None) -> None:
    """a song is one mono fp32 waveform: a 1-D float32 tensor on the CPU or the GPU"""
    if not isinstance(wave, torch.Tensor) or wave.dim() != 1 or wave.dtype != torch.float32:
        what = f"{tuple(wave.shape)} {wave.dtype}" if isinstance(wave, torch.Tensor) else type(wave).__name__
        raise TypeError(f"a song must be a 1-D float32 tensor (mono waveform), got {what}")
    if length is not None and wave.numel() != length:
        raise ValueError(f"a song of {wave.numel()} samples where the plan has {length}")


class PackArena:
    """buffers a driver reuses from pack to pack (grown on demand, never shrunk): the pinned staging buffer, the device buffer of
    tables + waveforms and the packed spectrogram. Reusing the staging buffer is safe once the previous pack's upload has
    completed; fpdb.build_fp_db_from_waves ends every pack with a blocking device-to-host copy."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._host = self._dev = self._spec = None

    def host(self, nbytes: int) -> torch.Tensor:
        if self._host is None or self._host.numel() < nbytes:
            self._host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return self._host[:nbytes]

    def dev(self, nbytes: int) -> torch.Tensor:
        if self._dev is None or self._dev.numel() < nbytes:
            self._dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._dev[:nbytes]

    def spec(self, numel: int) -> torch.Tensor:
        if self._spec is None or self._spec.numel() < numel:
            self._spec = torch.empty(numel, dtype=torch.float32, device=self.device)
        return self._spec[:numel]


class WavePack:
    """one pack on the device: tables and waveforms in ONE buffer (one pinned staging copy, one upload), the front end run over
    all of it in one launch into `spec` (n_rows, ld), and `segments()` to cut micro-batches out of it.

    waves: the plan's songs in plan order (`waves[j]` has `plan.lengths[j]` samples), 1-D fp32 tensors on the CPU or on `device`.
    CPU songs travel through the staging buffer; songs already on the device are copied into their slot there."""

    def __init__(self, plan: PackPlan, waves: Sequence[torch.Tensor], device="cuda", arena: Optional[PackArena] = None):
        if not isinstance(plan, PackPlan):
            raise TypeError("WavePack takes a PackPlan from plan_pack")
        waves = list(waves)
        if len(waves) != plan.n_songs:
            raise ValueError(f"{len(waves)} songs for a plan of {plan.n_songs}")
        for w, L in zip(waves, plan.lengths):
            check_wave(w, int(L))
        plan.validate()
        front = plan.front
        if front_kind(front) != plan.kind or (int(front.hop), int(front.n_frames), int(front.step)) != (plan.hop, plan.n_frames, plan.step):
            raise ValueError("the plan does not describe its front end")
        self.plan, self.front = plan, front
        self.device = torch.device(device)
        arena = arena or PackArena(self.device)
        n, nseg, ns = plan.n_songs, plan.total_segs, plan.total_samples
        tb, sb = 8 * TABLE_COLS * n, 8 * nseg                  # int64 tables first: both stay 8-byte aligned
        host = arena.host(tb + sb + 4 * ns)
        host[:tb].view(torch.int64).copy_(torch.from_numpy(plan.table().reshape(-1)))
        if nseg:
            host[tb:tb + sb].view(torch.int64).copy_(torch.from_numpy(np.array(plan.seg_col)))      # a copy: the plan's is read-only
        hw = host[tb + sb:].view(torch.float32)
        on_dev = []
        for j, w in enumerate(waves):
            o, L = int(plan.offsets[j]), int(plan.lengths[j])
            if w.is_cuda:
                on_dev.append((o, L, w))
            else:
                hw[o:o + L].copy_(w)
        dev = arena.dev(host.numel())
        if on_dev and len(on_dev) == n:
            dev[:tb + sb].copy_(host[:tb + sb], non_blocking=True)     # nothing but the tables to upload
        else:
            dev.copy_(host, non_blocking=True)
        self._songs = dev[:tb].view(torch.int64)
        self._seg_col = dev[tb:tb + sb].view(torch.int64)
        self.wave = dev[tb + sb:].view(torch.float32)
        for o, L, w in on_dev:
            self.wave[o:o + L].copy_(w.to(self.device), non_blocking=True)
        self.spec = arena.spec(plan.n_rows * plan.ld).view(plan.n_rows, plan.ld)
        from . import ops
        if plan.kind == "logmel":
            ops.logmel_fft_ragged(self, front.n_fft, front.window, front.twiddle, front.fb, front.band, self.spec)
        else:
            ops.cqt_ragged(self, front.width, front.groups, front.taps, front.scale, self.spec)

    def song_spec(self, j: int) -> torch.Tensor:
        """(n_rows, T_j) view of song j's columns"""
        c, T = int(self.plan.cols[j]), int(self.plan.frames[j])
        return self.spec[:, c:c + T]

    def segments(self, s0: int, nseg: int, out: torch.Tensor) -> torch.Tensor:
        """segments s0 .. s0 + nseg - 1 of the pack's segment list into the first nseg rows of `out` (>= nseg, n_rows, n_frames),
        one launch; the rows behind them are not touched. Returns out[:nseg]."""
        from . import ops
        return ops.unfold_segments_ragged(self, int(s0), int(nseg), out)
