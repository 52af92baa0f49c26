"""The DSP of the reference's modules/data.py behind the decoder, on the MI355X: what NeuralSampleIDDataset.__getitem__ (:45-150)
does to four decoded stems -- mono downmix, torchaudio Resample, the `dur + offset` window, the SNR gate, the random split into
x_j (sample stems) and x_i (the remaining stem), the two crops, the silence test -- and the downmix + Resample of Sample100Dataset
(:222-224) in front of the train=False transforms. Decoding files stays with the caller.

    GPUResample(orig_freq, new_freq)   forward(audio (T,) or (C, T)) -> (T_out,): audio.mean(dim=0) + Resample in one launch
    StemBank(cfg, device)              the resampled training stems of many tracks in one flat device buffer
    GPUStemPairSampler(cfg, bank)      draw() on the host, forward(params) / batch(B) on the device: (x_i, x_j) pairs for the augmenters

DESIGN.md "Stem pairs" is the definition (csrc/stems.hip the kernels, tests/stem_pairs_oracle.py the restatement). Two stated
deviations: the resampler restates torchaudio's formula and is not checked against the package where it is not installed, and
batch() replaces the reference's "take the next index" re-draw by oversampling and packing the accepted clips."""
import math
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from .. import ops
from ..ops import resample_table  # noqa: F401  (part of this module's surface)

STEM_ROWS = ("bass + other", "vocals", "drums")      # data.py:76-78: the three training stems, in the order of torch.stack at :92


class GPUResample(nn.Module):
    """torchaudio.transforms.Resample(orig_freq, new_freq) with its defaults on the mono downmix of the input (data.py:59/70, :222-224):
    forward(audio) takes (T,) or (C, T) float32 on the device, C <= 8, and returns (ceil(new T / orig),)."""

    def __init__(self, orig_freq: int, new_freq: int):
        super().__init__()
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        if self.orig_freq != self.new_freq:
            ops.resample_compact(self.orig_freq, self.new_freq, ops.RESAMPLE_LDS_BYTES)      # refuse an oversized table here

    def forward(self, audio: torch.Tensor) -> torch.Tensor:
        return ops.resample_sinc(audio, self.orig_freq, self.new_freq)


def _clip_frames(cfg):
    fs = cfg["fs"]
    return int(fs * cfg["dur"]), int(fs * cfg["offset"])        # data.py:73-74


class StemBank:
    """Per track the three training stems of data.py:76-78 at cfg['fs'] -- bass + other, vocals, drums -- as (3, T_t) float32 rows in
    one flat device buffer that grows by doubling. `base` (int64 element offsets) and `length` (int32) are the device tables the
    sampler's kernels read. Growth and add() replace `buf`, `base` and `length`: fill the bank before capturing a step."""

    def __init__(self, cfg, device, capacity: int = 1 << 22):
        self.cfg, self.device = cfg, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("StemBank lives on the MI355X device; there is no host path")
        self.fs = int(cfg["fs"])
        L, O = _clip_frames(cfg)
        self.min_length = L + O
        self.buf = torch.empty((max(int(capacity), 1),), device=self.device, dtype=torch.float32)
        self.used = 0
        self.bases, self.lengths = [], []
        self.base = torch.empty((0,), device=self.device, dtype=torch.int64)
        self.length = torch.empty((0,), device=self.device, dtype=torch.int32)

    def __len__(self):
        return len(self.lengths)

    def nbytes(self) -> int:
        return self.used * 4

    def track(self, t: int) -> torch.Tensor:
        """(3, T_t) view of track t"""
        return self.buf[self.bases[t]:self.bases[t] + 3 * self.lengths[t]].view(3, self.lengths[t])

    def add_resampled(self, rows: torch.Tensor) -> int:
        """append (3, T) rows that are already at fs; returns the track's index"""
        if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape[0] != 3 or rows.dtype != torch.float32:
            raise RuntimeError("StemBank.add_resampled takes (3, T) float32 rows: bass + other, vocals, drums")
        T = rows.shape[1]
        if T < self.min_length:
            raise ValueError(f"track of {T} samples is shorter than int(fs * dur) + int(fs * offset) = {self.min_length}: the "
                             "reference skips it at every draw, the bank refuses it")
        if T >= 2 ** 31:
            raise ValueError("a track must have fewer than 2^31 samples")
        need = self.used + 3 * T
        if need > self.buf.numel():
            grown = torch.empty((max(2 * self.buf.numel(), need),), device=self.device, dtype=torch.float32)
            grown[:self.used].copy_(self.buf[:self.used])
            self.buf = grown
        self.buf[self.used:need].view(3, T).copy_(rows)
        self.bases.append(self.used)
        self.lengths.append(T)
        self.used = need
        self.base = torch.tensor(self.bases, dtype=torch.int64).to(self.device)
        self.length = torch.tensor(self.lengths, dtype=torch.int32).to(self.device)
        return len(self.lengths) - 1

    def add(self, stems: dict, sr: int) -> int:
        """decoded stems {'bass', 'other', 'vocals', 'drums'} ((T,) or (C, T) float32 at rate sr; other keys such as 'mix' are
        ignored): downmix and resample on the device, bass + other in fp32 after resampling, cut to the common length"""
        res = {}
        for name in ("bass", "other", "vocals", "drums"):
            if name not in stems:
                raise KeyError(f"StemBank.add needs the stem {name!r}")
            a = stems[name]
            if not isinstance(a, torch.Tensor) or a.dtype != torch.float32:
                raise RuntimeError("StemBank.add takes decoded float32 tensors")
            res[name] = ops.resample_sinc(a.to(self.device), int(sr), self.fs)
        bass_mix = res["bass"][:min(res["bass"].numel(), res["other"].numel())] + \
            res["other"][:min(res["bass"].numel(), res["other"].numel())]
        T = min(bass_mix.numel(), res["vocals"].numel(), res["drums"].numel())
        return self.add_resampled(torch.stack((bass_mix[:T], res["vocals"][:T], res["drums"][:T])))


class StemPairParams(NamedTuple):
    """one draw for N clips, device tensors: track (N,) i32, start (N,) i32 (first sample of the W-sample window), key (N, 3) f32 (the
    shuffle: valid stems are ordered by key), off_i / off_j (N,) i32 (crop offsets in [0, O))"""
    track: torch.Tensor
    start: torch.Tensor
    key: torch.Tensor
    off_i: torch.Tensor
    off_j: torch.Tensor


def draw_stem_pairs(lengths, W: int, O: int, N: int, generator: Optional[torch.Generator] = None) -> StemPairParams:
    """the host half of GPUStemPairSampler.draw: N clips over tracks of the given lengths (each >= W), fp64 uniforms from the
    generator -> host tensors. track = floor(u n_tracks), start = floor(u (length - W + 1)), key = three uniforms,
    off_i / off_j = floor(u O)."""
    u = torch.rand((7, N), dtype=torch.float64, generator=generator)                 # host draw: torch.manual_seed reproduces it
    n_tracks = len(lengths)
    track = torch.clamp(torch.floor(u[0] * n_tracks).to(torch.int64), max=n_tracks - 1)
    length = torch.tensor(list(lengths), dtype=torch.int64)[track]
    start = torch.minimum(torch.floor(u[1] * (length - W + 1).to(torch.float64)).to(torch.int64), length - W)
    off = torch.clamp(torch.floor(u[5:7] * O).to(torch.int64), max=O - 1)
    return StemPairParams(track.to(torch.int32), start.to(torch.int32), u[2:5].t().contiguous().to(torch.float32),
                          off[0].to(torch.int32), off[1].to(torch.int32))


class GPUStemPairSampler(nn.Module):
    """data.py:87-148 for a batch: L = int(fs dur), O = int(fs offset), W = L + O.

    draw(N) runs on the host in fp64 from a torch.Generator and returns device tensors; forward(params) -> (x_i, x_j, status, snr)
    and batch(B) -> (x_i, x_j, n_ok) run two launches (csrc/stems.hip), do no host synchronisation and allocate by host-known sizes
    only, so both can be captured; a replay reads the params' current contents. status: 0 accepted, 1 fewer than two stems pass the
    SNR gate, 2 a silent side; rejected rows are zero."""

    def __init__(self, cfg, bank: StemBank):
        super().__init__()
        self.cfg, self.bank = cfg, bank
        self.L, self.O = _clip_frames(cfg)
        self.W = self.L + self.O
        self.silence = float(cfg["silence"])
        if self.L < 1 or self.O < 1:
            raise ValueError("need int(fs * dur) >= 1 and int(fs * offset) >= 1 (the reference draws randint(0, offset_frames))")
        if int(cfg["fs"]) != bank.fs:
            raise ValueError("the bank was resampled to another fs")

    def draw(self, N: int, generator: Optional[torch.Generator] = None) -> StemPairParams:
        if len(self.bank) == 0:
            raise RuntimeError("the bank is empty")
        dev = self.bank.device
        return StemPairParams(*(t.to(dev) for t in draw_stem_pairs(self.bank.lengths, self.W, self.O, N, generator)))

    def _run(self, params: StemPairParams, pack):
        b = self.bank
        return ops.stem_pairs(b.buf, b.base, b.length, params.track, params.start, params.key, params.off_i, params.off_j, self.L,
                              self.O, self.silence, pack=pack)

    def forward(self, params: StemPairParams):
        return self._run(params, None)

    def batch(self, B: int, generator: Optional[torch.Generator] = None, oversample: float = 1.25,
              params: Optional[StemPairParams] = None):
        """B pairs from ceil(B * oversample) candidates (or from the given params): the accepted candidates in candidate order in rows
        0 .. n_ok - 1, zeros behind them; n_ok = min(accepted, B) is a device int32 scalar"""
        if params is None:
            if oversample < 1.0:
                raise ValueError("oversample >= 1")
            params = self.draw(int(math.ceil(B * oversample)), generator)
        x_i, x_j, n_ok, _, _ = self._run(params, int(B))
        return x_i, x_j, n_ok
