"""GPUTransformSampleID (the reference's modules/transformations.py) on the MI355X: the module train.py:100 and :146
construct and train.py:58 / test_fp.py call as `augment`.

    train=True    forward(x_i, x_j) -> (X_i, X_j), each (B, n_mels, T): MelSpectrogram + AmplitudeToDB of both waveform
                  batches, one launch each (frontend.LogMelFrontEnd.batch, csrc/frontend.hip)
    train=False   forward(x, None)  -> (segments (S, n_mels, n_frames), None) for one waveform given as (L,), (1, L) or
                  (1, 1, L); audio shorter than one segment comes back as the un-segmented (T, n_mels) matrix, the
                  reference's fall-through when unfold raises (transformations.py:101-104): callers test that shape.

The waveform augmentations (Gain, PitchShift, TimeStretch through audiomentations) run on DataLoader workers in the
reference (`cpu=True`); that constructor argument keeps raising here. Their GPU form is a module of its own, GPUWaveAugment
(below): the 'grafp' branch of forward(..., cpu=True) for a whole batch on the device, in front of `augment`. No module here
has parameters or buffers: nothing of them is ever saved.

GPUTransformCQT is the same module for arch 'resnet-ibn' (transformations.py:36,48: nnAudio CQT(sr=fs, hop_length=hop_len)
instead of the log-mel pair): (B, 84, T) magnitudes in training, (S, 84, n_frames) segments or the (T, 84) fall-through in
evaluation, through frontend.CQTFrontEnd (csrc/cqt.hip). It is a class of its own so that GPUTransformSampleID keeps refusing
the arch: at baseline/run_eval.py:241 substitute GPUTransformCQT(cfg, train=False) for GPUTransformSampleID(cfg, train=False)."""
import math
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .._lib import call
from ..frontend import CQTFrontEnd, LogMelFrontEnd


class GPUTransformSampleID(nn.Module):
    def __init__(self, cfg, ir_dir=None, train=True, cpu=False, max_transforms_1=1, max_transforms_2=1):
        super().__init__()
        if cpu:
            raise NotImplementedError("cpu=True is the audiomentations branch that runs on DataLoader workers (host DSP): keep the "
                                      "reference's GPUTransformSampleID(cpu=True) for it, or run GPUWaveAugment on the device in "
                                      "front of this module; this module is the GPU spectrogram half")
        arch = cfg.get("arch", "grafp")
        if arch == "resnet-ibn":
            raise NotImplementedError("arch 'resnet-ibn' (CQT front end of the baseline model) is a module of its own here: "
                                      "construct modules.transformations.GPUTransformCQT with the same arguments")
        if arch != "grafp":
            raise ValueError(f"Unsupported arch: {arch}")
        self.sample_rate, self.ir_dir, self.overlap, self.arch = cfg["fs"], ir_dir, cfg["overlap"], arch
        self.n_frames, self.train, self.cpu, self.cfg = cfg["n_frames"], train, cpu, cfg
        self.max_transforms_1, self.max_transforms_2 = max_transforms_1, max_transforms_2
        self._front = None                       # tables are built on the device of the first waveform

    def front(self, device) -> LogMelFrontEnd:
        device = torch.device(device)
        if self._front is None or self._front.device != device:
            self._front = LogMelFrontEnd(self.cfg, device, stft="fft")
        return self._front

    def forward(self, x_i, x_j):
        front = self.front(x_i.device)
        if self.train:
            return front.batch(x_i), front.batch(x_j)
        if x_i.dim() > 1 and x_i.shape[0] == 1:
            x_i = x_i.squeeze(0)                                             # transformations.py:96
        if x_i.dim() == 2 and x_i.shape[0] == 1:
            x_i = x_i.squeeze(0)                                             # (1, 1, L): the :99-100 squeeze
        lm = front.logmel(x_i)                                               # (n_mels, T)
        T = lm.shape[1]
        if T < front.n_frames:
            return lm.transpose(1, 0), None                                  # unfold raises in the reference: un-segmented (T, n_mels)
        S = (T - front.n_frames) // front.step + 1
        out = torch.empty((S, front.n_mels, front.n_frames), device=lm.device, dtype=torch.float32)
        call("nsid_unfold_segments", ops._p(lm), front.n_mels, T, front.n_frames, front.step, S, ops._p(out), ops._stream())
        return out, None


class GPUTransformCQT(nn.Module):
    """GPUTransformSampleID(arch='resnet-ibn') of the reference: the constant-Q front end of the ResNet-IBN baseline"""

    def __init__(self, cfg, ir_dir=None, train=True, cpu=False, max_transforms_1=1, max_transforms_2=1):
        super().__init__()
        if cpu:
            raise NotImplementedError("cpu=True is the audiomentations branch that runs on DataLoader workers (host DSP): keep the "
                                      "reference's GPUTransformSampleID(cpu=True) for it; this module is the GPU spectrogram half")
        self.sample_rate, self.ir_dir, self.overlap, self.arch = cfg["fs"], ir_dir, cfg["overlap"], "resnet-ibn"
        self.n_frames, self.train, self.cpu, self.cfg = cfg["n_frames"], train, cpu, cfg
        self.max_transforms_1, self.max_transforms_2 = max_transforms_1, max_transforms_2
        self._front = None                       # tables are built on the device of the first waveform

    def front(self, device) -> CQTFrontEnd:
        device = torch.device(device)
        if self._front is None or self._front.device != device:
            self._front = CQTFrontEnd(self.cfg, device)
        return self._front

    def forward(self, x_i, x_j):
        front = self.front(x_i.device)
        if self.train:
            return front.batch(x_i), front.batch(x_j)
        if x_i.dim() > 1 and x_i.shape[0] == 1:
            x_i = x_i.squeeze(0)                                             # transformations.py:96
        if x_i.dim() == 2 and x_i.shape[0] == 1:
            x_i = x_i.squeeze(0)                                             # (1, 1, L): the :99-100 squeeze
        spec = front.cqt(x_i)                                                # (84, T)
        T = spec.shape[1]
        if T < front.n_frames:
            return spec.transpose(1, 0), None                                # unfold raises in the reference: un-segmented (T, 84)
        S = (T - front.n_frames) // front.step + 1
        out = torch.empty((S, front.n_bins, front.n_frames), device=spec.device, dtype=torch.float32)
        call("nsid_unfold_segments", ops._p(spec), front.n_bins, T, front.n_frames, front.step, S, ops._p(out), ops._stream())
        return out, None


AUG_ZEROS, AUG_PRECISION = 64, 512                   # resampling filter: zero crossings, table points per zero crossing
AUG_ROLLOFF, AUG_BETA = 0.9475937167399596, 14.769656459379492     # resampy's kaiser_best design
AUG_CHUNK = 64                                       # clips per pass through the spectrum workspaces


def aug_filter_table() -> np.ndarray:
    """half of the Kaiser-windowed sinc, fp64, AUG_ZEROS * AUG_PRECISION + 1 points; the kernel and the oracle round it to fp32 and
    interpolate linearly: table and interpolation together are the filter's definition"""
    n = AUG_ZEROS * AUG_PRECISION
    return np.kaiser(2 * n + 1, AUG_BETA)[n:] * AUG_ROLLOFF * np.sinc(AUG_ROLLOFF * np.linspace(0, AUG_ZEROS, n + 1))


def aug_twiddles() -> torch.Tensor:
    """(2048, 2) = (cos, sin)(-2 pi j / 2048), evaluated in fp64"""
    ang = -2.0 * math.pi * torch.arange(ops.AUG_N_FFT, dtype=torch.float64) / ops.AUG_N_FFT
    return torch.stack((torch.cos(ang), torch.sin(ang)), 1).to(torch.float32).contiguous()


class WaveAugmentParams(NamedTuple):
    """one draw for a batch: device tensors gain (B,) f32 linear, mode (B,) i32 (0 = time stretch, 1 = pitch shift), rate (B,) f32;
    semitones (B,) f64 on the host is the pitch draw the rates of the mode-1 clips come from (NaN for mode 0)"""
    gain: torch.Tensor
    mode: torch.Tensor
    rate: torch.Tensor
    semitones: Optional[torch.Tensor] = None


class GPUWaveAugment(nn.Module):
    """The 'grafp' branch of the reference's GPUTransformSampleID.forward(x_i, x_j) with cpu=True (transformations.py:39-46, :81-86)
    for a batch on the device:

        x_i_out = T2(gain_b * x_j + x_i)[:L], zero-padded to L        x_j: the sample stems, x_i: the remaining stem
        x_j_out = x_j

    gain_b = 10^(g/20), g ~ U(-cfg.gain, cfg.gain) (audiomentations Gain); T2 = with probability 1/2 each a TimeStretch by
    rate ~ U(min_rate, max_rate) or a PitchShift by n ~ U(-pitch_shift, pitch_shift) semitones, both librosa's phase vocoder
    (csrc/augment.hip, four launches per chunk of AUG_CHUNK clips; DESIGN.md "Waveform augmentations" is the definition).
    max_transforms_1 = 0: no gain; max_transforms_2 = 0: rate 1 for every clip.

    draw() runs on the host from a torch.Generator; forward() with given params does no host synchronisation and nothing in it
    depends on the drawn values on the host side (extents come from the config's bounds), so it can be captured."""

    def __init__(self, cfg, max_transforms_1=1, max_transforms_2=1):
        super().__init__()
        arch = cfg.get("arch", "grafp")
        if arch != "grafp":
            raise NotImplementedError(f"GPUWaveAugment is the 'grafp' augmentation set (Gain, PitchShift, TimeStretch); arch {arch!r} "
                                      "uses the reference's fx_util chain, which stays host DSP")
        self.cfg = cfg
        self.max_transforms_1, self.max_transforms_2 = max_transforms_1, max_transforms_2
        self.gain_db = float(cfg["gain"])
        self.min_rate, self.max_rate, self.pitch_shift = float(cfg["min_rate"]), float(cfg["max_rate"]), float(cfg["pitch_shift"])
        if not 0.0 < self.min_rate <= self.max_rate or self.pitch_shift < 0:
            raise ValueError("need 0 < min_rate <= max_rate and pitch_shift >= 0")
        # the host-side bounds every extent comes from: float32, as the kernels see them
        lo = min(self.min_rate, 2.0 ** (-self.pitch_shift / 12.0), 1.0)
        hi = max(self.max_rate, 2.0 ** (self.pitch_shift / 12.0), 1.0)
        self.rate_lo, self.rate_hi = float(np.float32(lo)), float(np.float32(hi))      # rounding is monotonic: draws stay inside
        self._ws = {}                                   # (device, B, L) -> tables and workspaces

    def extents(self, L: int):
        """(T_in, T_out_max, S_max): frames in, most frames after the vocoder, most samples after the inverse STFT"""
        return ops.aug_frames_in(L), ops.aug_frames_out_max(L, self.rate_lo), ops.aug_stretched_max(L, self.rate_lo)

    def draw(self, B: int, generator: Optional[torch.Generator] = None, device="cuda") -> WaveAugmentParams:
        u = torch.rand((4, B), dtype=torch.float64, generator=generator)             # host draw: torch.manual_seed reproduces it
        g_db = (2.0 * u[0] - 1.0) * self.gain_db if self.max_transforms_1 else torch.zeros(B, dtype=torch.float64)
        gain = torch.pow(10.0, g_db / 20.0)
        mode = (u[1] >= 0.5).to(torch.int32)
        stretch = self.min_rate + u[2] * (self.max_rate - self.min_rate)
        semis = (2.0 * u[3] - 1.0) * self.pitch_shift
        rate = torch.where(mode == 1, torch.pow(2.0, -semis / 12.0), stretch)        # fp64 first, one rounding to fp32
        semis = torch.where(mode == 1, semis, torch.full_like(semis, float("nan")))
        if not self.max_transforms_2:
            mode, rate, semis = torch.zeros_like(mode), torch.ones_like(rate), torch.full_like(semis, float("nan"))
        return WaveAugmentParams(gain.to(torch.float32).to(device), mode.to(device), rate.to(torch.float32).to(device), semis)

    def _workspace(self, device, B, L):
        key = (device, B, L)
        ws = self._ws.get(key)
        if ws is None:
            T_in, T_max, S_max = self.extents(L)
            Bc = min(B, AUG_CHUNK)
            tables = next((w for (d, _, _), w in self._ws.items() if d == device), None)
            ws = {
                "window": tables["window"] if tables else
                torch.hann_window(ops.AUG_N_FFT, periodic=True, dtype=torch.float64).to(torch.float32).to(device),
                "twiddle": tables["twiddle"] if tables else aug_twiddles().to(device),
                "table": tables["table"] if tables else torch.from_numpy(aug_filter_table().astype(np.float32)).to(device),
                "spec": torch.empty((Bc, T_in, ops.AUG_BINS, 2), device=device, dtype=torch.float32),
                "voc": torch.empty((Bc, T_max, ops.AUG_BINS, 2), device=device, dtype=torch.float32),
                "wave": torch.empty((Bc, S_max), device=device, dtype=torch.float32),
                "chunk": Bc,
            }
            self._ws[key] = ws
        return ws

    def workspace_bytes(self, B: int, L: int) -> int:
        T_in, T_max, S_max = self.extents(L)
        return min(B, AUG_CHUNK) * ((T_in + T_max) * ops.AUG_BINS * 8 + S_max * 4)

    def forward(self, x_i, x_j, params: Optional[WaveAugmentParams] = None):
        for x in (x_i, x_j):
            if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
                raise RuntimeError("GPUWaveAugment takes (B, L) float32 waveforms on the MI355X device with a contiguous last "
                                   "dimension; there is no host path")
        if x_i.shape != x_j.shape:
            raise RuntimeError("x_i and x_j must have one shape (B, L)")
        B, L = x_i.shape
        if params is None:
            params = self.draw(B, device=x_i.device)
        gain, mode, rate = params.gain, params.mode, params.rate
        if not self.max_transforms_1:
            gain = torch.ones_like(gain)
        if not self.max_transforms_2:
            mode, rate = torch.zeros_like(mode), torch.ones_like(rate)
        ws = self._workspace(x_i.device, B, L)
        out = torch.empty((B, L), device=x_i.device, dtype=torch.float32)
        lo, hi = self.rate_lo, self.rate_hi
        for b0 in range(0, B, ws["chunk"]):
            b1 = min(B, b0 + ws["chunk"])
            n, g, m, r = b1 - b0, gain[b0:b1], mode[b0:b1], rate[b0:b1]
            ops.aug_stft(x_i[b0:b1], x_j[b0:b1], g, ws["window"], ws["twiddle"], ws["spec"])
            ops.aug_vocoder(ws["spec"], n, L, r, lo, hi, ws["voc"])
            ops.aug_istft(ws["voc"], n, L, r, lo, hi, ws["window"], ws["twiddle"], ws["wave"])
            ops.aug_finish(ws["wave"], n, L, m, r, lo, hi, ws["table"], out[b0:b1])
        return out, x_j
