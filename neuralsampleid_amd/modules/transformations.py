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
has parameters or buffers: nothing of them is ever saved. GPUBaselineWaveAugment (at the end) is the same for arch 'resnet-ibn':
the fx_util chain (BandEQ, Compressor, Gain; PitchShift, TimeStretch, FrameLevelCorruption) for a batch on the device.

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
from .._lib import DEFINES, call
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
                                      "reference's GPUTransformSampleID(cpu=True) for it, or run GPUBaselineWaveAugment on the device "
                                      "in front of this module; this module is the GPU spectrogram half")
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


AUG_ZEROS, AUG_PRECISION = DEFINES["NSID_AUG_ZEROS"], DEFINES["NSID_AUG_PRECISION"]      # filter table: zero crossings, points each
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
                                      "uses the reference's fx_util chain: construct GPUBaselineWaveAugment with the same arguments")
        self._configure(cfg, max_transforms_1, max_transforms_2)

    def _configure(self, cfg, max_transforms_1, max_transforms_2):
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


# ---- arch 'resnet-ibn': the fx_util chain ------------------------------------------------------------------------------------------
FX_SECTIONS = 32                                     # 8 bands x order 4: width of the section table
FX_T1_EQ, FX_T1_COMPRESS, FX_T1_GAIN = 0, 1, 2       # mode1
FX_T2_STRETCH, FX_T2_PITCH, FX_T2_DUPLICATE, FX_T2_REMOVE, FX_T2_SILENCE = 0, 1, 2, 3, 4      # mode2; 2..4: frame edits
FX_OP_DUPLICATE, FX_OP_REMOVE, FX_OP_SILENCE = 1, 2, 4                                       # frame_ops bits
EQ_BANDS, EQ_CENTRE, EQ_BANDWIDTH, EQ_GAIN_DB = (1, 8), (50.0, 8000.0), (0.01, 1.0), (-20.0, 10.0)      # fx_util.BandEQ's defaults
EQ_ORDERS = (2, 3, 4)                                # roll-off 12, 18, 24 dB per octave
EQ_NYQUIST_FRACTION = 0.9999
FRAME_FPS, FRAME_PROB = (0.5, 5.0), 0.1              # fx_util.FrameLevelCorruption's defaults


def hz_to_mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, np.float64) / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, np.float64) / 2595.0) - 1.0)


def butter_bandpass_sos(order: int, lo: float, hi: float, fs: float) -> np.ndarray:
    """Butterworth band-pass of `order` between lo and hi Hz as `order` second-order sections, (order, 5) fp64 rows b0, b1, b2, a1,
    a2 (a0 = 1): the analog prototype's poles, low-pass to band-pass, bilinear transform with pre-warped edges, conjugate pairs to
    sections -- scipy.signal.butter(order, [lo, hi], 'bandpass', fs=fs, output='sos') up to the pairing and the order of the
    sections. Every section takes one zero at +1 and one at -1; the filter's gain sits on the first section."""
    if not 0.0 < lo < hi < 0.5 * fs:
        raise ValueError("need 0 < lo < hi < fs / 2")
    proto = -np.exp(1j * np.pi * np.arange(-order + 1, order, 2) / (2.0 * order))
    w1, w2 = 4.0 * np.tan(np.pi * lo / fs), 4.0 * np.tan(np.pi * hi / fs)         # pre-warped at the bilinear transform's fs = 2
    bw, w0 = w2 - w1, np.sqrt(w1 * w2)
    p_lp = proto * (0.5 * bw)
    root = np.sqrt(p_lp * p_lp - w0 * w0 + 0j)
    p_s = np.concatenate([p_lp + root, p_lp - root])                              # 2 * order analog poles, `order` zeros at 0
    p_z = (4.0 + p_s) / (4.0 - p_s)
    k = (bw ** order) * np.real(4.0 ** order / np.prod(4.0 - p_s))                # zeros at 0 -> +1 (factor 4 each), at infinity -> -1
    cplx = np.abs(p_z.imag) > 1e-12 * np.abs(p_z)
    upper = sorted(p_z[cplx & (p_z.imag > 0)], key=abs)
    real = sorted(p_z[~cplx].real)
    if len(real) % 2 or 2 * len(upper) + len(real) != 2 * order:
        raise ValueError("poles do not pair")
    rows = [(-2.0 * p.real, p.real * p.real + p.imag * p.imag) for p in upper]
    rows += [(-(real[i] + real[i + 1]), real[i] * real[i + 1]) for i in range(0, len(real), 2)]
    sos = np.array([[1.0, 0.0, -1.0, a1, a2] for a1, a2 in rows], np.float64)
    sos[0, :3] *= k
    return sos


class BaselineAugmentParams(NamedTuple):
    """one draw for a batch, device tensors only:
    mode1 (B,) i32       T1: 0 band EQ, 1 compressor, anything else gain
    gain (B,) f32        linear gain of the sample stems in the mix: the Gain draw for mode1 = 2, 1 otherwise
    cmp (B, 4) f64       compressor threshold (linear), ratio, attack and release coefficients
    sos (B, 32, 6) f64   band EQ sections b0, b1, b2, a1, a2 and the factor on the section's output (a band's gain on its last one)
    n_sec (B,) i32       sections in use
    mode2 (B,) i32       T2: 0 time stretch, 1 pitch shift, 2 / 3 / 4 frame duplicate / remove / silence; anything else is 0
    rate (B,) f32        vocoder rate (1 for the frame edits)
    frame_size (B,) i32  samples per frame
    frame_ops (B, F) i32 per frame: bit 1 duplicate, 2 remove, 4 silence"""
    mode1: torch.Tensor
    gain: torch.Tensor
    cmp: torch.Tensor
    sos: torch.Tensor
    n_sec: torch.Tensor
    mode2: torch.Tensor
    rate: torch.Tensor
    frame_size: torch.Tensor
    frame_ops: torch.Tensor


class GPUBaselineWaveAugment(GPUWaveAugment):
    """The 'resnet-ibn' branch of the reference's GPUTransformSampleID.forward(x_i, x_j) with cpu=True (transformations.py:47-64,
    :84-89) for a batch on the device:

        x_i_out = T2(T1(x_j) + x_i)[:L], zero-padded to L        x_j: the sample stems, x_i: the remaining stem
        x_j_out = x_j

    T1 = one of BandEQ, Compressor, Gain, T2 = one of PitchShift, TimeStretch and the three FrameLevelCorruption instances
    (duplicate-only, remove-only, silence-only), each picked uniformly per clip. As in the reference the number of EQ bands and their
    gains are drawn once, at construction; every draw() re-draws the bands' filters. DESIGN.md "Baseline waveform augmentations" is the
    definition. max_transforms_1 = 0: T1 is the identity; max_transforms_2 = 0: rate 1 and no frame edit.

    forward(): nsid_aug_compress and nsid_aug_biquad write T1 of their clips into a (B, L) copy of x_j, the four launches of
    GPUWaveAugment run on the mix of every clip (the frame-edit clips at rate 1), nsid_aug_frames overwrites the rows of the
    frame-edit clips. No host synchronisation with given params; it can be captured."""

    def __init__(self, cfg, max_transforms_1=1, max_transforms_2=1, generator: Optional[torch.Generator] = None):
        nn.Module.__init__(self)
        arch = cfg.get("arch", "grafp")
        if arch != "resnet-ibn":
            raise NotImplementedError(f"GPUBaselineWaveAugment is the 'resnet-ibn' augmentation set; arch {arch!r} is GPUWaveAugment's")
        self._configure(cfg, max_transforms_1, max_transforms_2)
        self.fs = float(cfg["fs"])
        self.dc_threshold = tuple(float(v) for v in cfg["DC_threshold"])
        self.dc_ratio = tuple(float(v) for v in cfg["DC_ratio"])
        self.dc_attack = tuple(float(v) for v in cfg["DC_attack"])
        self.dc_release = tuple(float(v) for v in cfg["DC_release"])
        self.num_bands = int(torch.randint(EQ_BANDS[0], EQ_BANDS[1] + 1, (1,), generator=generator))
        u = torch.rand(self.num_bands, dtype=torch.float64, generator=generator)
        self.band_gains_db = (EQ_GAIN_DB[0] + u * (EQ_GAIN_DB[1] - EQ_GAIN_DB[0])).tolist()

    def frames_max(self, L: int) -> int:
        """the most frames a clip of L samples is cut into: the shortest frame is int(fs / 5.0) samples"""
        return -(-L // int(self.fs / FRAME_FPS[1]))

    def band_sections(self, centre: float, fraction: float, order: int) -> np.ndarray:
        bw = centre * fraction
        return butter_bandpass_sos(order, centre - 0.5 * bw, min(centre + 0.5 * bw, EQ_NYQUIST_FRACTION * 0.5 * self.fs), self.fs)

    def draw(self, B: int, generator: Optional[torch.Generator] = None, device="cuda", L: Optional[int] = None) -> BaselineAugmentParams:
        """L: samples per clip (the frame table's width follows it); the config's fs * dur when not given"""
        L = int(self.fs * float(self.cfg["dur"])) if L is None else int(L)
        F, nb = self.frames_max(L), self.num_bands
        u = torch.rand((10 + 3 * nb + F, B), dtype=torch.float64, generator=generator).numpy()      # host draw, fp64
        mode1 = np.minimum((u[0] * 3).astype(np.int32), 2) if self.max_transforms_1 else np.full(B, FX_T1_GAIN, np.int32)
        mode2 = np.minimum((u[1] * 5).astype(np.int32), 4) if self.max_transforms_2 else np.zeros(B, np.int32)
        g_db = (2.0 * u[2] - 1.0) * self.gain_db
        gain = np.where(mode1 == FX_T1_GAIN, 10.0 ** (g_db / 20.0), 1.0) if self.max_transforms_1 else np.ones(B)
        stretch = self.min_rate + u[3] * (self.max_rate - self.min_rate)
        semis = (2.0 * u[4] - 1.0) * self.pitch_shift
        rate = np.where(mode2 == FX_T2_PITCH, 2.0 ** (-semis / 12.0), np.where(mode2 == FX_T2_STRETCH, stretch, 1.0))
        if not self.max_transforms_2:
            rate = np.ones(B)
        # compressor
        thr_db = self.dc_threshold[0] + u[5] * (self.dc_threshold[1] - self.dc_threshold[0])
        ratio = np.asarray(self.dc_ratio)[np.minimum((u[6] * len(self.dc_ratio)).astype(np.int64), len(self.dc_ratio) - 1)]
        t_att = self.dc_attack[0] + u[7] * (self.dc_attack[1] - self.dc_attack[0])
        t_rel = self.dc_release[0] + u[8] * (self.dc_release[1] - self.dc_release[0])
        cmp = np.stack([10.0 ** (thr_db / 20.0), ratio, np.exp(-1.0 / (self.fs * t_att)), np.exp(-1.0 / (self.fs * t_rel))], 1)
        # band EQ: the sections of the EQ clips; identity rows elsewhere
        sos = np.zeros((B, FX_SECTIONS, 6), np.float64)
        sos[:, :, 0] = sos[:, :, 5] = 1.0
        n_sec = np.zeros(B, np.int32)
        m_lo, m_hi = hz_to_mel(EQ_CENTRE[0]), hz_to_mel(EQ_CENTRE[1])
        for b in np.nonzero(mode1 == FX_T1_EQ)[0]:
            n = 0
            for k in range(nb):
                uc, ub, uo = u[10 + 3 * k:13 + 3 * k, b]
                order = EQ_ORDERS[min(int(uo * len(EQ_ORDERS)), len(EQ_ORDERS) - 1)]
                sec = self.band_sections(float(mel_to_hz(m_lo + uc * (m_hi - m_lo))),
                                         EQ_BANDWIDTH[0] + ub * (EQ_BANDWIDTH[1] - EQ_BANDWIDTH[0]), order)
                sos[b, n:n + order, :5] = sec
                sos[b, n + order - 1, 5] = 10.0 ** (self.band_gains_db[k] / 20.0)
                n += order
            n_sec[b] = n
        # frame edits
        fps = FRAME_FPS[0] + u[9] * (FRAME_FPS[1] - FRAME_FPS[0])
        frame_size = (self.fs / fps).astype(np.int32)
        bit = np.select([mode2 == FX_T2_DUPLICATE, mode2 == FX_T2_REMOVE, mode2 == FX_T2_SILENCE],
                        [FX_OP_DUPLICATE, FX_OP_REMOVE, FX_OP_SILENCE], 0).astype(np.int32)
        frame_ops = np.ascontiguousarray((u[10 + 3 * nb:] < FRAME_PROB).T.astype(np.int32) * bit[:, None])

        def dev(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(device)
        return BaselineAugmentParams(dev(mode1, torch.int32), dev(gain, torch.float32), dev(cmp, torch.float64), dev(sos, torch.float64),
                                     dev(n_sec, torch.int32), dev(mode2, torch.int32), dev(rate, torch.float32),
                                     dev(frame_size, torch.int32), dev(frame_ops, torch.int32))

    def workspace_bytes(self, B: int, L: int) -> int:
        return super().workspace_bytes(B, L) + 4 * B * L

    def forward(self, x_i, x_j, params: Optional[BaselineAugmentParams] = None):
        for x in (x_i, x_j):
            if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
                raise RuntimeError("GPUBaselineWaveAugment takes (B, L) float32 waveforms on the MI355X device with a contiguous last "
                                   "dimension; there is no host path")
        if x_i.shape != x_j.shape:
            raise RuntimeError("x_i and x_j must have one shape (B, L)")
        B, L = x_i.shape
        if params is None:
            params = self.draw(B, device=x_i.device, L=L)
        p = params
        mode1, gain, mode2, rate = p.mode1, p.gain, p.mode2, p.rate
        if not self.max_transforms_1:
            mode1, gain = torch.full_like(mode1, FX_T1_GAIN), torch.ones_like(gain)
        if not self.max_transforms_2:
            mode2, rate = torch.zeros_like(mode2), torch.ones_like(rate)
        ws = self._workspace(x_i.device, B, L)
        if "t1" not in ws:
            ws["t1"] = torch.empty((B, L), device=x_i.device, dtype=torch.float32)
        t1 = ws["t1"]
        t1.copy_(x_j)                                    # the gain clips' rows; the two T1 kernels overwrite theirs
        ops.aug_compress(x_j, mode1, p.cmp, t1)
        ops.aug_biquad(x_j, mode1, p.sos, p.n_sec, t1)
        out = torch.empty((B, L), device=x_i.device, dtype=torch.float32)
        lo, hi = self.rate_lo, self.rate_hi
        for b0 in range(0, B, ws["chunk"]):
            b1 = min(B, b0 + ws["chunk"])
            n, r = b1 - b0, rate[b0:b1]
            ops.aug_stft(x_i[b0:b1], t1[b0:b1], gain[b0:b1], ws["window"], ws["twiddle"], ws["spec"])
            ops.aug_vocoder(ws["spec"], n, L, r, lo, hi, ws["voc"])
            ops.aug_istft(ws["voc"], n, L, r, lo, hi, ws["window"], ws["twiddle"], ws["wave"])
            ops.aug_finish(ws["wave"], n, L, mode2[b0:b1], r, lo, hi, ws["table"], out[b0:b1])
        ops.aug_frames(x_i, t1, gain, mode2, p.frame_size, p.frame_ops, out)
        return out, x_j
