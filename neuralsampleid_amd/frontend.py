"""Log-mel front end on the MI355X: waveform -> (S, n_mels, n_frames) segments for the encoder.

Mirrors the evaluation branch of the reference's GPUTransformSampleID (modules/transformations.py:27-34 and :94-105):
    MelSpectrogram(sample_rate=fs, win_length, hop_length, n_fft, n_mels)   torchaudio 2.3.0 defaults: f_min 0, f_max fs/2,
        center=True / reflect pad, periodic Hann window, power 2.0, HTK mel scale, norm None, onesided
    AmplitudeToDB()                                                         stype power: 10*log10(clamp(x, 1e-10)), ref 1
    X.transpose -> unfold(0, size=n_frames, step=int(n_frames*(1-overlap))) -> (S, n_mels, n_frames)

MI355X form: the STFT is one exact-fp32 MFMA GEMM — frames are overlapping rows of the reflect-padded waveform (row stride
= hop, no frame matrix is materialised) against the constant matrix [hann*cos ; -hann*sin] — followed by a per-frame
power/mel/dB kernel and the segment gather (csrc/misc.hip). Everything is stream-ordered; no host sync.

stft="fft" takes the fused kernel instead (csrc/frontend.hip, nsid_logmel_fft): reflection by index arithmetic, a real FFT in
LDS and registers, power, mel sums and dB in one launch for a whole batch of clips — `batch(waves)`, the `augment` of the
reference's train.py:58 (GPUTransformSampleID(train=True)); `logmel()` and `__call__` go through it with B = 1. The default
stays "gemm": the two modes differ by fp32 rounding, which stored fingerprints would see.

CQTFrontEnd is the same surface for the ResNet-IBN baseline (GPUTransformSampleID(arch='resnet-ibn'), transformations.py:36,48:
nnAudio CQT(sr=fs, hop_length=hop_len)): waveform -> constant-Q magnitudes (84, T) -> (S, 84, n_frames) segments, one launch of
the banded kernel (csrc/cqt.hip, nsid_cqt) for a whole batch of clips."""
import math

import numpy as np
import torch

from . import ops
from ._lib import DEFINES, call


def mel_filterbank(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int) -> torch.Tensor:
    """torchaudio.functional.melscale_fbanks(norm=None, mel_scale='htk') restated: (n_freqs, n_mels), float32 arithmetic
    in the same order (triangles from the slopes between the mel-spaced centre frequencies)."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = torch.linspace(m_min, m_max, n_mels + 2)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1), torch.min(down, up))


class LogMelFrontEnd:
    """front = LogMelFrontEnd(cfg, device); segs = front(wave)  — wave (L,) fp32 on the GPU, segs (S, n_mels, n_frames)."""

    def __init__(self, cfg: dict, device="cuda", stft: str = "gemm"):
        if stft not in ("gemm", "fft"):
            raise ValueError(f"stft must be 'gemm' or 'fft', got {stft!r}")
        self.stft = stft
        self.fs, self.n_fft, self.hop = int(cfg["fs"]), int(cfg["n_fft"]), int(cfg["hop_len"])
        self.win = int(cfg.get("win_len", self.n_fft))
        self.n_mels, self.n_frames = int(cfg["n_mels"]), int(cfg["n_frames"])
        self.step = int(self.n_frames * (1 - float(cfg["overlap"])))          # transformations.py:102
        if self.win != self.n_fft:
            raise NotImplementedError("win_length != n_fft (the reference config uses 1024/1024)")
        if stft == "gemm" and (self.n_fft % 4 or self.hop % 4):
            raise NotImplementedError("n_fft and hop_len must be multiples of 4 (16-byte rows of the framing GEMM)")
        if stft == "fft" and (self.n_fft != 1024 or not 1 <= self.hop <= self.n_fft):
            raise NotImplementedError("stft='fft' is built for n_fft = 1024 with 1 <= hop_len <= n_fft (csrc/frontend.hip)")
        self.n_freq = self.n_fft // 2 + 1
        self.device = torch.device(device)
        # tables of the fused kernel, evaluated in fp64: the periodic Hann window and the twiddles e^(-2 pi i j / n_fft)
        j = torch.arange(self.n_fft, dtype=torch.float64)
        self.window = torch.hann_window(self.n_fft, periodic=True, dtype=torch.float64).to(torch.float32).to(self.device)
        ang = -2.0 * math.pi * j / self.n_fft
        self.twiddle = torch.stack((torch.cos(ang), torch.sin(ang)), 1).to(torch.float32).contiguous().to(self.device)
        # DFT matrix with the periodic Hann window folded in, built in fp64: rows [0, n_freq) = w*cos, then -w*sin
        n = torch.arange(self.n_fft, dtype=torch.float64)
        k = torch.arange(self.n_freq, dtype=torch.float64).unsqueeze(1)
        win = torch.hann_window(self.n_fft, periodic=True, dtype=torch.float64)
        ang = 2.0 * math.pi * k * n / self.n_fft
        rows = 2 * self.n_freq
        self.ld = (rows + 3) // 4 * 4
        W = torch.zeros(self.ld, self.n_fft, dtype=torch.float64)
        W[:self.n_freq] = win * torch.cos(ang)
        W[self.n_freq:rows] = -win * torch.sin(ang)
        self.W = W.to(torch.float32).to(self.device).contiguous() if stft == "gemm" else None     # 4 MB the fused kernel never reads
        fb = mel_filterbank(self.n_freq, 0.0, float(self.fs // 2), self.n_mels, self.fs).t().contiguous()   # (n_mels, n_freq)
        nz = fb > 0
        lo = torch.where(nz.any(1), nz.float().argmax(1), torch.zeros(self.n_mels, dtype=torch.long))
        hi = torch.where(nz.any(1), self.n_freq - nz.flip(1).float().argmax(1), torch.zeros(self.n_mels, dtype=torch.long))
        self.fb = fb.to(self.device)
        self.band = torch.stack((lo, hi), 1).to(torch.int32).contiguous().to(self.device)

    def n_frames_of(self, L: int) -> int:
        return 1 + L // self.hop                                             # torch.stft, center=True

    def batch(self, waves: torch.Tensor) -> torch.Tensor:
        """(B, L) fp32 on the GPU -> (B, n_mels, T) dB in one launch of the fused kernel, whatever `stft` says for the
        single-waveform calls; stream-ordered, no allocation besides the result, capture-safe. Clip b of the result is
        bit-equal to the same clip in a call of its own."""
        return ops.logmel_fft(waves, self.n_fft, self.hop, self.window, self.twiddle, self.fb, self.band)

    def logmel(self, wave: torch.Tensor) -> torch.Tensor:
        """(L,) fp32 on the GPU -> (n_mels, T) dB"""
        if wave.dim() != 1 or not wave.is_cuda or wave.dtype != torch.float32:
            raise RuntimeError("the front end takes one mono fp32 waveform on the MI355X device")
        if self.stft == "fft":
            return self.batch(wave.contiguous().unsqueeze(0))[0]
        wave = wave.contiguous()
        L, pad = wave.numel(), self.n_fft // 2
        T = self.n_frames_of(L)
        s = ops._stream()
        padded = torch.empty(L + 2 * pad, device=wave.device, dtype=torch.float32)
        call("nsid_reflect_pad", ops._p(wave), L, pad, ops._p(padded), s)
        prec = ops.get_gemm_precision()
        ops.set_gemm_precision("fp32")                                       # dB dynamic range needs exact fp32 products
        try:
            spec = torch.empty((T, self.ld), device=wave.device, dtype=torch.float32)
            call("nsid_linear_fwd", ops._p(padded), self.hop, ops._p(self.W), ops.F32, None, ops._p(spec), self.ld, T,
                 self.ld, self.n_fft, 1, None, None, ops.ACT_NONE, ops.ACT_NONE, None, 1, ops.F32, s)
        finally:
            ops.set_gemm_precision(prec)
        out = torch.empty((self.n_mels, T), device=wave.device, dtype=torch.float32)
        call("nsid_power_mel_db", ops._p(spec), self.ld, self.n_freq, ops._p(self.fb), ops._p(self.band), self.n_mels, T,
             ops._p(out), s)
        return out

    def __call__(self, wave: torch.Tensor) -> torch.Tensor:
        """(L,) -> (S, n_mels, n_frames); S = 0 rows when the audio is shorter than one segment (the reference's unfold
        raises there and its caller skips the file, transformations.py:101-104)"""
        lm = self.logmel(wave)
        T = lm.shape[1]
        S = (T - self.n_frames) // self.step + 1 if T >= self.n_frames else 0
        out = torch.empty((S, self.n_mels, self.n_frames), device=wave.device, dtype=torch.float32)
        if S > 0:
            call("nsid_unfold_segments", ops._p(lm), self.n_mels, T, self.n_frames, self.step, S, ops._p(out),
                 ops._stream())
        return out


CQT_FMIN, CQT_BINS, CQT_BPO = 32.70, 84, 12          # nnAudio CQT defaults (filter_scale 1, norm 1, Hann)
CQT_GROUP = DEFINES["NSID_CQT_GROUP_BINS"]           # bins per group of the banded kernel: 16 re/im columns of one MFMA tile
CQT_RC = DEFINES["NSID_CQT_RC"]                      # the table pads the hop to a multiple of it


def cqt_kernels(fs: float):
    """nnAudio create_cqt_kernels(Q, fs, fmin 32.70, n_bins 84, bins_per_octave 12, norm 1, window 'hann') restated in fp64:
    -> (freqs (84,), lengths (84,) int, starts (84,) int, width, taps: list of 84 complex128 arrays of l_k entries). Bin k's taps
    occupy [starts[k], starts[k] + lengths[k]) of a zero row of `width` entries."""
    Q = 1.0 / (2.0 ** (1.0 / CQT_BPO) - 1.0)
    freqs = CQT_FMIN * 2.0 ** (np.arange(CQT_BINS, dtype=np.float64) / float(CQT_BPO))
    if freqs.max() > fs / 2:
        raise ValueError(f"The top bin {freqs.max():.2f}Hz has exceeded the Nyquist frequency {fs / 2}Hz")
    lengths = np.ceil(Q * fs / freqs).astype(np.int64)
    width = int(2 ** math.ceil(math.log2(int(lengths.max()))))
    starts, taps = np.zeros(CQT_BINS, dtype=np.int64), []
    for k in range(CQT_BINS):
        l = int(lengths[k])
        starts[k] = int(math.ceil(width / 2.0 - l / 2.0)) - l % 2
        m = np.arange(-(l // 2) - l % 2, l // 2, dtype=np.float64)            # np.r_[-l//2 : l//2] on the float l
        n = np.arange(l, dtype=np.float64)
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / l)                            # periodic Hann
        ph = m * 2.0 * np.pi * freqs[k] / fs
        sig = w * (np.cos(ph) + 1j * np.sin(ph)) / l
        taps.append(sig / np.abs(sig).sum())
    return freqs, lengths, starts, width, taps


class CQTFrontEnd:
    """front = CQTFrontEnd(cfg, device); segs = front(wave)  — wave (L,) fp32 on the GPU, segs (S, 84, n_frames) magnitudes."""

    def __init__(self, cfg: dict, device="cuda"):
        self.fs, self.hop = int(cfg["fs"]), int(cfg["hop_len"])
        self.n_frames = int(cfg["n_frames"])
        self.step = int(self.n_frames * (1 - float(cfg["overlap"])))          # transformations.py:102
        if self.hop < 1:
            raise ValueError("hop_len must be positive")
        self.n_bins = CQT_BINS
        self.device = torch.device(device)
        self.freqs, self.lengths, self.starts, self.width, taps = cqt_kernels(self.fs)
        taps32 = [t.astype(np.complex64) for t in taps]                       # nnAudio stores complex64: one rounding from fp64
        hopP = (self.hop + CQT_RC - 1) // CQT_RC * CQT_RC
        groups, blocks, off = [], [], 0
        for b0 in range(0, self.n_bins, CQT_GROUP):
            nb = min(CQT_GROUP, self.n_bins - b0)
            tap0 = int(min(self.starts[b0:b0 + nb]))
            extent = int(max(self.starts[b0:b0 + nb] + self.lengths[b0:b0 + nb])) - tap0
            Q = (extent - 1) // self.hop + 1
            P = np.zeros((Q * hopP, 2 * CQT_GROUP), dtype=np.float32)         # row q*hopP + r = tap tap0 + q*hop + r
            for j in range(nb):
                n = np.arange(int(self.lengths[b0 + j])) + int(self.starts[b0 + j]) - tap0
                row = n // self.hop * hopP + n % self.hop
                P[row, 2 * j], P[row, 2 * j + 1] = taps32[b0 + j].real, taps32[b0 + j].imag
            blocks.append(P.reshape(-1, 4, 2 * CQT_GROUP).transpose(0, 2, 1).reshape(-1))    # [row/4][column][row%4]
            groups.append((b0, nb, tap0, extent, off))
            off += P.size
        self.groups = np.ascontiguousarray(np.array(groups, dtype=np.int32))  # host: the entry point reads it before the launch
        self.taps = torch.from_numpy(np.concatenate(blocks)).to(self.device)
        self.scale = torch.sqrt(torch.from_numpy(self.lengths.astype(np.float32))).to(self.device)     # fp32 sqrt of float32(l_k)

    def n_frames_of(self, L: int) -> int:
        return 1 + L // self.hop                                             # conv1d with stride hop over L + width samples

    def batch(self, waves: torch.Tensor) -> torch.Tensor:
        """(B, L) fp32 on the GPU -> (B, 84, T) magnitudes in one launch; stream-ordered, no allocation besides the result,
        capture-safe. Clip b of the result is bit-equal to the same clip in a call of its own."""
        return ops.cqt(waves, self.hop, self.width, self.groups, self.taps, self.scale)

    def cqt(self, wave: torch.Tensor) -> torch.Tensor:
        """(L,) fp32 on the GPU -> (84, T) magnitudes"""
        if wave.dim() != 1 or not wave.is_cuda or wave.dtype != torch.float32:
            raise RuntimeError("the front end takes one mono fp32 waveform on the MI355X device")
        return self.batch(wave.contiguous().unsqueeze(0))[0]

    def __call__(self, wave: torch.Tensor) -> torch.Tensor:
        """(L,) -> (S, 84, n_frames); S = 0 rows when the audio is shorter than one segment"""
        spec = self.cqt(wave)
        T = spec.shape[1]
        S = (T - self.n_frames) // self.step + 1 if T >= self.n_frames else 0
        out = torch.empty((S, self.n_bins, self.n_frames), device=wave.device, dtype=torch.float32)
        if S > 0:
            call("nsid_unfold_segments", ops._p(spec), self.n_bins, T, self.n_frames, self.step, S, ops._p(out),
                 ops._stream())
        return out
