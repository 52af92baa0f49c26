"""Test helper (like compare.py): nnAudio's CQT(sr, hop_length) = CQT1992v2 with its defaults (fmin 32.70, 84 bins, 12 per octave,
filter_scale 1, norm 1, Hann window, center=True, pad_mode 'reflect', magnitude output, normalization_type 'librosa') restated in
numpy / torch on the CPU, with the arithmetic type selectable. No scipy, nothing from the reference tree.

    k = CQTOracle(fs, hop);  k.lengths, k.starts, k.width, k.freqs, k.taps (84, width) complex64
    k(x, torch.float64) -> (B, 84, T)        x (L,) or (B, L)

The taps are evaluated in fp64 and rounded once to complex64 (what nnAudio stores); `dtype` is the type of the correlation, the
sqrt(l_k) scaling (an fp32 sqrt of float32(l_k) in either case) and the magnitude."""
import math

import numpy as np
import torch
import torch.nn.functional as F

FMIN, N_BINS, BPO = 32.70, 84, 12


class CQTOracle:
    def __init__(self, fs, hop):
        self.fs, self.hop = fs, hop
        Q = 1 / (2 ** (1 / BPO) - 1)
        self.freqs = FMIN * 2.0 ** (np.r_[0:N_BINS] / float(BPO))
        if max(self.freqs) > fs / 2:
            raise ValueError("the top bin exceeds the Nyquist frequency")
        self.lengths = np.ceil(Q * fs / self.freqs)                           # fp64
        self.width = int(2 ** np.ceil(np.log2(max(self.lengths))))
        kern = np.zeros((N_BINS, self.width), dtype=np.complex64)
        self.starts = np.zeros(N_BINS, dtype=np.int64)
        for k in range(N_BINS):
            freq, l = self.freqs[k], self.lengths[k]
            start = int(np.ceil(self.width / 2.0 - l / 2.0)) - int(l % 2)
            n = np.arange(int(l), dtype=np.float64)
            window = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / l)                  # periodic Hann
            ph = np.r_[-l // 2:l // 2] * 2.0 * np.pi * freq / fs
            sig = window * (np.cos(ph) + 1j * np.sin(ph)) / l
            kern[k, start:start + int(l)] = sig / np.abs(sig).sum()           # norm 1
            self.starts[k] = start
        self.taps = kern
        self.lengths = self.lengths.astype(np.int64)
        self.scale32 = torch.sqrt(torch.from_numpy(self.lengths.astype(np.float32)))

    def n_frames_of(self, L):
        return 1 + L // self.hop

    def __call__(self, x, dtype=torch.float64):
        x = torch.as_tensor(x)
        if x.dim() == 1:
            x = x[None]
        pad = self.width // 2
        if x.shape[-1] <= pad:
            raise ValueError("input is too short for reflect padding")
        xp = F.pad(x.to(dtype)[:, None, :], (pad, pad), mode="reflect")
        wr = torch.from_numpy(np.ascontiguousarray(self.taps.real)).to(dtype)[:, None, :]
        wi = torch.from_numpy(np.ascontiguousarray(self.taps.imag)).to(dtype)[:, None, :]
        re = F.conv1d(xp, wr, stride=self.hop)
        im = -F.conv1d(xp, wi, stride=self.hop)
        s = self.scale32.to(dtype).view(1, -1, 1)
        re, im = re * s, im * s
        return torch.sqrt(re * re + im * im)


def segments(spec, n_frames, overlap):
    """the evaluation branch (transformations.py:96-105) on one (84, T) spectrogram: (S, 84, n_frames), or the (T, 84) fall-through"""
    X = spec.transpose(1, 0)
    if X.shape[0] < n_frames:
        return X
    return X.unfold(0, size=n_frames, step=int(n_frames * (1 - overlap)))


def tone(fs, f, L, amp=1.0):
    n = torch.arange(L, dtype=torch.float64)
    return (amp * torch.cos(2 * math.pi * f * n / fs)).to(torch.float32)
