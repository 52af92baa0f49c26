"""GPUTransformSampleID (the reference's modules/transformations.py) on the MI355X: the module train.py:100 and :146
construct and train.py:58 / test_fp.py call as `augment`.

    train=True    forward(x_i, x_j) -> (X_i, X_j), each (B, n_mels, T): MelSpectrogram + AmplitudeToDB of both waveform
                  batches, one launch each (frontend.LogMelFrontEnd.batch, csrc/frontend.hip)
    train=False   forward(x, None)  -> (segments (S, n_mels, n_frames), None) for one waveform given as (L,), (1, L) or
                  (1, 1, L); audio shorter than one segment comes back as the un-segmented (T, n_mels) matrix, the
                  reference's fall-through when unfold raises (transformations.py:101-104): callers test that shape.

The waveform augmentations (Gain, PitchShift, TimeStretch through audiomentations) run on DataLoader workers in the
reference (`cpu=True`); that branch is host DSP and stays the reference's own. The module has no parameters and no buffers:
nothing of it is ever saved.

GPUTransformCQT is the same module for arch 'resnet-ibn' (transformations.py:36,48: nnAudio CQT(sr=fs, hop_length=hop_len)
instead of the log-mel pair): (B, 84, T) magnitudes in training, (S, 84, n_frames) segments or the (T, 84) fall-through in
evaluation, through frontend.CQTFrontEnd (csrc/cqt.hip). It is a class of its own so that GPUTransformSampleID keeps refusing
the arch: at baseline/run_eval.py:241 substitute GPUTransformCQT(cfg, train=False) for GPUTransformSampleID(cfg, train=False)."""
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
                                      "reference's GPUTransformSampleID(cpu=True) for it; this module is the GPU spectrogram half")
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
