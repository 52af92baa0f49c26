"""CPU: the shells around the batched log-mel front end (csrc/frontend.hip, nsid_logmel_fft): the binding, the host-side tables
of LogMelFrontEnd(stft="fft"), and the module train.py constructs (modules/transformations.GPUTransformSampleID). No GPU."""
import inspect
import math

import pytest
import torch

CFG = {"fs": 16000, "n_fft": 1024, "win_len": 1024, "hop_len": 512, "n_mels": 64, "n_frames": 128, "overlap": 0.875,
       "arch": "grafp"}


def test_entry_point_is_bound_and_counted():
    from neuralsampleid_amd import _lib
    assert _lib.SIGNATURES["nsid_logmel_fft"] == "pliliippppiplls"
    assert hasattr(_lib.lib, "nsid_logmel_fft")
    assert _lib.launch_counters()["logmel_fft"] == 0
    # bad arguments are refused on the host before any launch: NSID_EINVAL = -1, and nothing is counted
    assert _lib.lib.nsid_logmel_fft(None, 0, 1, 65280, 1024, 512, None, None, None, None, 64, None, 0, 0, None) == -1
    assert _lib.launch_counters()["logmel_fft"] == 0


def test_module_shell_keeps_the_reference_signature():
    from neuralsampleid_amd.modules.transformations import GPUTransformSampleID
    sig = inspect.signature(GPUTransformSampleID.__init__)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("self", inspect.Parameter.empty), ("cfg", inspect.Parameter.empty), ("ir_dir", None), ("train", True), ("cpu", False),
        ("max_transforms_1", 1), ("max_transforms_2", 1)]
    assert list(inspect.signature(GPUTransformSampleID.forward).parameters) == ["self", "x_i", "x_j"]
    m = GPUTransformSampleID(CFG, ir_dir="irs", train=False)
    assert m.train is False and m.ir_dir == "irs" and m.n_frames == 128 and m.overlap == 0.875 and m.sample_rate == 16000
    assert list(m.parameters()) == [] and list(m.buffers()) == [] and m.state_dict() == {}


def test_module_refuses_what_stays_with_the_reference():
    from neuralsampleid_amd.modules.transformations import GPUTransformSampleID
    with pytest.raises(NotImplementedError, match="audiomentations"):
        GPUTransformSampleID(CFG, cpu=True)
    with pytest.raises(NotImplementedError, match="resnet-ibn"):
        GPUTransformSampleID(dict(CFG, arch="resnet-ibn"))
    with pytest.raises(ValueError):
        GPUTransformSampleID(dict(CFG, arch="something-else"))


def test_fft_tables_on_the_host():
    from neuralsampleid_amd.frontend import LogMelFrontEnd
    front = LogMelFrontEnd(CFG, "cpu", stft="fft")
    assert front.stft == "fft" and front.W is None
    tw = front.twiddle
    assert tw.shape == (1024, 2) and tw.dtype == torch.float32 and tw.is_contiguous()
    j = torch.arange(1024, dtype=torch.float64)
    want = torch.stack((torch.cos(-2 * math.pi * j / 1024), torch.sin(-2 * math.pi * j / 1024)), 1)
    # <= 1 ulp of fp32 at the value's own magnitude (entries within rounding of zero: 1 ulp of the smallest normal step taken there)
    ulp = torch.maximum(2.0 ** (torch.floor(torch.log2(want.abs().clamp_min(1e-30))) - 23), torch.tensor(1e-16, dtype=torch.float64))
    assert bool(((tw.double() - want).abs() <= ulp).all())
    assert float(tw[0, 0]) == 1.0 and float(tw[0, 1]) == 0.0 and float(tw[256, 1]) == -1.0 and float(tw[512, 0]) == -1.0
    win = torch.hann_window(1024, periodic=True, dtype=torch.float64)
    assert float((front.window.double() - win).abs().max()) <= 2.0 ** -24
    assert front.fb.shape == (64, 513) and front.band.shape == (64, 2) and front.band.dtype == torch.int32
    # hop_len need not be a multiple of 4 here (that is the GEMM path's 16-byte rows)
    assert LogMelFrontEnd(dict(CFG, hop_len=510), "cpu", stft="fft").n_frames_of(65280) == 129
    with pytest.raises(NotImplementedError):
        LogMelFrontEnd(dict(CFG, hop_len=510), "cpu")
    with pytest.raises(NotImplementedError):
        LogMelFrontEnd(dict(CFG, n_fft=512, win_len=512), "cpu", stft="fft")           # refused, not computed some other way


def test_stft_mode_is_checked_and_defaults_to_gemm():
    from neuralsampleid_amd.frontend import LogMelFrontEnd
    assert inspect.signature(LogMelFrontEnd.__init__).parameters["stft"].default == "gemm"
    front = LogMelFrontEnd(CFG, "cpu")
    assert front.stft == "gemm" and front.W.shape == (1028, 1024)
    for bad in ("FFT", "", "dft", None):
        with pytest.raises(ValueError):
            LogMelFrontEnd(CFG, "cpu", stft=bad)


def test_batch_refuses_host_tensors():
    from neuralsampleid_amd.frontend import LogMelFrontEnd
    front = LogMelFrontEnd(CFG, "cpu", stft="fft")
    with pytest.raises(RuntimeError):
        front.batch(torch.zeros(2, 65280))


def test_graphed_step_takes_a_front_end():
    from neuralsampleid_amd.graphs import GraphedTrainStep
    assert inspect.signature(GraphedTrainStep.__init__).parameters["front"].default is None
