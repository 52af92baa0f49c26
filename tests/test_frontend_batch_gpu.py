"""GPU: the batched log-mel front end in one launch (csrc/frontend.hip nsid_logmel_fft, LogMelFrontEnd.batch / stft="fft"), the
module train.py constructs (modules/transformations.GPUTransformSampleID) and the captured training step from waveforms
(graphs.GraphedTrainStep(front=...)), against the oracle restatement of the reference's torchaudio pipeline.

The dB bound is the project's own (tests/test_frontend_gpu.py): 2e-3 dB on every bin. On these inputs the fp32 oracle is 2.6e-5 dB
from an fp64 evaluation of the same formulas and an fp32 DFT-by-matmul 7e-5 dB, so the bound has 30x headroom over fp32 noise.
Measured on an MI355X (docs/experiments.md): fused kernel vs oracle 2.5e-5 .. 3.1e-5 dB on the tonal inputs, 6.7e-6 dB on white noise,
4.4e-5 dB worst of 256 clips, 2.1e-5 dB at hop 510; the GEMM path 5.2e-5 dB on the 8.7 s clip (the two modes 5.2e-5 dB apart);
captured step from waveforms vs from mels: |dloss| 2.4e-7, mean |dp|/lr 2.1e-6, BatchNorm buffers 0."""
import math

import pytest
import torch

from oracle import ref_frontend
from compare import maxerr
from synth import GRAFP_CFG, synth_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = {"fs": 16000, "n_fft": 1024, "win_len": 1024, "hop_len": 512, "n_mels": 64, "n_frames": 128, "overlap": 0.875,
       "arch": "grafp"}
TOL_DB = 2e-3
L_TRAIN = 65280                                       # 4.08 s at 16 kHz (grafp.yaml): T = 128


def wave_n(n, seed):
    """tests/test_frontend_gpu.py::wave at an exact length: tones + 0.05 noise + edge taper"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / CFG["fs"]
    x = 0.3 * torch.sin(2 * math.pi * 440.0 * t) + 0.1 * torch.sin(2 * math.pi * 3100.0 * t * (1 + 0.05 * t))
    x = x + 0.05 * torch.randn(n, generator=g)
    return (x * torch.hann_window(n, periodic=False).clamp_min(0.05)).float()


def noise_n(n, seed):
    return 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(seed))


def front_of(stft="fft", **over):
    from neuralsampleid_amd.frontend import LogMelFrontEnd
    return LogMelFrontEnd(dict(CFG, **over), DEV, stft=stft)


def counters(reset=False):
    from neuralsampleid_amd import _lib
    return _lib.launch_counters(reset=reset)


@pytest.mark.parametrize("L,kind", [(65280, "wave"), (65281, "wave"), (70001, "wave"), (80000, "wave"), (65280, "noise")])
def test_parity_with_the_oracle(L, kind):
    """every bin within 2e-3 dB; the reflected frames (first two, last two) asserted on their own; L odd and L % hop != 0"""
    w = wave_n(L, 3) if kind == "wave" else noise_n(L, 4)
    front = front_of()
    lm = front.batch(w.unsqueeze(0).to(DEV))[0].cpu()
    ref = ref_frontend.logmel(w, CFG)
    assert lm.shape == ref.shape == (64, 1 + L // 512)
    err = (lm - ref).abs()
    edge = max(float(err[:, :2].max()), float(err[:, -2:].max()))
    print(f"fft vs oracle, {kind} L={L}: max {float(err.max()):.3e} dB, reflected frames {edge:.3e} dB")
    assert edge < TOL_DB, edge
    assert float(err.max()) < TOL_DB, float(err.max())


@pytest.mark.parametrize("B", [1, 3, 256])
def test_batches_match_the_oracle_per_clip(B):
    w = torch.stack([wave_n(L_TRAIN, 10 + b) if b % 2 == 0 else noise_n(L_TRAIN, 10 + b) for b in range(B)])
    lm = front_of().batch(w.to(DEV)).cpu()
    assert lm.shape == (B, 64, 128)
    worst = max(float((lm[b] - ref_frontend.logmel(w[b], CFG)).abs().max()) for b in range(B))
    print(f"batch {B}: max {worst:.3e} dB")
    assert worst < TOL_DB, worst


def test_hop_that_the_gemm_path_refuses():
    """hop = 510 (hop % 4 != 0): T = 1 + L // 510 against the oracle"""
    cfg = dict(CFG, hop_len=510)
    w = wave_n(70001, 5)
    lm = front_of(hop_len=510).batch(w.unsqueeze(0).to(DEV))[0].cpu()
    ref = ref_frontend.logmel(w, cfg)
    assert lm.shape == ref.shape == (64, 1 + 70001 // 510)
    err = float((lm - ref).abs().max())
    print(f"hop 510: max {err:.3e} dB")
    assert err < TOL_DB, err
    with pytest.raises(NotImplementedError):
        front_of("gemm", hop_len=510)


def test_other_transform_sizes_are_refused_cleanly():
    """n_fft = 512: refused at construction, and by the entry point itself with NSID_EINVAL before any launch"""
    from neuralsampleid_amd import ops
    with pytest.raises(NotImplementedError):
        front_of(n_fft=512, win_len=512)
    front = front_of()
    w = torch.zeros(2, 40000, device=DEV)
    counters(reset=True)
    with pytest.raises(RuntimeError, match="NSID_EINVAL"):
        ops.logmel_fft(w, 512, 256, front.window, front.twiddle, front.fb, front.band)
    with pytest.raises(RuntimeError, match="NSID_EINVAL"):
        ops.logmel_fft(w, 1024, 1025, front.window, front.twiddle, front.fb, front.band)      # hop > n_fft
    torch.cuda.synchronize()
    assert counters()["logmel_fft"] == 0


def test_silence_short_audio_and_bad_inputs():
    front = front_of()
    lm = front.batch(torch.zeros(3, 40000, device=DEV))
    assert lm.shape == (3, 64, 79) and float((lm + 100.0).abs().max()) < 1e-4           # clamp(1e-10) -> -100 dB
    with pytest.raises(RuntimeError):
        front.batch(torch.zeros(2, 40000))                                              # host tensor
    with pytest.raises(RuntimeError):
        front.batch(torch.zeros(2, 40000, device=DEV, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        front.batch(torch.zeros(40000, 2, device=DEV).t())                              # last dimension not contiguous
    with pytest.raises(RuntimeError):
        front.batch(torch.zeros(2, 512, device=DEV))                                    # L <= n_fft/2: torch's reflect pad raises
    assert front.batch(torch.zeros(1, 513, device=DEV)).shape == (1, 64, 2)


def test_clip_stride_larger_than_the_clip():
    """a view into a longer buffer (clip stride L + 107, first sample at an odd offset)"""
    L = 65281
    w = torch.stack([wave_n(L, 20), noise_n(L, 21), wave_n(L, 22)])
    big = torch.full((3, L + 107), float("nan"))
    big[:, 7:7 + L] = w
    view = big.to(DEV)[:, 7:7 + L]
    assert view.stride(0) == L + 107 and not view.is_contiguous()
    front = front_of()
    a = front.batch(view)
    assert torch.equal(a, front.batch(w.to(DEV)))
    assert float((a[1].cpu() - ref_frontend.logmel(w[1], CFG)).abs().max()) < TOL_DB


def test_batch_independence_and_determinism():
    """no atomics: clip b of a batch is bit-equal to the clip alone, to logmel() under stft='fft', and between runs"""
    w = torch.stack([wave_n(70001, 30 + b) for b in range(5)]).to(DEV)
    front = front_of()
    a = front.batch(w)
    assert torch.equal(a, front.batch(w))
    for b in range(5):
        assert torch.equal(a[b], front.batch(w[b:b + 1])[0]), b
        assert torch.equal(a[b], front.logmel(w[b])), b


def test_the_two_modes_agree():
    w = wave_n(int(8.7 * 16000), 1)
    fft, gemm = front_of("fft"), front_of("gemm")
    a, g = fft.logmel(w.to(DEV)).cpu(), gemm.logmel(w.to(DEV)).cpu()
    ref = ref_frontend.logmel(w, CFG)
    print(f"fft vs gemm {float((a - g).abs().max()):.3e} dB; fft vs oracle {float((a - ref).abs().max()):.3e} dB; "
          f"gemm vs oracle {float((g - ref).abs().max()):.3e} dB")
    assert float((a - g).abs().max()) < TOL_DB
    segs = fft(w.to(DEV)).cpu()
    rsegs = ref_frontend.segments(w, CFG)
    assert segs.shape == rsegs.shape and segs.shape[0] > 1 and segs.shape[1:] == (64, 128)
    assert float((segs - rsegs).abs().max()) < TOL_DB
    assert torch.equal(segs[1, :, :112], segs[0, :, 16:])                               # hop of 16 frames between segments
    assert fft(torch.zeros(20000, device=DEV)).shape == (0, 64, 128)


def test_the_new_kernel_is_what_ran():
    """one launch per batch() call and none of the GEMM path's three; the default mode never reaches the new kernel"""
    w = wave_n(L_TRAIN, 40).to(DEV)
    fft, gemm = front_of("fft"), front_of("gemm")
    old = ("gemm_fwd", "ws_fwd", "gemm256")
    counters(reset=True)
    fft.batch(w.unsqueeze(0).repeat(4, 1))
    c = counters()
    assert c["logmel_fft"] == 1 and all(c[k] == 0 for k in old), c
    fft.logmel(w)
    fft(w)
    c = counters(reset=True)
    assert c["logmel_fft"] == 3 and all(c[k] == 0 for k in old), c
    gemm.logmel(w)
    gemm(w)
    c = counters(reset=True)
    assert c["logmel_fft"] == 0 and c["gemm_fwd"] + c["ws_fwd"] + c["gemm256"] == 2, c                               # no existing behaviour changes


def test_module_train_branch():
    from neuralsampleid_amd.modules.transformations import GPUTransformSampleID
    aug = GPUTransformSampleID(CFG)
    x_i = torch.stack([wave_n(L_TRAIN, 50 + b) for b in range(3)])
    x_j = torch.stack([noise_n(L_TRAIN, 60 + b) for b in range(3)])
    counters(reset=True)
    with torch.no_grad():
        X_i, X_j = aug(x_i.to(DEV), x_j.to(DEV))
    assert counters()["logmel_fft"] == 2
    assert X_i.shape == X_j.shape == (3, 64, 128)
    for b in range(3):
        assert float((X_i[b].cpu() - ref_frontend.logmel(x_i[b], CFG)).abs().max()) < TOL_DB
        assert float((X_j[b].cpu() - ref_frontend.logmel(x_j[b], CFG)).abs().max()) < TOL_DB


@pytest.mark.parametrize("shape", ["L", "1L", "11L"])
def test_module_eval_branch(shape):
    from neuralsampleid_amd.modules.transformations import GPUTransformSampleID
    aug = GPUTransformSampleID(CFG, train=False)
    w = wave_n(int(8.7 * 16000), 2)
    x = {"L": w, "1L": w[None], "11L": w[None, None]}[shape].to(DEV)
    segs, none = aug(x, None)
    ref = ref_frontend.segments(w, CFG)
    assert none is None and segs.shape == ref.shape
    assert float((segs.cpu() - ref).abs().max()) < TOL_DB
    # audio shorter than one segment: the reference's unfold raises and the un-segmented (T, n_mels) matrix comes back
    short = wave_n(20000, 3)
    X, none = aug(short[None].to(DEV), None)
    assert none is None and X.shape == (40, 64)
    assert float((X.cpu() - ref_frontend.logmel(short, CFG).t()).abs().max()) < TOL_DB


# ---- the captured step from waveforms
GRAPH_TOL = {"loss": 2e-6, "dp": 6e-6, "bn": 1e-7}          # tests/test_e2e_gpu.py::test_graphed_train_step_equals_eager


def build_model(k):
    from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
    from neuralsampleid_amd.simclr.simclr import SimCLR
    m = SimCLR(GRAFP_CFG, GraphEncoder(GRAFP_CFG, in_channels=GRAFP_CFG["n_filters"], k=k, size="t"))
    m.load_state_dict(synth_state(m.state_dict(), ""))
    return m.to(DEV)


def wave_pairs(B):
    w_i = torch.stack([wave_n(L_TRAIN, 100 + b) * (0.5 + 0.1 * (b % 7)) for b in range(B)])
    w_j = torch.stack([w_i[b] + noise_n(L_TRAIN, 200 + b) * 0.3 for b in range(B)])
    return w_i.to(DEV), w_j.to(DEV)


def test_graphed_step_from_waveforms_equals_the_step_from_mels():
    """single steps from equal states S0, S1, S2 (not trajectories: chaotic at B = 16, see test_graphed_train_step_equals_eager):
    GraphedTrainStep(front=front) on waveforms against front.batch followed by today's GraphedTrainStep on the resulting mels.
    Both sides see bit-equal mels, so only the order of atomics differs."""
    from neuralsampleid_amd.graphs import GraphedTrainStep
    from neuralsampleid_amd.optim import FusedClipAdam
    from neuralsampleid_amd.simclr.ntxent import ntxent_loss
    from neuralsampleid_amd import ops
    w_i, w_j = wave_pairs(16)
    front = front_of()
    lr = 8e-5

    def state(model, opt):
        return ([t.clone() for t in (opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.step_count)], [b.clone() for b in model.buffers()])

    def load(model, opt, st):
        with torch.no_grad():
            for dst, src in zip((opt.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.step_count), st[0]):
                dst.copy_(src)
            for b, v in zip(model.buffers(), st[1]):
                b.copy_(v)
        ops.bump_state_epoch()

    m1, m2 = build_model(3).train(), build_model(3).train()
    o1, o2 = FusedClipAdam(m1.parameters(), lr=lr), FusedClipAdam(m2.parameters(), lr=lr)
    p0 = o1.flat_p.clone()
    from_mel = GraphedTrainStep(m1, o1, GRAFP_CFG, front.batch(w_i), front.batch(w_j), loss_fn=ntxent_loss, warmup=1)
    from_wave = GraphedTrainStep(m2, o2, GRAFP_CFG, w_i, w_j, loss_fn=ntxent_loss, warmup=1, front=front)
    assert int(o2.step_count) == 0 and torch.equal(o2.flat_p, p0) and torch.equal(o1.flat_p, p0)   # construction restored the state
    worst_loss = worst_dp = worst_bn = 0.0
    for s_ in range(3):
        st = state(m1, o1)
        load(m2, o2, st)
        a_i, a_j = w_i.roll(s_, 0), w_j.roll(s_, 0)
        counters(reset=True)
        want = float(from_mel(front.batch(a_i), front.batch(a_j)))
        got = float(from_wave(a_i, a_j))
        torch.cuda.synchronize()
        assert math.isfinite(want) and int(o1.step_count) == int(o2.step_count) == s_ + 1
        worst_loss = max(worst_loss, abs(got - want))
        worst_dp = max(worst_dp, float((o2.flat_p - o1.flat_p).abs().mean()) / lr)
        worst_bn = max(worst_bn, max(maxerr(b.double(), v.double()) / max(1.0, float(v.double().abs().max()))
                                     for b, v in zip(m2.buffers(), m1.buffers())))
    print(f"graphed from waveforms vs graphed from mels, per state: |dloss| {worst_loss:.2e}, mean |dp|/lr {worst_dp:.3e}, "
          f"BN buffers {worst_bn:.2e}")
    assert worst_loss < GRAPH_TOL["loss"] and worst_dp < GRAPH_TOL["dp"] and worst_bn < GRAPH_TOL["bn"]


def test_graphed_step_from_waveforms_skips_a_batch_with_a_constant_clip():
    """an all-zero waveform is a constant -100 dB clip, which peak_extractor.py:48 turns into NaN: train.py:65-68 skips the batch"""
    from neuralsampleid_amd.graphs import GraphedTrainStep
    from neuralsampleid_amd.optim import FusedClipAdam
    from neuralsampleid_amd.simclr.ntxent import ntxent_loss
    w_i, w_j = wave_pairs(4)
    model = build_model(3).train()
    opt = FusedClipAdam(model.parameters(), lr=8e-5, max_norm=1.0)
    step = GraphedTrainStep(model, opt, GRAFP_CFG, w_i, w_j, loss_fn=ntxent_loss, warmup=1, front=front_of())
    before = opt.flat_p.clone()
    bad = w_i.clone()
    bad[1] = 0.0
    loss = step(bad, w_j)
    torch.cuda.synchronize()
    assert torch.isnan(loss)
    assert torch.equal(opt.flat_p, before) and int(opt.step_count) == 0
    loss = step(w_i, w_j)                                                                # the next good batch trains
    torch.cuda.synchronize()
    assert math.isfinite(float(loss)) and int(opt.step_count) == 1 and not torch.equal(opt.flat_p, before)
