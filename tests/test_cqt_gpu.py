"""GPU: the constant-Q front end in one launch (csrc/cqt.hip nsid_cqt, frontend.CQTFrontEnd, modules/transformations.GPUTransformCQT)
against tests/cqt_oracle.py evaluated in fp64 on the CPU inside the test.

Tolerance of a parity case: 4 x the largest deviation of the fp32 oracle from the fp64 oracle on that same input. Both the kernel
and the fp32 oracle are fp32 sums of the same products in different orders, so 4 x leaves room for the order and for the final sqrt.
Every case prints both figures; the measured ones are in docs/experiments.md."""
import numpy as np
import pytest
import torch

from cqt_oracle import CQTOracle, segments

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = {"fs": 22050, "hop_len": 512, "n_frames": 216, "overlap": 0.5, "arch": "resnet-ibn"}
_ORACLES, _FRONTS = {}, {}


def oracle_of(fs=22050, hop=512):
    if (fs, hop) not in _ORACLES:
        _ORACLES[fs, hop] = CQTOracle(fs, hop)
    return _ORACLES[fs, hop]


def front_of(fs=22050, hop=512):
    from neuralsampleid_amd.frontend import CQTFrontEnd
    if (fs, hop) not in _FRONTS:
        _FRONTS[fs, hop] = CQTFrontEnd(dict(CFG, fs=fs, hop_len=hop), DEV)
    return _FRONTS[fs, hop]


def noise(B, L, seed):
    return 0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(seed))


def counters(reset=False):
    from neuralsampleid_amd import _lib
    return _lib.launch_counters(reset=reset)


@pytest.mark.parametrize("fs,hop,B,L", [
    (22050, 512, 3, 9254),        # every frame reflects on the left, all but the first three on the right; L % hop != 0
    (22050, 512, 1, 8193),        # the shortest legal input
    (22050, 512, 2, 110250),      # T = 216: interior frames without reflection, T no multiple of the frame tile
    (22050, 500, 1, 9001),        # hop no power of two: the table pads every hop to 512 rows
    (8000, 256, 2, 5000),         # the other table (width 8192)
], ids=lambda v: str(v))
def test_parity_with_the_fp64_oracle(fs, hop, B, L):
    o, front = oracle_of(fs, hop), front_of(fs, hop)
    x = noise(B, L, 1000 + L)
    ref = o(x, torch.float64)
    tol = 4.0 * float((o(x, torch.float32).double() - ref).abs().max())
    counters(reset=True)
    got = front.batch(x.to(DEV))
    assert counters()["cqt"] == 1
    assert got.shape == ref.shape == (B, 84, 1 + L // hop) and got.dtype == torch.float32
    err = float((got.cpu().double() - ref).abs().max())
    print(f"cqt fs={fs} hop={hop} B={B} L={L}: kernel vs fp64 {err:.3e}, fp32 oracle vs fp64 {tol / 4:.3e} (largest output "
          f"{float(ref.max()):.3f})")
    assert err <= tol, (err, tol)


def test_too_short_input_raises():
    front = front_of()
    with pytest.raises(RuntimeError):
        front.batch(torch.zeros(1, 8192, device=DEV))                         # L <= width/2: torch's reflect pad raises
    with pytest.raises(ValueError):
        oracle_of()(torch.zeros(8192))


def test_unit_impulses_read_the_taps():
    """out[k, t] == |taps_k[p - t hop + width/2]| sqrt(l_k) at 1e-6 relative (tests/test_cqt_cpu.py explains the choice of L and p):
    an off-by-one in start_k for odd or even lengths, or a reflection that duplicates the edge sample, shows here"""
    o, front = oracle_of(), front_of()
    L, W, ps = 20000, 16384, (0, 9216, 19999)
    x = torch.zeros(len(ps), L)
    for b, p in enumerate(ps):
        x[b, p] = 1.0
    got = front.batch(x.to(DEV)).cpu().double().numpy()
    sq = torch.sqrt(torch.from_numpy(o.lengths.astype(np.float32))).double().numpy()
    taps = np.abs(o.taps.astype(np.complex128))
    for b, p in enumerate(ps):
        want = np.zeros((84, 40))
        for t in range(40):
            n = p - t * 512 + W // 2
            if 0 <= n < W:
                want[:, t] = taps[:, n] * sq
        assert (want > 0).any(1).all()                                        # every bin is read, the 94-tap one included
        err = np.abs(got[b] - want)
        assert (err <= 1e-6 * want).all(), (p, float((err / np.maximum(want, 1e-30))[want > 0].max()), float(err[want == 0].max()))


def test_batch_independence_strides_and_one_launch():
    """no atomics, no split that depends on B: clip b of a batch is bit-equal to the clip alone, also through a view with a clip
    stride larger than the clip; one batch() call is one launch"""
    L = 9254
    w = noise(5, L, 7)
    big = torch.full((5, L + 107), float("nan"))
    big[:, 7:7 + L] = w
    view = big.to(DEV)[:, 7:7 + L]
    assert view.stride(0) == L + 107 and not view.is_contiguous()
    front = front_of()
    counters(reset=True)
    a = front.batch(w.to(DEV))
    assert counters()["cqt"] == 1
    assert torch.equal(a, front.batch(w.to(DEV)))
    assert torch.equal(a, front.batch(view))
    for b in range(5):
        assert torch.equal(a[b], front.batch(w[b:b + 1].to(DEV))[0]), b
        assert torch.equal(a[b], front.batch(view[b:b + 1])[0]), b
        assert torch.equal(a[b], front.cqt(w[b].to(DEV))), b
    assert bool(torch.isfinite(a).all())


def test_eval_path_and_module():
    from neuralsampleid_amd.modules.transformations import GPUTransformCQT
    o, front = oracle_of(), front_of()
    L = 110250 + 108 * 512                                                    # T = 324: S = 2 segments of 216 frames, step 108
    w = noise(1, L, 11)[0]
    spec = front.batch(w[None].to(DEV))[0]
    segs = front(w.to(DEV))
    assert segs.shape == (2, 84, 216)
    assert torch.equal(segs, segments(spec, 216, 0.5).contiguous())           # bit-equal to unfolding front.batch
    assert torch.equal(segs[1, :, :108], segs[0, :, 108:])
    assert front(torch.zeros(20000, device=DEV)).shape == (0, 84, 216)        # S = 0 for short audio
    aug = GPUTransformCQT(CFG, train=False)
    for x in (w, w[None], w[None, None]):
        out, none = aug(x.to(DEV), None)
        assert none is None and torch.equal(out, segs)
    X, none = aug(noise(1, 20000, 12).to(DEV), None)                          # the reference's fall-through: un-segmented (T, 84)
    assert none is None and X.shape == (40, 84)
    ref = o(noise(1, 20000, 12), torch.float64)[0].t()
    tol = 4.0 * float((o(noise(1, 20000, 12), torch.float32)[0].t().double() - ref).abs().max())
    assert float((X.cpu().double() - ref).abs().max()) <= tol
    train = GPUTransformCQT(CFG)
    x_i, x_j = noise(2, 9254, 13).to(DEV), noise(2, 9254, 14).to(DEV)
    X_i, X_j = train(x_i, x_j)
    assert X_i.shape == X_j.shape == (2, 84, 19)
    assert torch.equal(X_i, front.batch(x_i)) and torch.equal(X_j, front.batch(x_j))


def test_capture_and_replay():
    """torch.cuda.graph capture of front.batch on one stream, replayed on fresh input: bit-equal to eager"""
    front = front_of()
    static = noise(3, 9254, 21).to(DEV)
    fresh = noise(3, 9254, 22).to(DEV)
    front.batch(static)                                                       # warm-up outside the capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = front.batch(static)
    torch.cuda.current_stream().wait_stream(s)
    static.copy_(fresh)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, front.batch(fresh))


def test_end_to_end_fingerprints_from_a_waveform():
    from synth import synth_state
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    from neuralsampleid_amd.fingerprint import extract_fingerprints, fingerprints_from_waveform
    from neuralsampleid_amd.simclr.triplet import BaselineModel
    F_.set_activation_dtype(torch.float32)
    ops.set_gemm_precision("fp32")
    model = BaselineModel(CFG, ResNetIBN())
    model.load_state_dict(synth_state(model.state_dict()))
    model = model.to(DEV).eval()
    front = front_of()
    w = noise(1, 110250 + 108 * 512, 31)[0].to(DEV)
    with torch.no_grad():
        fp = fingerprints_from_waveform(model, front, w)
        want = extract_fingerprints(model, front(w))
    assert fp.shape == (2, 2048) and torch.equal(fp, want)
    assert float((fp.norm(dim=1) - 1).abs().max()) < 1e-5
    assert bool(torch.isfinite(fp).all()) and not torch.equal(fp[0], fp[1])
