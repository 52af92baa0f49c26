"""GPU: the training-mode stem of the ResNet-IBN baseline (csrc/resnet.hip: nsid_stem7_stat, nsid_stem7_pool_train_fwd, nsid_stem7_bwd;
ResNetIBN.stem_train) against the fp64 oracle of tests/stem_train_oracle.py.

Shapes (B, H, W): (3, 37, 70) two column tiles, a ragged second, odd edges; (2, 21, 130) three column tiles; (1, 84, 65) the model's
84 bins; (3, 1, 1) one conv pixel per clip (N = 3); (2, 84, 216), the model's segment, once (fp32 storage).

Forward: the rows within 20 x the oracle's own fp32-vs-fp64 distance under fp32 storage (MULT of test_resnet_train_gpu.py), within 4 x
the distance of the bf16-rounded fp32 oracle under bf16 storage. bn1's running statistics never pass through bf16 (the conv is
recomputed in fp32 registers), so they have the fp32 bound under both storages; the counter is 1.

Backward: the upstream gradient is synth_randn, rounded to bf16 on both sides under bf16 storage, and ZERO at the entries of
stem_band(pre64, 1e-4) (at most 1e-3 of them: tests/test_stem_train_cpu.py holds that condition and that torch's fp32 run then
picks the fp64 winners): those entries add nothing on either side whichever way rounding decides them, so no mask is forced.
dW, dgamma, dbeta each within 20 x the fp32 oracle's distance from fp64, under both storages (the backward computes in fp32 from the
fp32 input whatever the rows' storage). Every multiple is printed; DESIGN.md 3a records them.

Also: a second run gives the same bits (no atomics); the last clip alone, handed the batch's affine, gives the rows it has inside the
batch; the launch counters stem7_stat, stem7_pool_train and stem7_bwd move once per call."""
import functools

import pytest
import torch

import stem_train_oracle as S
from compare import relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MULT = {torch.float32: 20.0, torch.bfloat16: 4.0}
MULT_BWD = 20.0
CASES = [(shape, dt) for shape in S.SHAPES for dt in (torch.float32, torch.bfloat16)] + [((2, 84, 216), torch.float32)]


@pytest.fixture
def restore():
    from neuralsampleid_amd import functional as F_
    yield
    F_.set_activation_dtype(torch.float32)


@functools.lru_cache(maxsize=None)
def _oracle(shape, bf):
    """(x, dy, ref64, ref32, emulated rows or None, share of the upstream gradient zeroed); computed once per (shape, rounding)"""
    from synth import synth_randn
    B, H, W = shape
    sd, x = S.stem_state(), S.stem_input(B, H, W)
    with torch.no_grad():
        f64 = S.stem_forward(x.double(), {k: v.double() for k, v in sd.items()})
    band = S.stem_band(f64["pre"], S.BAND_THR)
    dy = synth_randn(f"stem_train_d_{B}x{H}x{W}", *f64["y"].shape)
    if bf:
        dy = dy.to(torch.bfloat16).float()
    dy = dy * (~band).float()
    ref64 = S.stem_reference(x, sd, dy, torch.float64)
    ref32 = S.stem_reference(x, sd, dy, torch.float32)
    return x, dy, ref64, ref32, float(band.double().mean())


def _rows(x4, dt):
    b, c, h, w = x4.shape
    return x4.permute(0, 2, 3, 1).reshape(b * h * w, c).to(dt).contiguous()


def _bchw(rows, b, h, w):
    return rows.detach().double().view(b, h, w, -1).permute(0, 3, 1, 2).cpu()


def _model():
    from synth import synth_state
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    model = ResNetIBN()
    model.load_state_dict(synth_state(model.state_dict()))
    return model.to(DEV).train()


def _run(model, x, dy, dt):
    rows, Hp, Wp = model.stem_train(x.to(DEV))
    rows.backward(_rows(dy, dt).to(DEV))
    return rows.detach(), Hp, Wp, [model.conv1.weight.grad.clone(), model.bn1.weight.grad.clone(), model.bn1.bias.grad.clone()]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-%s" % (*c[0], "bf16" if c[1] == torch.bfloat16 else "fp32"))
def test_stem_train_vs_oracle(case, restore):
    from neuralsampleid_amd import _lib, ops
    from neuralsampleid_amd import functional as F_
    shape, dt = case
    B, H, W = shape
    bf = dt == torch.bfloat16
    F_.set_activation_dtype(dt)
    x, dy, ref64, ref32, share = _oracle(shape, bf)
    print(f"stem {shape} {dt}: {share:.2e} of the upstream gradient zeroed (band)")
    assert share <= S.BAND_CAP
    model = _model()
    before = _lib.launch_counters()
    rows, Hp, Wp, grads = _run(model, x, dy, dt)
    after = _lib.launch_counters()
    for k in ("stem7_stat", "stem7_pool_train", "stem7_bwd"):
        assert after[k] == before[k] + 1, k
    assert after["stem7_pool"] == before["stem7_pool"]
    assert rows.dtype == dt and tuple(rows.shape) == (B * Hp * Wp, 64) and tuple(ref64["y"].shape) == (B, 64, Hp, Wp)
    bad = []

    def one(name, a, r, f, mult):
        err, floor = relerr(a, r), relerr(f, r)
        m = err / max(floor, 1e-30)
        print(f"  {name}: rel {err:.3e} = {m:.2f} x the floor {floor:.3e} (allowed {mult:g} x)")
        if not err <= mult * floor:
            bad.append((name, err, floor))

    # forward
    y_floor = ref32["y"].to(torch.bfloat16).double() if bf else ref32["y"].double()
    one("rows", _bchw(rows, B, Hp, Wp), ref64["y"], y_floor, MULT[dt])
    for k in ("bn1.running_mean", "bn1.running_var"):
        one(k, model.state_dict()[k].double().cpu(), ref64["running"][k], ref32["running"][k].double(), MULT[torch.float32])
    assert int(model.bn1.num_batches_tracked) == 1
    # backward
    for name, g in zip(("conv1.weight", "bn1.weight", "bn1.bias"), grads):
        assert g.dtype == torch.float32 and g.shape == ref64["grads"][name].shape
        one("grad." + name, g.double().cpu(), ref64["grads"][name], ref32["grads"][name].double(), MULT_BWD)
    assert not bad, bad
    # a second model with the same state: the same bits everywhere
    model2 = _model()
    rows2, _, _, grads2 = _run(model2, x, dy, dt)
    assert torch.equal(rows2, rows) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    for k in ("bn1.running_mean", "bn1.running_var"):
        assert torch.equal(model2.state_dict()[k], model.state_dict()[k]), k
    # the last clip alone with the batch's affine: its rows inside the batch
    xd, w49 = x.to(DEV), ops.w2d(model2.conv1.weight.detach())
    stat, tiles, N = ops.stem7_stat(xd, w49)
    assert N == B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) and tuple(stat.shape) == (2, tiles, 64)
    aff = ops.bn_finalize(stat, N, model2.bn1.weight.detach(), model2.bn1.bias.detach(), None, None, None, tiles=tiles)
    last, _, _ = ops.stem7_pool_train_fwd(xd[B - 1:].contiguous(), w49, aff, dt)
    assert torch.equal(last, rows[(B - 1) * Hp * Wp:])
    # the op by itself writes its outputs (nothing accumulated), twice the same
    d1 = ops.stem7_bwd(_rows(dy, dt).to(DEV), xd, w49, aff, model2.bn1.weight.detach())
    d2 = ops.stem7_bwd(_rows(dy, dt).to(DEV), xd, w49, aff, model2.bn1.weight.detach())
    assert all(torch.equal(a, b) for a, b in zip(d1, d2))
    assert torch.equal(d1[0].view(64, 1, 7, 7), grads[0]) and torch.equal(d1[1], grads[1]) and torch.equal(d1[2], grads[2])


def test_stem_ops_refuse_wrong_shapes():
    from neuralsampleid_amd import ops
    x, w, f = torch.zeros(2, 9, 6, device=DEV), torch.zeros(64, 49, device=DEV), torch.zeros(64, device=DEV)
    aff = ops.BNAffine(f, f, f, f)
    with pytest.raises(ValueError):
        ops.stem7_stat(x, torch.zeros(64, 9, device=DEV))
    with pytest.raises(ValueError):
        ops.stem7_bwd(torch.zeros(5, 64, device=DEV), x, w, aff, f)
    # nsid_bn_finalize takes nsid_row_tiles(M) or a stem7_stat count (at most 1024), nothing else
    with pytest.raises(RuntimeError, match="NSID_EINVAL"):
        ops.bn_finalize(torch.zeros(2, 2000, 64, device=DEV), 15, f + 1, f, None, None, None, tiles=2000)
