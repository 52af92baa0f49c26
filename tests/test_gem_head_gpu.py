"""GPU: ops.gem_pool_bwd and ResNetIBN.head_train (GeM pooling -> embedding head, forward and backward) against fp64 autograd of the
reference's formula (tests/gem_head_oracle.py).

Tolerance: 4 x the distance of torch's own fp32 autograd (CPU) from the fp64 run, per quantity (max abs for tensors), computed here
and printed; the kernels round in other places than torch does. For bf16 rows the references are evaluated on the bf16-rounded
inputs. Negative inputs and inputs below eps get exactly zero gradient."""
import pytest
import torch

import gem_head_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 3


def within(what, got, ref64, ref32):
    floor = float((ref32.double() - ref64).abs().max())
    err = float((got.detach().double().cpu().reshape(ref64.shape) - ref64).abs().max())
    print(f"  {what}: max |kernel - fp64| = {err:.3g}, allowed 4 x {floor:.3g}")
    return err <= 4.0 * floor


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("p", [3.0, 2.3])
@pytest.mark.parametrize("C", [64, 1024])
@pytest.mark.parametrize("HW", [5, 84])
def test_gem_pool_bwd(HW, C, p, bf16):
    from neuralsampleid_amd import ops
    x = G.make_rows(B, HW, C, seed=HW + C, bf16=bf16)
    dy = torch.randn(B, C, generator=torch.Generator().manual_seed(2))
    r64, r32 = G.autograd_reference(x, p, dy, torch.float64), G.autograd_reference(x, p, dy, torch.float32)
    rows = x.reshape(B * HW, C).to(torch.bfloat16 if bf16 else torch.float32).to(DEV)
    pt = torch.tensor([p], device=DEV)
    dx, dp = ops.gem_pool_bwd(rows, dy.to(DEV), B, HW, C, pt, G.EPS)
    assert dx.dtype == torch.float32 and tuple(dx.shape) == (B * HW, C)
    print(f"HW={HW} C={C} p={p} bf16={bf16}")
    ok = [within("dx", dx.view(B, HW, C), r64["dx"], r32["dx"]), within("dp", dp, r64["dp"], r32["dp"])]
    dead = (x <= G.EPS).reshape(B * HW, C)
    assert bool(dead.any()) and float(dx.cpu()[dead].abs().max()) == 0.0
    assert all(ok)
    dx2, dp2 = ops.gem_pool_bwd(rows, dy.to(DEV), B, HW, C, pt, G.EPS)          # two stages, no atomics: bitwise reproducible
    assert torch.equal(dx, dx2) and torch.equal(dp, dp2)


@pytest.fixture(scope="module")
def model():
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    torch.manual_seed(0)
    return ResNetIBN().to(DEV)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("p", [3.0, 2.3])
@pytest.mark.parametrize("HW", [5, 84])
def test_head_train(model, HW, p, bf16):
    C, E = 1024, 2048
    head = model.embedding_head
    with torch.no_grad():
        model.global_pool.p.fill_(p)
    for q in (model.global_pool.p, head.weight, head.bias):
        q.grad = None
    x = G.make_rows(B, HW, C, seed=HW, bf16=bf16)
    dh = torch.randn(B, E, generator=torch.Generator().manual_seed(3)) / 32
    w, b = head.weight.detach().cpu(), head.bias.detach().cpu()
    r64 = G.autograd_reference(x, p, None, torch.float64, w, b, dh)
    r32 = G.autograd_reference(x, p, None, torch.float32, w, b, dh)
    rows = x.reshape(B * HW, C).to(torch.bfloat16 if bf16 else torch.float32).to(DEV).requires_grad_(True)
    h = model.head_train(rows, B, HW)
    assert tuple(h.shape) == (B, E) and h.dtype == torch.float32
    h.backward(dh.to(DEV))
    print(f"HW={HW} p={p} bf16={bf16}")
    # autograd hands a bf16 leaf its gradient in bf16 (its own rule for a gradient of another type): there the fp32 rows of the same
    # two kernels are compared, and the leaf's gradient must be their rounding to bf16
    drows = rows.grad
    if bf16:
        from neuralsampleid_amd import ops
        dpooled = ops.linear_bwd_data(dh.to(DEV), head.weight.detach(), B, E, C)
        drows, _ = ops.gem_pool_bwd(rows.detach(), dpooled, B, HW, C, model.global_pool.p.detach(), G.EPS)
        # bf16 keeps 8 significant bits: rounding moves a value by at most 2^-9 of itself (2^-8 allowed: the backward-data GEMM of
        # so few rows splits its reduction over atomics, so its last bit, and with it a rounding direction, can change between calls)
        assert rows.grad.dtype == torch.bfloat16
        assert bool(((rows.grad.float() - drows).abs() <= drows.abs() * 2.0 ** -8 + 1e-38).all())
    ok = [within("h", h, r64["h"], r32["h"]), within("d rows", drows.view(B, HW, C), r64["dx"], r32["dx"]),
          within("d p", model.global_pool.p.grad, r64["dp"], r32["dp"]), within("d weight", head.weight.grad, r64["dw"], r32["dw"]),
          within("d bias", head.bias.grad, r64["db"], r32["db"])]
    dead = (x <= G.EPS).reshape(B * HW, C)
    assert float(drows.cpu()[dead].abs().max()) == 0.0
    assert all(ok)
