"""GPU: the backward kernels of the ResNet-IBN residual blocks (csrc/resnet.hip): ops.conv2d_bwd_data, ops.conv2d_bwd_weight,
ops.col_stat and ops.ibn_relu_bwd against fp64.

Convolutions: fp64 autograd of F.conv2d on the storage-rounded operands, the project's kernel bounds (relative L2 2e-6 fp32, 1e-2 bf16).
IBN + ReLU: the closed form of tests/resnet_train_oracle.py in fp64 on the stored r with the kernel's own ReLU mask; bound 4 x the
distance of the same formula in torch fp32 from fp64, per quantity (max abs, as in tests/test_gem_head_gpu.py). Under fp32 storage
that is the bound of every quantity, with nothing added. Under bf16 storage two things cannot meet an fp32-sized floor, and only
there the floor is taken differently (every use is printed with the numbers that need it):
  dr       is a bf16 tensor, whose rounding alone (2^-9 of a value, 3e-2 at |dr| = 8) is four orders above any fp32 distance
           (1.7e-6 ... 2.5e-6 measured): the fp32 formula's dr is rounded to bf16 as well before its distance is taken.
  dgamma, dbeta   are fp32 sums of bf16-representable values, which torch's pairwise fp32 sum gets exact or within 1/8 ulp
           (measured: floor 0 for dbeta IN at C = 128, 11 x 27, and 2.38e-7 for dbeta BN against a kernel error of 1.91e-6 = one unit
           in the last place of a sum of magnitude 17; that one case is the only use in this file's runs): the floor is not taken below half a unit in the last place of fp32 at the
           quantity's largest magnitude, 2^-24 max |ref|.
The BatchNorm half's statistics are an INPUT of nsid_ibn_relu_bwd (as its affine is of the forward in that file's test): in
test_ibn_relu_bwd_vs_closed_form they are taken from the stored r in fp64 and rounded to fp32.
test_ibn_relu_bwd_on_fp32_sum_statistics runs the same kernel on the statistics the block really uses (ops.col_stat ->
ops.bn_finalize: E[x^2] - E[x]^2 from fp32 sums, the layout every BatchNorm of this library uses), whose variance loses its low digits
to cancellation at these offsets of up to twenty standard deviations, and bounds what that costs."""
import pytest
import torch

import resnet_train_oracle as O
from compare import relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = torch.nn.functional
TOL = {torch.float32: 2e-6, torch.bfloat16: 1e-2}
BS = [1, 3, 8]
# (C, Cout, ksize, stride) as in tests/test_resnet_ibn_gpu.py::CONV_PAIRS, each with the input map it meets in the model
CONV_PAIRS = [(128, 128, 3, 1), (256, 256, 3, 1), (256, 256, 1, 1), (512, 512, 3, 2), (512, 512, 3, 1), (1024, 1024, 3, 2),
              (1024, 1024, 3, 1), (128, 128, 1, 1), (512, 512, 1, 1), (1024, 1024, 1, 1), (256, 512, 1, 2), (512, 1024, 1, 2)]
MODEL_MAP = [(21, 54), (21, 54), (21, 54), (21, 54), (11, 27), (11, 27), (6, 14), (21, 54), (11, 27), (6, 14), (21, 54), (11, 27)]
SMALL_MAPS = [(1, 1), (2, 3), (6, 7), (11, 13)]
IBN_HW = [(21, 54), (21, 25), (11, 27), (11, 13), (6, 14), (6, 7), (1, 1), (2, 3)]


def _rows(x4, dt):
    B, C, H, W = x4.shape
    return x4.permute(0, 2, 3, 1).reshape(B * H * W, C).to(dt).contiguous()


def _bchw(rows, B, H, W):
    return rows.double().view(B, H, W, -1).permute(0, 3, 1, 2)


def _conv_grads64(x, w, dy, stride, padding):
    """fp64 autograd of F.conv2d -> (dx, dw): on the GPU (ATen's own fp64 path); on the CPU where the GPU build has no fp64 convolution"""
    def run(dev):
        xs, ws = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
        return torch.autograd.grad(F.conv2d(xs, ws, stride=stride, padding=padding), (xs, ws), dy.to(dev))
    try:
        dx, dw = run(DEV)
    except RuntimeError:
        dx, dw = run("cpu")
    return dx.cpu(), dw.cpu()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("pair", CONV_PAIRS, ids=lambda p: "C%dCo%dk%ds%d" % p)
def test_conv2d_backward_vs_fp64(pair, dt):
    from neuralsampleid_amd import _lib, ops
    C, Co, k, s = pair
    pi = CONV_PAIRS.index(pair)
    for hi, (H, W) in enumerate(SMALL_MAPS + [MODEL_MAP[pi]]):
        B = BS[(hi + pi) % 3]
        g = torch.Generator().manual_seed(2000 * pi + 10 * hi)
        Ho, Wo = ops.conv_out_size(H, k, s), ops.conv_out_size(W, k, s)
        # positive means: a tap that read a neighbouring image row or clip instead of zero shows in full
        x = (torch.randn(B, C, H, W, generator=g) + 0.7).to(dt)
        dy = (torch.randn(B, Co, Ho, Wo, generator=g) + 0.5).to(dt)
        w = torch.randn(Co, C, k, k, generator=g) * (C * k * k) ** -0.5
        add = (torch.randn(B, C, H, W, generator=g) + 0.3).to(dt)
        w_op = w.to(dt).double()                     # the operand the data kernel multiplies with
        dx64, dw64 = _conv_grads64(x.double(), w_op, dy.double(), s, k // 2)
        wt = ops.pack_conv_bwd(w).to(DEV)
        xr, dyr, addr = _rows(x, dt).to(DEV), _rows(dy, dt).to(DEV), _rows(add, dt).to(DEV)
        where = f"C{C} Co{Co} k{k} s{s} B{B} {H}x{W} {dt}"
        # ---- data gradient, without and with the addend
        before = _lib.launch_counters()
        dx = ops.conv2d_bwd_data(dyr, B, H, W, C, wt, Co, k, s)
        after = _lib.launch_counters()
        assert after["conv2d_bwd_data"] == before["conv2d_bwd_data"] + 1
        assert dx.dtype == dt and dx.shape == (B * H * W, C)
        err = relerr(_bchw(dx, B, H, W).cpu(), dx64)
        dxa = ops.conv2d_bwd_data(dyr, B, H, W, C, wt, Co, k, s, addend=addr)
        erra = relerr(_bchw(dxa, B, H, W).cpu(), dx64 + add.double())
        print(f"conv2d_bwd_data {where}: rel {err:.2e}, with addend {erra:.2e}")
        assert err < TOL[dt] and erra < TOL[dt], (pair, B, H, W, err, erra)
        assert torch.equal(dx, ops.conv2d_bwd_data(dyr, B, H, W, C, wt, Co, k, s))
        if k == 1 and s == 2:                        # input pixels no output pixel reads
            dead = torch.ones(H, W, dtype=torch.bool)
            dead[::2, ::2] = False
            if dead.any():
                assert float(dx.float().view(B, H, W, C).cpu()[:, dead].abs().max()) == 0.0
        # ---- weight gradient (fp32, packed, accumulated)
        dwp = torch.zeros(Co, k * k * C, device=DEV)
        before = _lib.launch_counters()
        ops.conv2d_bwd_weight(dyr, xr, dwp, B, H, W, C, Co, k, s)
        after = _lib.launch_counters()
        assert after["conv2d_bwd_weight"] == before["conv2d_bwd_weight"] + 1
        errw = relerr(ops.unpack_conv_wgrad(dwp, C, k).cpu(), dw64)
        print(f"conv2d_bwd_weight {where}: rel {errw:.2e}")
        assert errw < TOL[dt], (pair, B, H, W, errw)
        dwp2 = torch.zeros_like(dwp)
        ops.conv2d_bwd_weight(dyr, xr, dwp2, B, H, W, C, Co, k, s)
        assert torch.equal(dwp, dwp2)
        if hi == 2:                                  # accumulates into what the buffer holds
            ops.conv2d_bwd_weight(dyr, xr, dwp2, B, H, W, C, Co, k, s)
            assert relerr(dwp2.cpu(), 2.0 * dwp.double().cpu()) < 1e-6


def test_conv2d_backward_narrow_input_and_refusals():
    """C = 64 < one column tile (the first block's shapes are row GEMMs in the model, but the kernels take them); unsupported shapes"""
    from neuralsampleid_amd import ops
    g = torch.Generator().manual_seed(7)
    B, C, Co, H, W = 2, 64, 128, 5, 6
    x, dy = torch.randn(B, C, H, W, generator=g) + 0.7, torch.randn(B, Co, H, W, generator=g) + 0.5
    w = torch.randn(Co, C, 3, 3, generator=g) / 24
    dx64, dw64 = _conv_grads64(x.double(), w.double(), dy.double(), 1, 1)
    dx = ops.conv2d_bwd_data(_rows(dy, torch.float32).to(DEV), B, H, W, C, ops.pack_conv_bwd(w).to(DEV), Co, 3, 1)
    dwp = torch.zeros(Co, 9 * C, device=DEV)
    ops.conv2d_bwd_weight(_rows(dy, torch.float32).to(DEV), _rows(x, torch.float32).to(DEV), dwp, B, H, W, C, Co, 3, 1)
    assert relerr(_bchw(dx, B, H, W).cpu(), dx64) < 2e-6 and relerr(ops.unpack_conv_wgrad(dwp, C, 3).cpu(), dw64) < 2e-6
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(RuntimeError, match="NSID_EINVAL"):            # C % 16
        ops.conv2d_bwd_data(z(20, 128), 1, 4, 5, 24, z(24, 9 * 128), 128, 3, 1)
    with pytest.raises(RuntimeError, match="NSID_EINVAL"):            # Cout % 128
        ops.conv2d_bwd_data(z(20, 64), 1, 4, 5, 48, z(48, 9 * 64), 64, 3, 1)
    with pytest.raises(RuntimeError, match="NSID_EINVAL"):            # stride 3
        ops.conv2d_bwd_data(z(4, 128), 1, 4, 5, 48, z(48, 9 * 128), 128, 3, 3)
    with pytest.raises(RuntimeError, match="NSID_EINVAL"):            # C % 32 under bf16
        ops.conv2d_bwd_weight(z(20, 128).bfloat16(), z(20, 48).bfloat16(), z(128, 9 * 48), 1, 4, 5, 48, 128, 3, 1)
    with pytest.raises(RuntimeError, match="NSID_EINVAL"):            # Cout % 128
        ops.conv2d_bwd_weight(z(20, 64), z(20, 48), z(64, 9 * 48), 1, 4, 5, 48, 64, 3, 1)
    with pytest.raises(RuntimeError, match="NSID_EINVAL"):            # ksize 5
        ops.conv2d_bwd_weight(z(20, 128), z(20, 48), z(128, 25 * 48), 1, 4, 5, 48, 128, 5, 1)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("pair", [(128, 128, 3, 1), (512, 512, 3, 2), (256, 512, 1, 2)], ids=lambda p: "C%dCo%dk%ds%d" % p)
def test_conv_statistics_through_bn_finalize(pair, dt):
    """col_stat of a conv2d output through bn_finalize (momentum 1: the running statistics become the batch's) against the mean and
    the unbiased variance of the fp64 convolution"""
    from neuralsampleid_amd import _lib, ops
    C, Co, k, s = pair
    for hi, (H, W) in enumerate([(2, 3), (11, 13), (21, 54)]):
        B = BS[hi]
        g = torch.Generator().manual_seed(C + hi)
        x = (torch.randn(B, C, H, W, generator=g) + 0.7).to(dt)
        w = torch.randn(Co, C, k, k, generator=g) * (C * k * k) ** -0.5
        wp = ops.pack_conv_bn(w)[0].to(DEV)
        try:
            ref = F.conv2d(x.to(DEV).double(), w.to(dt).to(DEV).double(), stride=s, padding=k // 2).cpu()
        except RuntimeError:
            ref = F.conv2d(x.double(), w.to(dt).double(), stride=s, padding=k // 2)
        y = ops.conv2d_fwd(_rows(x, dt).to(DEV), B, H, W, C, wp, None, Co, k, s)
        M = y.shape[0]
        before = _lib.launch_counters()
        stat = ops.col_stat(y, M, Co)
        assert _lib.launch_counters()["col_stat"] == before["col_stat"] + 1 and stat.shape == (2, ops.row_tiles(M), Co)
        rm, rv, nbt = torch.zeros(Co, device=DEV), torch.zeros(Co, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
        aff = ops.bn_finalize(stat, M, torch.ones(Co, device=DEV), torch.zeros(Co, device=DEV), rm, rv, nbt, momentum=1.0)
        mean64 = ref.mean(dim=(0, 2, 3))
        var64 = ((ref - mean64.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
        em, ev = relerr(rm.cpu(), mean64), relerr(rv.cpu(), var64 * (M / max(M - 1, 1)))
        print(f"conv stat C{C} Co{Co} k{k} s{s} B{B} {H}x{W} {dt}: mean {em:.2e} var {ev:.2e}")
        assert int(nbt) == 1 and em < TOL[dt] and ev < TOL[dt]
        assert bool(torch.isfinite(aff.invstd).all()) and bool((aff.invstd > 0).all())
        assert torch.equal(stat, ops.col_stat(y, M, Co))
        # a column slice (the BatchNorm half of the IBN) gives the slice's columns
        assert torch.equal(ops.col_stat(y[:, Co // 2:], M, Co // 2), stat[:, :, Co // 2:])


def _within(what, got, ref64, ref32, ulp=None):
    """max |got - ref64| <= 4 x max |ref32 - ref64|. ulp (bf16 storage only, module docstring): the floor is at least ulp x max |ref64|;
    a use of that is printed"""
    floor = float((ref32.double() - ref64).abs().max())
    err = float((got.detach().double().cpu().reshape(ref64.shape) - ref64).abs().max())
    if ulp is not None and err > 4.0 * floor:
        clamped = max(floor, ulp * float(ref64.abs().max()))
        print(f"  {what}: max |kernel - fp64| = {err:.3g} exceeds 4 x the fp32 formula's {floor:.3g}: NEEDS the half-ulp floor {clamped:.3g}")
        floor = clamped
    print(f"  {what}: max |kernel - fp64| = {err:.3g}, allowed 4 x {floor:.3g}")
    return err <= 4.0 * floor


BAND = {torch.float32: (1e-4, 1e-3), torch.bfloat16: (2.0 ** -5, 5e-2)}      # (distance from zero in rms units, share of the elements)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [128, 256, 512, 1024])
def test_ibn_relu_bwd_vs_closed_form(C, dt):
    from neuralsampleid_amd import _lib, ops
    half = C // 2
    for hi, (H, W) in enumerate(IBN_HW):
        B = BS[(hi + C // 128) % 3]
        HW = H * W
        g = torch.Generator().manual_seed(3 * C + hi)
        # per-channel offsets of several standard deviations, as in the forward's test
        r = (torch.randn(B, C, H, W, generator=g) * 0.5 + 3.0 * torch.randn(1, C, 1, 1, generator=g) + 1.0).to(dt)
        dy = torch.randn(B, C, H, W, generator=g).to(dt)
        gi, bi = 1.0 + 0.1 * torch.randn(half, generator=g), 0.2 + 0.1 * torch.randn(half, generator=g)
        gb, bb = 1.0 + 0.1 * torch.randn(half, generator=g), 0.2 + 0.1 * torch.randn(half, generator=g)
        rows, dyr = _rows(r, dt).to(DEV), _rows(dy, dt).to(DEV)
        d = lambda t: t.to(DEV)
        # the forward as the block runs it: batch statistics in the BatchNorm half (from fp64: module docstring), then IBN + ReLU
        rb = r.double()[:, half:]
        mean64 = rb.mean(dim=(0, 2, 3))
        invstd64 = (((rb - mean64.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3)) + 1e-5).rsqrt()
        sc64 = gb.double() * invstd64
        aff = ops.BNAffine(d(sc64.float()), d((bb.double() - mean64 * sc64).float()), d(mean64.float()), d(invstd64.float()))
        y = ops.ibn_relu_fwd(rows, B, HW, C, d(gi), d(bi), aff, 1e-5)
        mask = (_bchw(y, B, H, W) > 0).cpu()
        # the kernel's mask is the fp64 mask wherever the fp64 pre-activation is clear of zero
        pre64 = O.ibn_relu_forward(r.double(), gi.double(), bi.double(), gb.double(), bb.double())
        thr, cap = BAND[dt]
        clear = pre64.abs() > thr * pre64.pow(2).mean().sqrt()
        share = 1.0 - float(clear.double().mean())
        assert torch.equal(mask[clear], (pre64 > 0)[clear]) and share <= cap, (C, H, W, share)
        zs = [torch.zeros(half, device=DEV) for _ in range(4)]
        before = _lib.launch_counters()
        dr = ops.ibn_relu_bwd(dyr, rows, B, HW, C, d(gi), d(bi), aff, *zs, 1e-5)
        assert _lib.launch_counters()["ibn_relu_bwd"] == before["ibn_relu_bwd"] + 1 and dr.dtype == dt
        ref64 = O.ibn_relu_bwd_closed_form(r.double(), dy.double(), mask, gi.double(), gb.double())
        ref32 = O.ibn_relu_bwd_closed_form(r.float(), dy.float(), mask, gi, gb)
        print(f"ibn bwd C{C} B{B} {H}x{W} {dt}: band share {share:.2e}")
        bf = dt == torch.bfloat16
        dr32 = ref32[0].to(dt).float()               # bf16 storage: the stored tensor's rounding belongs to its floor (fp32: a no-op)
        ok = [_within("dr", _bchw(dr, B, H, W), ref64[0], dr32)]
        for name, got, i in (("dgamma IN", zs[0], 1), ("dbeta IN", zs[1], 2), ("dgamma BN", zs[2], 3), ("dbeta BN", zs[3], 4)):
            ok.append(_within(name, got, ref64[i], ref32[i], 2.0 ** -24 if bf else None))
        if HW == 1:
            assert float(dr.float().view(B, HW, C)[:, :, :half].abs().max()) == 0.0
        # no atomics: bitwise reproducible
        zs2 = [torch.zeros(half, device=DEV) for _ in range(4)]
        dr2 = ops.ibn_relu_bwd(dyr, rows, B, HW, C, d(gi), d(bi), aff, *zs2, 1e-5)
        assert torch.equal(dr, dr2) and all(torch.equal(a, b) for a, b in zip(zs, zs2))
        # the instance-norm half of a clip alone is that half inside the batch (the BatchNorm half keeps the batch's statistics)
        b0 = (B - 1) * HW
        zs3 = [torch.zeros(half, device=DEV) for _ in range(4)]
        last = ops.ibn_relu_bwd(dyr[b0:].contiguous(), rows[b0:].contiguous(), 1, HW, C, d(gi), d(bi), aff, *zs3, 1e-5)
        assert torch.equal(last[:, :half], dr[b0:, :half])
        assert all(ok), (C, B, H, W)


@pytest.mark.parametrize("case", [(128, 3, 21, 54), (256, 8, 6, 7)], ids=lambda c: "C%dB%d_%dx%d" % c)
def test_ibn_relu_bwd_on_fp32_sum_statistics(case):
    """fp32 storage, the BatchNorm half on the statistics ResidualIBN.train_rows gives it (col_stat -> bn_finalize) at the offsets of
    the test above. The tile sums of x^2 are fp32 numbers added in chains of 32: each carries a relative error of about
    2^-24 sqrt(32), which E[x^2] - mean^2 turns into kappa = E[x^2] / var times as much in the variance, half of it in invstd, and dr
    is proportional to invstd. Bound: 4 x the fp32 formula's distance (the kernel's own arithmetic, as above) + max |dr| x
    max_c kappa_c x 2^-24 sqrt(32) / 2. Measured on one MI355X (printed): C = 128 on 21 x 54, kappa 453: invstd 1.8e-6 relative, dr
    9.5e-5 from fp64 = 72 x the fp32 formula's 1.3e-6, allowed 7.7e-4; C = 256 on 6 x 7, kappa 318: 2.1e-6, 6.6e-5 = 62 x, allowed
    5.1e-4. The instance-norm half, which takes no statistics from outside, keeps the plain 4 x bound (1.2 x and 2.6 x measured)."""
    from neuralsampleid_amd import ops
    C, B, H, W = case
    half, HW = C // 2, H * W
    g = torch.Generator().manual_seed(5 * C + H)
    r = torch.randn(B, C, H, W, generator=g) * 0.5 + 3.0 * torch.randn(1, C, 1, 1, generator=g) + 1.0
    dy = torch.randn(B, C, H, W, generator=g)
    gi, bi = 1.0 + 0.1 * torch.randn(half, generator=g), 0.2 + 0.1 * torch.randn(half, generator=g)
    gb, bb = 1.0 + 0.1 * torch.randn(half, generator=g), 0.2 + 0.1 * torch.randn(half, generator=g)
    rows, dyr = _rows(r, torch.float32).to(DEV), _rows(dy, torch.float32).to(DEV)
    d = lambda t: t.to(DEV)
    aff = ops.bn_finalize(ops.col_stat(rows[:, half:], B * HW, half), B * HW, d(gb), d(bb), None, None, None)
    y = ops.ibn_relu_fwd(rows, B, HW, C, d(gi), d(bi), aff, 1e-5)
    mask = (_bchw(y, B, H, W) > 0).cpu()
    zs = [torch.zeros(half, device=DEV) for _ in range(4)]
    dr = _bchw(ops.ibn_relu_bwd(dyr, rows, B, HW, C, d(gi), d(bi), aff, *zs, 1e-5), B, H, W).cpu()
    ref64 = O.ibn_relu_bwd_closed_form(r.double(), dy.double(), mask, gi.double(), gb.double())
    ref32 = O.ibn_relu_bwd_closed_form(r, dy, mask, gi, gb)
    rb = r.double()[:, half:]
    mean = rb.mean(dim=(0, 2, 3))
    var = ((rb - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    kappa = float(((mean * mean + var) / var).max())
    floor = float((ref32[0].double() - ref64[0])[:, half:].abs().max())
    stat_term = float(ref64[0][:, half:].abs().max()) * kappa * 2.0 ** -24 * 32 ** 0.5 / 2
    err_bn = float((dr - ref64[0])[:, half:].abs().max())
    err_is = relerr(aff.invstd.cpu(), (var + 1e-5).rsqrt())
    print(f"ibn bwd on fp32-sum statistics C{C} B{B} {H}x{W}: invstd rel {err_is:.2e}, kappa {kappa:.0f}; BatchNorm-half dr max error "
          f"{err_bn:.3g} = {err_bn / floor:.1f} x the fp32 formula's {floor:.3g}; allowed 4 x {floor:.3g} + {stat_term:.3g}")
    assert err_bn <= 4.0 * floor + stat_term
    assert _within("dr, instance-norm half", dr[:, :half], ref64[0][:, :half], ref32[0][:, :half])
