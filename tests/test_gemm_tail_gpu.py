"""The peeled tail of the full-tile pipelined loop of csrc/gemm.hip (gemm_body, DEPTH == 2): the last two sub-steps of a tile request no
operands, commit nothing past the last stage, and the backward-data form asks for the BatchNorm input of its epilogue there.

Shapes are the smallest at which that logic can go wrong: reduction lengths of 2, 4 and 6 stages (the prologue meets the tail with no
steady iteration, with one, and with an odd count) in the 32-deep (KS = 1) and the 64-deep (KS = 2) form, one and two row tiles, one and two
column tiles of both tile widths, groups 1 and 4. The full-tile forms exist for bf16 storage with bf16 weights only, so every case runs on
bf16 tensors; references are fp64 products of the SAME bf16 operand values, so what is left is fp32 accumulation and, where the output is
stored as bf16, one rounding of it.

The weight-stationary kernels (csrc/wsgemm.hip) take most of these small shapes by default: ws_gemm = 0 keeps every launch here on
gemm.hip, and the launch counters say which form ran."""
import itertools

import pytest
import torch

from compare import absmax, maxerr, relerr
from synth import synth_randn

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture()
def ops():
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops as o
    o.set_gemm_precision("bf16")
    o.set_tuning("ws_gemm", 0)
    yield o
    o.reset_tuning()
    o.set_gemm_precision("fp32")
    F_.set_activation_dtype("fp32")


def close(a, b, tol, what=""):
    """tests/test_ops_gpu.py::close: max error relative to the reference's scale"""
    scale = max(1.0, absmax(b))
    err = maxerr(a, b)
    assert err <= tol * scale, f"{what}: max err {err:.3e} (scale {scale:.3e})"


_CACHE = {}


def rnd(tag, *shape):
    """one synthetic tensor per (tag, shape), generated once and shared (never modified)"""
    key = (tag,) + shape
    if key not in _CACHE:
        _CACHE[key] = synth_randn("tail:" + tag, *shape)
    return _CACHE[key]


def bn_affine(ops, r):
    C = r.shape[1]
    mean, var = r.float().mean(0), r.float().var(0, unbiased=False)
    invstd = 1 / torch.sqrt(var + 1e-5)
    gamma, beta = (1 + 0.2 * rnd("g", C)).to(DEV), (0.1 * rnd("b", C)).to(DEV)
    return ops.BNAffine((gamma * invstd).contiguous(), (beta - mean * gamma * invstd).contiguous(), mean.contiguous(), invstd.contiguous())


def bwd_data_reference(dout, w, add, r, aff, act, M, R, K, groups):
    """fp64: din = dout w (+ addend) per group, and the BatchNorm-backward column sums per 128-row tile of the UNROUNDED din"""
    wd = w.to(BF).double().cpu()
    din = torch.cat([dout.double().cpu()[:, g * R:(g + 1) * R] @ wd[g * R:(g + 1) * R] for g in range(groups)], 1)
    if add is not None:
        din = din + add.double().cpu()
    if r is None:
        return din, None
    x = r.double().cpu()
    z = aff.scale.double().cpu() * x + aff.shift.double().cpu()
    g = din * {0: torch.ones_like(z), 1: (z > 0).double(), 2: torch.where(z > 0, 1.0, 0.2)}[act]
    xh = (x - aff.mean.double().cpu()) * aff.invstd.double().cpu()
    part = torch.stack([g.reshape(M // 128, 128, -1).sum(1), (g * xh).reshape(M // 128, 128, -1).sum(1)])
    return din, part


@pytest.mark.parametrize("deep", [False, True])
@pytest.mark.parametrize("stages", [2, 4, 6])
@pytest.mark.parametrize("M", [128, 256])
def test_backward_data_tail(ops, M, stages, deep):
    """Backward-data on full tiles. KS = 1 cases: reduction 64 / 128 / 192. Deep cases: reduction 128 / 256 / 384, run with gemm_deep_kinds
    = 5 (32-deep stages) and = 7 (64-deep stages): din and the BatchNorm partial sums are equal bit for bit (the order of the MFMAs over
    the reduction index is the same), and the gemm_ks2 counter says that each form really ran. Either way din and the sums agree with the
    fp64 product of the same bf16 operands within the bf16-storage tolerance of test_bf16_storage_gpu.py::test_linear_family_bf16_storage
    (relative L2 2.5e-3: one rounding of din to bf16; the sums are taken over the rounded din)."""
    R = stages * (64 if deep else 32)
    for K, groups, narrow, has_add, bnact in itertools.product((128, 256), (1, 4), (0, 1), (False, True), (None, 0, 1, 2)):
        ops.set_tuning("bwd_narrow", narrow)
        dout = rnd("dout", M, groups * R).to(BF).to(DEV)
        w = (rnd("w", groups * R, K) * R ** -0.5).to(DEV)
        add = rnd("add", M, groups * K).to(BF).to(DEV) if has_add else None
        r = (rnd("r", M, groups * K) * 1.3 + 0.2).to(BF).to(DEV) if bnact is not None else None
        aff = bn_affine(ops, r) if r is not None else None
        got = {}
        for kinds in ((5, 7) if deep else (5,)):
            ops.set_tuning("gemm_deep_kinds", kinds)
            ops.launch_counters(reset=True)
            if r is None:
                din, part = ops.linear_bwd_data(dout, w, M, R, K, groups, add), None
            else:
                din, part = ops.linear_bwd_data(dout, w, M, R, K, groups, add, bn=(r, aff, bnact))
            c = ops.launch_counters()
            what = f"K={K} groups={groups} narrow={narrow} add={has_add} bn={bnact} kinds={kinds}"
            assert c["gemm_bwd_data"] == 1 and c["gemm_full"] == 1 and c["gemm_ks2"] == (1 if kinds == 7 else 0), (what, c)
            assert c["gemm_bn_sums"] == (0 if r is None else 1), (what, c)
            got[kinds] = (din, part)
        ref_din, ref_part = bwd_data_reference(dout, w, add, r, aff, bnact, M, R, K, groups)
        for kinds, (din, part) in got.items():
            assert din.dtype == BF and relerr(din, ref_din) < 2.5e-3, (what, kinds, relerr(din, ref_din))
            if r is not None:
                assert part.shape == (2, M // 128, groups * K)
                assert relerr(part, ref_part) < 2.5e-3, (what, kinds, relerr(part, ref_part))
        if deep:
            assert torch.equal(got[5][0], got[7][0]), what
            if r is not None:
                assert torch.equal(got[5][1], got[7][1]), what


@pytest.mark.parametrize("R", [64, 192])
def test_full_tile_rows_equal_the_predicated_launch(ops, R):
    """Row independence: rows 0..127 of a ragged launch (M = 200: the predicated loop with its zero-filled phantom stages, which this
    change does not touch) equal the M = 128 launch (full tiles: the peeled loop) on the same rows bit for bit, forward (operand affine
    + ReLU, statistics) and backward-data (addend, BatchNorm sums) at KS = 1, both tile widths."""
    Mr, M, C = 200, 128, 128
    for narrow in (0, 1):
        ops.set_tuning("fwd_narrow", narrow)
        ops.set_tuning("bwd_narrow", narrow)
        # forward: out[M][C] = relu(sc x + sh) w^T, reduction R
        x = rnd("fx", Mr, R).to(BF).to(DEV)
        w = (rnd("fw", C, R) * R ** -0.5).to(DEV)
        bias = rnd("fb", C).to(DEV)
        sc, sh = (1 + 0.2 * rnd("fsc", R)).to(DEV), (0.3 * rnd("fsh", R)).to(DEV)
        ops.launch_counters(reset=True)
        o_r, s_r = ops.linear_fwd(x, w, bias, Mr, C, R, 1, sc, sh, 1, 0, want_stat=True)
        assert ops.launch_counters()["gemm_full"] == 0
        ops.launch_counters(reset=True)
        o_f, s_f = ops.linear_fwd(x[:M].contiguous(), w, bias, M, C, R, 1, sc, sh, 1, 0, want_stat=True)
        c = ops.launch_counters()
        assert c["gemm_full"] == 1 and c["gemm_affine_load"] == 1 and c["gemm_ks2"] == 0, c
        assert torch.equal(o_r[:M], o_f) and torch.equal(s_r[:, 0], s_f[:, 0]), f"forward, narrow={narrow}"
        # backward-data: din[M][C] = dout w + addend, reduction R
        dout = rnd("bd", Mr, R).to(BF).to(DEV)
        wb = (rnd("bw", R, C) * R ** -0.5).to(DEV)
        add = rnd("ba", Mr, C).to(BF).to(DEV)
        r = (rnd("br", Mr, C) * 1.3 + 0.2).to(BF).to(DEV)
        aff = bn_affine(ops, r)
        ops.launch_counters(reset=True)
        d_r, p_r = ops.linear_bwd_data(dout, wb, Mr, R, C, 1, add, bn=(r, aff, 1))
        assert ops.launch_counters()["gemm_full"] == 0
        ops.launch_counters(reset=True)
        d_f, p_f = ops.linear_bwd_data(dout[:M].contiguous(), wb, M, R, C, 1, add[:M].contiguous(), bn=(r[:M].contiguous(), aff, 1))
        c = ops.launch_counters()
        assert c["gemm_full"] == 1 and c["gemm_bn_sums"] == 1 and c["gemm_ks2"] == 0, c
        assert torch.equal(d_r[:M], d_f) and torch.equal(p_r[:, 0], p_f[:, 0]), f"backward-data, narrow={narrow}"


@pytest.mark.parametrize("M,Nout,K,link", [(128, 64, 64, True), (256, 64, 128, False), (128, 128, 128, True), (256, 128, 256, True)])
def test_bn_apply_on_load_writes_every_stage_of_dr(ops, M, Nout, K, link):
    """The ABN form (BatchNorm backward evaluated on the operand load; reduction Nout = 2 or 4 stages, 64- and 128-wide tiles, one and two
    column tiles): the side output dr is complete -- every stage is committed, and therefore stored, exactly once, the last one included
    -- and equal to the two-call form within the statement of test_bf16_storage_gpu.py::test_bn_backward_on_the_backward_data_operand_load.
    The output buffers of the fused call are allocated inside ops; NaN-filled blocks of their size are freed just before, so that a
    stage that is not written shows as NaN (or, if the allocator hands out other memory, as a mismatch with the two-call form)."""
    act = 1
    dy = rnd("ady", M, Nout).to(BF).to(DEV)
    r = (rnd("ar", M, Nout) * 1.3 + 0.2).to(BF).to(DEV)
    w = (rnd("aw", Nout, K) * Nout ** -0.5).to(DEV)
    addend = rnd("aa", M, K).to(BF).to(DEV)
    aff = bn_affine(ops, r)
    bn = False
    if link:
        r_up = (rnd("au", M, K) * 0.8 - 0.1).to(BF).to(DEV)
        mu, vu = r_up.float().mean(0), r_up.float().var(0, unbiased=False)
        iu = 1 / torch.sqrt(vu + 1e-5)
        bn = (r_up, ops.BNAffine(iu, -mu * iu, mu, iu), 1)
    out = {}
    before = ops.FUSE_BN_BWD_APPLY
    for fuse in (False, True):
        dg, db = torch.zeros(Nout, device=DEV), torch.zeros(Nout, device=DEV)
        if fuse:
            poison = [torch.full((M, Nout), float("nan"), device=DEV, dtype=BF), torch.full((M, K), float("nan"), device=DEV, dtype=BF)]
            torch.cuda.synchronize()
            del poison
        ops.FUSE_BN_BWD_APPLY = fuse
        ops.launch_counters(reset=True)
        try:
            dr, din, part = ops.bn_backward_linear_bwd_data(dy.clone(), r, aff, act, dg, db, None, w, M, Nout, K, 1, addend=addend, bn=bn)
        finally:
            ops.FUSE_BN_BWD_APPLY = before
        torch.cuda.synchronize()
        out[fuse] = (dr.float(), din.float(), part, ops.launch_counters())
    (dr0, din0, p0, c0), (dr1, din1, p1, c1) = out[False], out[True]
    assert c0["gemm_bn_apply_load"] == 0 and c0["bn_bwd_apply"] == 1, c0
    assert c1["gemm_bn_apply_load"] == 1 and c1["bn_bwd_apply"] == 0, c1
    assert bool(torch.isfinite(dr1).all()) and bool(torch.isfinite(din1).all())
    assert relerr(dr1, dr0) < 1e-3, relerr(dr1, dr0)
    assert float(((dr1 - dr0).abs() > 2 ** -7 * dr0.abs().clamp_min(1e-3)).float().mean()) < 1e-4
    assert relerr(din1, din0) < 2.5e-3, relerr(din1, din0)
    if link:
        assert p1.shape == p0.shape and relerr(p1, p0) < 5e-3
    else:
        assert p0 is None and p1 is None


def act_ref(x, act):
    return {0: x, 1: torch.relu(x), 2: torch.nn.functional.leaky_relu(x, 0.2)}[act]


@pytest.mark.parametrize("K", [64, 128, 192, 256])
def test_forward_affine_relu_statistics_tail(ops, K):
    """Forward on full tiles with the producer's BatchNorm + ReLU on the operand load and the statistics epilogue (the affine vectors of a
    stage are prefetched per stage: the tail fetches those of the last stage and no more); K = 2 .. 8 stages of 32, K = 128 / 256 also in
    the 64-deep form. Against fp64 on the same bf16 operands (the affine has bf16-valued coefficients, so the kernel's fp32 fma and the
    reference round the operand to the same bf16 value). Tolerances of tests/test_ops_gpu.py::test_linear_fwd: statistics (fp32, from the
    accumulators) 5e-4 of the scale; out 2e-4 of the scale plus the rounding of its bf16 store (unit roundoff 2^-8 of the value: an
    8-bit significand), which a full-tile launch cannot avoid: it exists for bf16 storage only."""
    for M, Nout, narrow, kinds in itertools.product((128, 256), (128, 256), (0, 1), (0, 5)):
        ops.set_tuning("fwd_narrow", narrow)
        ops.set_tuning("gemm_deep_kinds", kinds)
        x = rnd("qx", M, K).to(BF)
        w = rnd("qw", Nout, K) * K ** -0.5
        bias = rnd("qb", Nout)
        sc, sh = (1 + 0.2 * rnd("qsc", K)).to(BF).float(), (0.3 * rnd("qsh", K)).to(BF).float()
        xin = torch.relu(x.double() * sc.double() + sh.double()).to(BF).double()
        ref = xin @ w.to(BF).double().t() + bias.double()
        ops.launch_counters(reset=True)
        out, stat = ops.linear_fwd(x.to(DEV), w.to(DEV), bias.to(DEV), M, Nout, K, 1, sc.to(DEV), sh.to(DEV), 1, 0, want_stat=True)
        c = ops.launch_counters()
        what = f"M={M} Nout={Nout} narrow={narrow} kinds={kinds}"
        assert c["gemm_full"] == 1 and c["gemm_affine_load"] == 1 and c["gemm_ks2"] == (1 if kinds == 5 and K % 128 == 0 else 0), (what, c)
        scale = max(1.0, absmax(ref))
        err = (out.double().cpu() - ref).abs()
        assert bool((err <= 2e-4 * scale + 2.0 ** -8 * ref.abs()).all()), (what, float(err.max()))
        rt = ref.reshape(M // 128, 128, -1)
        close(stat[0], rt.sum(1), 5e-4, what + " stat sum")
        close(stat[1], (rt * rt).sum(1), 5e-4, what + " stat sumsq")


def test_weight_gradient_splits_of_exactly_two_stages(ops):
    """Weight gradients whose every row split is exactly two stages (the prologue runs straight into the tail): the per-layer launch at
    M = 64 (two 32-deep stages) and M = 128 (two 64-deep stages), and the grouped launch (wgrad_grouped_kernel shares the body) at
    M = 512 with 128-row splits -- four splits of two 64-deep stages per view, both views as the two row segments of one problem, in
    the 128x64 and the 64x64 tile class, with and without the producer's BatchNorm + ReLU on x. fp32 output against fp64 on the same
    bf16 operands, tolerance of tests/test_ops_gpu.py::test_linear_bwd_weight (3e-4 of the scale)."""
    ops.set_tuning("wgrad_wide", 0)
    for key in ("wgg_rows", "wgg_rows_sq"):
        ops.set_tuning(key, 128)
    for key in ("wgg_w3", "wgrad256"):
        ops.set_tuning(key, 0)

    def operands(M, Nout, K, affine, view):
        dout = rnd(f"wd{view}", M, Nout).to(BF)
        x = rnd(f"wx{view}", M, K).to(BF)
        sc = (1 + 0.2 * rnd("wsc", K)).to(BF).float() if affine else None
        sh = (0.3 * rnd("wsh", K)).to(BF).float() if affine else None
        xin = torch.relu(x.double() * sc.double() + sh.double()).to(BF).double() if affine else x.double()
        return dout, x, sc, sh, dout.double().t() @ xin

    d = lambda t: None if t is None else t.to(DEV)
    for M, Nout, K, affine in itertools.product((64, 128), (64, 128), (64,), (False, True)):
        dout, x, sc, sh, ref = operands(M, Nout, K, affine, 0)
        dw = torch.ones(Nout, K, device=DEV)
        ops.launch_counters(reset=True)
        ops.linear_bwd_weight(d(dout), d(x), dw, M, Nout, K, 1, d(sc), d(sh), 1 if affine else 0)
        c = ops.launch_counters()
        assert c["gemm_bwd_weight"] == 1 and c["gemm_full"] == 1 and c["gemm_ks2"] == (1 if M == 128 else 0), c
        close(dw, ref + 1.0, 3e-4, f"per-layer M={M} Nout={Nout} affine={affine}")
    for Nout, affine in itertools.product((128, 64), (False, True)):
        M, K = 512, 64
        dout0, x0, sc, sh, ref0 = operands(M, Nout, K, affine, 0)
        dout1, x1, _, _, ref1 = operands(M, Nout, K, affine, 1)
        dw = torch.ones(Nout, K, device=DEV)
        act = 1 if affine else 0
        keep = [d(dout0), d(x0), d(dout1), d(x1), d(sc), d(sh)]
        ops.launch_counters(reset=True)
        ops.linear_bwd_weight_batch([(keep[0], keep[1], dw, M, Nout, K, 1, keep[4], keep[5], act),
                                     (keep[2], keep[3], dw, M, Nout, K, 1, keep[4], keep[5], act)])
        torch.cuda.synchronize()
        c = ops.launch_counters()
        assert c["wgrad_grouped"] == 1 and c["wgrad_grouped_w3"] == 0 and c["wgrad_grouped_256"] == 0, c
        close(dw, ref0 + ref1 + 1.0, 3e-4, f"grouped Nout={Nout} affine={affine}")
