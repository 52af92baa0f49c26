"""GPU: the ResNet-IBN baseline's eval-mode forward (csrc/resnet.hip, encoder/resnet_ibn.py, simclr/triplet.py).

Kernels against torch fp64 restatements; the whole model against the reference's goldens (tests/golden/make_resnet_golden.py) with
tolerances built from the noise floors stored in the fixtures; the consumers (extract_fingerprints, GraphedFingerprinter, build_fp_db);
reproducibility and launch counters."""
import hashlib
import os

import numpy as np
import pytest
import torch

from compare import relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = torch.nn.functional
TOL = {torch.float32: 2e-6, torch.bfloat16: 1e-2}          # the project's bounds: relative L2 error, fp32 / bf16 storage
HW = [(21, 54), (21, 25), (11, 27), (11, 13), (6, 14), (6, 7), (1, 1), (2, 3)]
BS = [1, 3, 8]
# (C, Cout, ksize, stride) of every launch of nsid_conv2d_fwd in the model: conv2 of the eight blocks, conv3 (1x1 with the residual
# epilogue), the stride-2 downsample branches of layer3 / layer4
CONV_PAIRS = [(128, 128, 3, 1), (256, 256, 3, 1), (256, 256, 1, 1), (512, 512, 3, 2), (512, 512, 3, 1), (1024, 1024, 3, 2),
              (1024, 1024, 3, 1), (128, 128, 1, 1), (512, 512, 1, 1), (1024, 1024, 1, 1), (256, 512, 1, 2), (512, 1024, 1, 2)]
INPUTS = [(4, 216), (3, 100), (1, 216), (2, 431)]
STAGES = ("stem", "layer1", "layer2", "layer3", "layer4")


@pytest.fixture
def restore():
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops
    yield
    F_.set_activation_dtype(torch.float32)
    ops.set_gemm_precision("fp32")


def _rows(x4, dt):
    """(B, C, H, W) -> channels-last rows (B*H*W, C) in storage type dt"""
    B, C, H, W = x4.shape
    return x4.permute(0, 2, 3, 1).reshape(B * H * W, C).to(dt).contiguous()


def _bchw(rows, B, H, W):
    return rows.double().view(B, H, W, -1).permute(0, 3, 1, 2)


def _conv64(x, w, stride, padding):
    """fp64 F.conv2d on the GPU (ATen's own fp64 path); on the CPU where the GPU build has no fp64 convolution"""
    try:
        return F.conv2d(x, w, stride=stride, padding=padding)
    except RuntimeError:
        return F.conv2d(x.cpu(), w.cpu(), stride=stride, padding=padding).to(x.device)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("epilogue", ["plain", "res_relu"])
@pytest.mark.parametrize("pair", CONV_PAIRS, ids=lambda p: "C%dCo%dk%ds%d" % p)
def test_conv2d_vs_fp64(pair, epilogue, dt):
    from neuralsampleid_amd import _lib, ops
    C, Co, k, s = pair
    pi = CONV_PAIRS.index(pair)
    for hi, (H, W) in enumerate(HW):                       # every map size; the three batch sizes rotate over them per pair
        B = BS[(hi + pi) % 3]
        g = torch.Generator().manual_seed(1000 * pi + 10 * hi + (epilogue == "plain"))
        # positive mean: a padding tap that read a neighbour (the next image row, the next clip) instead of 0 shows in full
        x = (torch.randn(B, C, H, W, generator=g) + 0.7).to(dt)
        w = torch.randn(Co, C, k, k, generator=g) * (C * k * k) ** -0.5
        gamma, beta = 1.0 + 0.1 * torch.randn(Co, generator=g), 0.2 + 0.1 * torch.randn(Co, generator=g)
        mean, var = 0.1 * torch.randn(Co, generator=g), 0.5 + torch.rand(Co, generator=g)
        wp, bias = ops.pack_conv_bn(w, gamma, beta, mean, var)
        wp, bias = wp.to(DEV), bias.to(DEV)
        Ho, Wo = ops.conv_out_size(H, k, s), ops.conv_out_size(W, k, s)
        assert (Ho, Wo) == ((H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1)
        add = (torch.randn(B, Co, Ho, Wo, generator=g) + 0.3).to(dt) if epilogue == "res_relu" else None
        # the operand the kernel multiplies with: the packed, folded weight in the storage type's precision
        w_op = wp.to(dt).double().view(Co, k, k, C).permute(0, 3, 1, 2).contiguous()
        ref = _conv64(x.to(DEV).double(), w_op, s, k // 2) + bias.double().view(1, -1, 1, 1)
        if add is not None:
            ref = torch.relu(ref + add.to(DEV).double())
        before = _lib.launch_counters()
        y = ops.conv2d_fwd(_rows(x, dt).to(DEV), B, H, W, C, wp, bias, Co, k, s,
                           addend=None if add is None else _rows(add, dt).to(DEV), relu=add is not None)
        after = _lib.launch_counters()
        key = "conv2d_3x3" if k == 3 else "conv2d_1x1"
        assert after[key] == before[key] + 1
        assert y.dtype == dt and y.shape == (B * Ho * Wo, Co)
        err = relerr(_bchw(y, B, Ho, Wo).cpu(), ref.cpu())
        print(f"conv2d C{C} Co{Co} k{k} s{s} B{B} {H}x{W} {epilogue} {dt}: rel {err:.2e}")
        assert err < TOL[dt], (pair, B, H, W, err)


def test_conv2d_refuses_unsupported_shapes():
    from neuralsampleid_amd import ops
    x = torch.zeros(4 * 5, 48, device=DEV)
    with pytest.raises(RuntimeError, match="NSID_EINVAL"):            # C % 16
        ops.conv2d_fwd(torch.zeros(20, 24, device=DEV), 1, 4, 5, 24, torch.zeros(128, 9 * 24, device=DEV), None, 128, 3, 1)
    with pytest.raises(RuntimeError, match="NSID_EINVAL"):            # Cout % 128
        ops.conv2d_fwd(x, 1, 4, 5, 48, torch.zeros(64, 9 * 48, device=DEV), None, 64, 3, 1)
    with pytest.raises(RuntimeError, match="NSID_EINVAL"):            # stride 3
        ops.conv2d_fwd(x, 1, 4, 5, 48, torch.zeros(128, 9 * 48, device=DEV), None, 128, 3, 3)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [128, 256, 512, 1024])
def test_ibn_relu_vs_fp64_and_batch_independence(C, dt):
    from neuralsampleid_amd import ops
    for hi, (H, W) in enumerate(HW):
        B = BS[(hi + C // 128) % 3]
        g = torch.Generator().manual_seed(C + hi)
        # per-channel offsets of several standard deviations: E[x^2] - E[x]^2 in fp32 would lose the variance
        x = (torch.randn(B, C, H, W, generator=g) * 0.5 + 3.0 * torch.randn(1, C, 1, 1, generator=g) + 1.0).to(dt)
        gam, bet = 1.0 + 0.1 * torch.randn(C // 2, generator=g), 0.2 + 0.1 * torch.randn(C // 2, generator=g)
        sc, sh = 0.5 + torch.rand(C // 2, generator=g), 0.2 + 0.1 * torch.randn(C // 2, generator=g)
        xd = x.double()
        if H * W > 1:
            a = F.instance_norm(xd[:, :C // 2], weight=gam.double(), bias=bet.double(), eps=1e-5)
        else:                       # one pixel (torch refuses it): x - mean = 0, so the half is its beta
            a = bet.double().view(1, -1, 1, 1).expand(B, -1, 1, 1)
        b = xd[:, C // 2:] * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
        ref = torch.relu(torch.cat([a, b], 1))
        rows = _rows(x, dt).to(DEV)
        aff = ops.BNAffine(sc.to(DEV), sh.to(DEV))
        y = ops.ibn_relu_fwd(rows, B, H * W, C, gam.to(DEV), bet.to(DEV), aff, 1e-5)
        assert y.dtype == dt
        err = relerr(_bchw(y, B, H, W).cpu(), ref)
        print(f"ibn C{C} B{B} {H}x{W} {dt}: rel {err:.2e}")
        assert err < TOL[dt], (C, B, H, W, err)
        # a clip alone is bitwise the clip inside the batch
        last = ops.ibn_relu_fwd(rows[(B - 1) * H * W:].contiguous(), 1, H * W, C, gam.to(DEV), bet.to(DEV), aff, 1e-5)
        assert torch.equal(last, y[(B - 1) * H * W:])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(1, 84, 216), (3, 84, 100), (8, 84, 431), (2, 37, 29), (3, 1, 1), (2, 5, 2), (1, 84, 65)],
                         ids=lambda s: "B%dH%dW%d" % s)
def test_stem_vs_fp64(shape, dt):
    from neuralsampleid_amd import ops
    B, H, W = shape
    g = torch.Generator().manual_seed(B + H + W)
    x = torch.randn(B, H, W, generator=g).abs() * 2 + 0.5
    w = torch.randn(64, 1, 7, 7, generator=g) / 7.0
    gamma, beta = 1.0 + 0.1 * torch.randn(64, generator=g), 0.3 + 0.1 * torch.randn(64, generator=g)
    mean, var = 0.1 * torch.randn(64, generator=g), 0.5 + torch.rand(64, generator=g)
    w49, bias = ops.pack_conv_bn(w, gamma, beta, mean, var)
    conv = F.conv2d(x.double().unsqueeze(1), w49.double().view(64, 1, 7, 7), bias.double(), stride=2, padding=3)
    ref = F.max_pool2d(torch.relu(conv), 3, 2, 1)
    y, Hp, Wp = ops.stem7_pool_fwd(x.to(DEV), w49.to(DEV), bias.to(DEV), dt)
    assert (Hp, Wp) == tuple(ref.shape[2:]) and y.dtype == dt and y.shape == (B * Hp * Wp, 64)
    err = relerr(_bchw(y, B, Hp, Wp).cpu(), ref)
    print(f"stem {shape} {dt}: rel {err:.2e}")
    assert err < TOL[dt], err


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("p", [2.5, 3.0, 1.0])
def test_gem_vs_fp64(p, dt):
    from neuralsampleid_amd import ops
    for hi, (H, W) in enumerate(HW):
        B, C = BS[hi % 3], (1024, 512, 64)[hi % 3]
        g = torch.Generator().manual_seed(hi)
        x = (torch.randn(B, C, H, W, generator=g) + 0.5).to(dt)          # negative values: the clamp is exercised
        ref = F.adaptive_avg_pool2d(x.double().clamp(min=1e-6).pow(p), (1, 1)).pow(1.0 / p).view(B, C)
        pt = torch.full((1,), p, device=DEV)
        y = ops.gem_pool_fwd(_rows(x, dt).to(DEV), B, H * W, C, pt, 1e-6)
        assert y.dtype == torch.float32 and y.shape == (B, C)
        err = relerr(y.cpu(), ref)
        print(f"gem p{p} B{B} C{C} {H}x{W} {dt}: rel {err:.2e}")
        assert err < TOL[dt], err


# ------------------------------------------------------------------------------------------------------------------ the model
def _model(dt=torch.float32, p=2.5):
    from synth import synth_state
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    from neuralsampleid_amd.simclr.triplet import BaselineModel
    F_.set_activation_dtype(dt)
    ops.set_gemm_precision("fp32")              # the parity arithmetic of the row GEMMs (a process-wide switch other tests move)
    model = BaselineModel({"arch": "resnet-ibn", "n_frames": 216}, ResNetIBN())
    sd = synth_state(model.state_dict())
    sd["encoder.global_pool.p"] = torch.full((1,), p)
    model.load_state_dict(sd)
    return model.to(DEV).eval()


def _input(gold, B, T):
    from synth import synth_randn
    x = synth_randn(f"resnet_ibn_b{B}_t{T}", B, 84, T).abs() * 2
    assert hashlib.sha256(x.numpy().tobytes()).hexdigest()[:16] == bytes(gold["input_sha"]).decode(), \
        "synth_randn no longer reproduces the fixture's input"
    return x.to(DEV)


def _run(model, x):
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.encoder.resnet_ibn import rows_to_bchw
    stages = {}
    with torch.no_grad():
        h = model.encoder.forward_rows(x, stages=stages)
        z, _ = ops.l2norm_fwd(h, 1e-10)
    return h, z, {k: rows_to_bchw(r, x.shape[0], H, W) for k, (r, H, W) in stages.items()}


@pytest.mark.parametrize("inp", INPUTS, ids=lambda s: "B%dT%d" % s)
def test_model_fp32_vs_reference(golden, restore, inp):
    """fp32 storage: every stage, h and z within 20 x the reference's own fp32-vs-fp64 noise on this input (the summation order over
    K up to 9 216 differs; the stored floor is one draw of that noise over 14 stacked layers with instance normalisation between).
    Measured on MI355X, as multiples of the stored floors over the four inputs: stages 1.2-1.6 x, h 2.8-3.2 x, max|dz| 4.1-6.3 x
    (DESIGN.md section 3a)."""
    B, T = inp
    gold = golden(f"resnet_ibn_b{B}_t{T}")
    model = _model()
    h, z, st = _run(model, _input(gold, B, T))
    torch.cuda.synchronize()
    fails = []
    for name, chw in zip(STAGES, gold["stage_chw"]):
        assert tuple(st[name].shape[1:]) == tuple(int(v) for v in chw), name
        e, floor = relerr(st[name].cpu(), gold.t(name)), float(gold[f"noise.fp32_rel.{name}"][0])
        print(f"fp32 B{B} T{T} {name}: rel {e:.2e} = {e / floor:.1f} x floor {floor:.1e}")
        if not e <= 20 * floor:
            fails.append((name, e, floor))
    e_h, f_h = relerr(h.cpu(), gold.t("h")), float(gold["noise.fp32_rel_h"][0])
    dz, f_z = float((z.cpu() - gold.t("z")).abs().max()), float(gold["noise.fp32_max_dz"][0])
    print(f"fp32 B{B} T{T} h: rel {e_h:.2e} = {e_h / f_h:.1f} x floor; max|dz| {dz:.2e} = {dz / f_z:.1f} x floor")
    assert not fails, fails
    assert e_h <= 20 * f_h, (e_h, f_h)
    assert dz <= 20 * f_z, (dz, f_z)
    # the model's own entry points give the same numbers
    with torch.no_grad():
        h_i, h_j, z_i, z_j = model(_input(gold, B, T), _input(gold, B, T))
    assert torch.equal(h_i, h) and torch.equal(h_j, h) and torch.equal(z_i, z) and torch.equal(z_j, z)


@pytest.mark.parametrize("inp", INPUTS, ids=lambda s: "B%dT%d" % s)
def test_model_bf16_vs_reference(golden, restore, inp):
    """bf16 storage: against the fp32 golden, within 4 x the deviation of the reference's own bf16 emulation on this input (the kernels
    round at other points than the emulation does). Measured on MI355X over the four inputs: 1 - min cos 1.00-1.11 x the emulation's,
    relative error of h 0.91-0.99 x."""
    B, T = inp
    gold = golden(f"resnet_ibn_b{B}_t{T}")
    model = _model(torch.bfloat16)
    h, z, st = _run(model, _input(gold, B, T))
    assert all(v is not None for v in st.values())
    cos = F.cosine_similarity(z.double().cpu(), gold.t("z").double(), dim=1)
    e_h = relerr(h.cpu(), gold.t("h"))
    f_cos, f_h = float(gold["emul.bf16_min_cos"][0]), float(gold["emul.bf16_rel_h"][0])
    print(f"bf16 B{B} T{T}: min cos {float(cos.min()):.7f} (1 - cos = {(1 - float(cos.min())) / (1 - f_cos):.2f} x emulation), "
          f"rel h {e_h:.2e} = {e_h / f_h:.2f} x emulation")
    assert float(cos.min()) >= 1 - 4 * (1 - f_cos), (float(cos.min()), f_cos)
    assert e_h <= 4 * f_h, (e_h, f_h)


def test_launch_counters_name_the_kernels(restore):
    from neuralsampleid_amd import _lib
    model = _model()
    x = torch.rand(2, 84, 216, device=DEV)
    with torch.no_grad():
        model._embed(x)
    before = _lib.launch_counters()
    with torch.no_grad():
        model._embed(x)
    after = _lib.launch_counters()
    d = {k: after[k] - before[k] for k in after}
    assert d["stem7_pool"] == 1 and d["gem_pool"] == 1 and d["ibn_relu"] == 8
    assert d["conv2d_3x3"] == 8                  # conv2 of the eight blocks
    assert d["conv2d_1x1"] == 8 + 2              # conv3 + residual + ReLU of the eight blocks, the stride-2 downsamples of layer3 / layer4
    # the 1x1 stride-1 layers are row GEMMs of the nsid_linear_fwd family: conv1 x 8, the stride-1 downsamples of layer1 / layer2, the head
    assert d["gemm_fwd"] + d["ws_fwd"] + d["gemm256"] == 8 + 2 + 1


def test_extraction_is_reproducible_and_batch_independent(golden, restore):
    from neuralsampleid_amd.fingerprint import extract_fingerprints
    gold = golden("resnet_ibn_b4_t216")
    model = _model()
    g = torch.Generator().manual_seed(5)
    specs = (torch.randn(64, 84, 216, generator=g).abs() * 2).to(DEV)
    z64 = extract_fingerprints(model, specs, batch=64)
    assert z64.shape == (64, 2048) and torch.equal(z64, extract_fingerprints(model, specs, batch=64))     # no atomics on the path
    z4 = extract_fingerprints(model, specs, batch=4)
    assert (z4.norm(dim=1) - 1).abs().max() < 1e-5
    dz, floor = float((z4 - z64).abs().max()), float(gold["noise.fp32_max_dz"][0])
    print(f"batch 4 vs batch 64: max|dz| {dz:.2e} ({dz / floor:.1f} x the fp32 floor)")
    assert dz <= 20 * floor


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_graphed_fingerprinter(restore, dt):
    from synth import synth_state
    from neuralsampleid_amd.fingerprint import GraphedFingerprinter, extract_fingerprints
    model = _model(dt)
    g = torch.Generator().manual_seed(9)
    specs = (torch.randn(19, 84, 216, generator=g).abs() * 2).to(DEV)
    fp = GraphedFingerprinter(model, micro_batch=8)
    assert tuple(fp.x.shape) == (8, 84, 216) and fp.d == 2048
    z = fp(specs)                                                     # 8 + 8 + a ragged tail of 3
    assert torch.equal(z, extract_fingerprints(model, specs, batch=8))
    with torch.no_grad():
        model.encoder.global_pool.p.fill_(3.0)
    with pytest.raises(RuntimeError, match="changed"):
        fp(specs)
    fp2 = GraphedFingerprinter(model, micro_batch=8, example=specs[:, :, :100].contiguous())
    assert tuple(fp2.x.shape) == (8, 84, 100)
    z2 = fp2(specs[:, :, :100].contiguous())
    assert torch.equal(z2, extract_fingerprints(model, specs[:, :, :100].contiguous(), batch=8))
    sd = synth_state(model.state_dict(), prefix="other.")
    sd["encoder.global_pool.p"] = torch.full((1,), 2.0)
    model.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="changed"):
        fp2(specs[:, :, :100].contiguous())
    # the eager path sees the new weights (folded / packed constants are keyed by parameter versions)
    z3 = extract_fingerprints(model, specs, batch=8)
    assert float((z3 - z).abs().max()) > 1e-3


def test_build_fp_db_writes_the_reference_format(restore, tmp_path):
    from neuralsampleid_amd import fpdb
    from neuralsampleid_amd.fingerprint import extract_fingerprints
    model = _model()
    g = torch.Generator().manual_seed(3)
    songs = [("a", (torch.randn(5, 84, 216, generator=g).abs() * 2).to(DEV)), ("b", (torch.randn(3, 84, 216, generator=g).abs() * 2).to(DEV))]
    n, d = fpdb.build_fp_db(model, songs, str(tmp_path), "ref_db", batch=4)
    assert (n, d) == (8, 2048)
    for suffix in (".mm", "_shape.npy", "_lookup.json"):
        assert os.path.exists(tmp_path / f"ref_db{suffix}")
    data, shape = fpdb.load_memmap_data(str(tmp_path), "ref_db")
    assert tuple(int(v) for v in shape) == (8, 2048) and fpdb.load_lookup(str(tmp_path), "ref_db") == ["a"] * 5 + ["b"] * 3
    want = torch.cat([extract_fingerprints(model, s, 4) for _, s in songs]).cpu().numpy()
    assert np.array_equal(np.asarray(data), want)
