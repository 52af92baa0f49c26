"""CPU: the training-mode ResidualIBN oracle (tests/resnet_train_oracle.py) pinned to the reference's goldens
(tests/golden/make_resnet_train_golden.py), its closed-form IBN backward pinned to autograd, the host-side weight packing of the
convolution backward, and the refusals of the new ops and of the model's training-mode forward."""
import pytest
import torch

import resnet_train_oracle as O
from compare import relerr

BLOCKS = [(64, 128, 1), (128, 256, 2)]
B, H, W = 3, 6, 7


@pytest.fixture(scope="module")
def lib():
    from neuralsampleid_amd.build import build_lib
    return build_lib(verbose=False)


def block_state(cin, cout, stride):
    """(tag, the block's synthesized state, input, upstream gradient) of a golden block"""
    from synth import synth_randn, synth_state
    from neuralsampleid_amd.encoder.resnet_ibn import ResidualIBN
    tag = f"c{cin}_{cout}_s{stride}"
    sd = synth_state(ResidualIBN(cin, cout, stride).state_dict(), prefix=tag + ".")
    x = synth_randn(tag, B, cin, H, W)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return tag, sd, x, synth_randn(tag + "_dout", B, cout, Ho, Wo)


@pytest.mark.parametrize("blk", BLOCKS, ids=lambda b: "c%d_%d_s%d" % b)
def test_oracle_matches_the_reference_golden(golden, blk):
    tag, sd, x, dout = block_state(*blk)
    gold = golden("resnet_train_" + tag)
    ref = O.block_reference(x, sd, blk[2], dout, torch.float64)
    errs = {"out": relerr(ref["out"], gold.t("out")), "dx": relerr(ref["dx"], gold.t("dx"))}
    for k, g in ref["grads"].items():
        errs["grad." + k] = relerr(g, gold.t("grad." + k))
    # bn2.bias has an exactly zero gradient (a per-channel constant in front of conv3 is removed by bn3's mean subtraction): what both
    # sides hold is rounding noise, measured against the norm of bn2.weight's gradient
    noise = ref["grads"]["bn2.bias"].norm() / ref["grads"]["bn2.weight"].norm()
    assert float(noise) < 1e-12 and gold.t("grad.bn2.bias").norm() < 1e-12 * gold.t("grad.bn2.weight").norm()
    errs["grad.bn2.bias"] = float(noise)
    for k, v in ref["running"].items():
        errs["state." + k] = relerr(v, gold.t("state." + k))
    assert len(errs) == 2 + 14 + 8
    assert list(gold["nbt"]) == [1, 1, 1, 1]
    for k, e in errs.items():
        print(f"  {tag} {k}: rel {e:.2e}")
    assert max(errs.values()) < 1e-10, errs


@pytest.mark.parametrize("hw", [(6, 7), (2, 3), (1, 1)])
def test_closed_form_ibn_backward_is_autograd(hw):
    g = torch.Generator().manual_seed(5)
    C = 16
    r = (torch.randn(3, C, *hw, generator=g, dtype=torch.float64) * 0.5 + torch.randn(1, C, 1, 1, generator=g, dtype=torch.float64))
    r.requires_grad_(True)
    ps = [(1.0 + 0.1 * torch.randn(C // 2, generator=g, dtype=torch.float64)).requires_grad_(True) for _ in range(4)]
    gi, bi, gb, bb = ps
    dy = torch.randn(3, C, *hw, generator=g, dtype=torch.float64)
    pre = O.ibn_relu_forward(r, gi, bi, gb, bb)
    want = torch.autograd.grad(torch.relu(pre), [r, gi, bi, gb, bb], dy)
    got = O.ibn_relu_bwd_closed_form(r.detach(), dy, pre.detach() > 0, gi.detach(), gb.detach())
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) < 1e-12
    if hw == (1, 1):                    # one pixel: the instance-norm half passes no gradient
        assert float(got[0][:, :C // 2].abs().max()) == 0.0


def test_forced_masks_and_bf16_emulation():
    tag, sd, x, dout = block_state(64, 128, 1)
    free = O.block_reference(x, sd, 1, dout, torch.float64)
    masks = {"relu1": free["pre1"] > 0, "relu2": free["pre2"] > 0}
    forced = O.block_reference(x, sd, 1, dout, torch.float64, masks=masks)
    assert torch.equal(forced["out"], free["out"]) and torch.equal(forced["dx"], free["dx"])
    emul = O.block_reference(x, sd, 1, dout, torch.float64, bf16=True)
    assert torch.equal(emul["out"], emul["out"].to(torch.bfloat16).double())           # stored in bf16
    e = relerr(emul["out"], free["out"])
    assert 1e-4 < e < 3e-2, e                                                           # bf16 storage noise, nothing larger


def test_trunk_forced_masks_of_its_own_free_run_change_nothing():
    """trunk_reference with the signs of its own free fp64 run forced on all sixteen ReLUs is the free run bit for bit"""
    sd, x, dh = O.trunk_case(6, 7)
    free = O.trunk_reference(x, sd, dh, torch.float64)
    assert set(free["blocks"]) == {p for p, _ in O.LAYERS}
    masks = {p: {"relu1": b["pre1"] > 0, "relu2": b["pre2"] > 0} for p, b in free["blocks"].items()}
    forced = O.trunk_reference(x, sd, dh, torch.float64, masks=masks)
    assert torch.equal(forced["h"], free["h"]) and torch.equal(forced["dx"], free["dx"])
    assert set(forced["grads"]) == set(free["grads"]) and set(forced["running"]) == set(free["running"])
    for k, g in free["grads"].items():
        assert torch.equal(forced["grads"][k], g), k
    for k, v in free["running"].items():
        assert torch.equal(forced["running"][k], v), k
    for p, b in free["blocks"].items():
        for k in ("pre1", "pre2", "out"):
            assert torch.equal(forced["blocks"][p][k], b[k]), (p, k)
    with pytest.raises(ValueError, match="eight prefixes"):
        O.trunk_reference(x, sd, dh, torch.float64, masks={"layer1.0.": masks["layer1.0."]})


@pytest.mark.parametrize("hw", O.TRUNK_MAPS, ids=lambda s: "%dx%d" % s)
def test_trunk_inputs_keep_the_relu_band_thin(hw):
    """the inputs of the GPU trunk tests: in the fp64 run, each of the sixteen pre-activations has at most the cap's share of its
    elements within the band around zero in which a kernel's mask bit may differ (BAND: fp32 1e-4 of the rms, cap 1e-3; bf16 2^-5 of
    the rms, cap 5e-2). A share above its cap is answered by another input seed, never by another cap."""
    sd, x, dh = O.trunk_case(*hw)
    with torch.no_grad():
        s = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
        t, pres = x.double(), []
        for prefix, stride in O.LAYERS:
            res = O.block_forward(t, O.sub_state(s, prefix), stride)
            t = res["out"]
            pres += [(prefix + "relu1", res["pre1"]), (prefix + "relu2", res["pre2"])]
    assert len(pres) == 16
    for dt, (thr, cap) in O.BAND.items():
        shares = {name: O.band_share(pre, thr)[0] for name, pre in pres}
        worst = max(shares, key=shares.get)
        print(f"  {hw[0]}x{hw[1]} {dt}: worst share within the band {shares[worst]:.2e} ({worst}), cap {cap:g}")
        assert shares[worst] <= cap, (dt, worst, shares[worst])


@pytest.mark.parametrize("shape", [(128, 64, 3), (256, 128, 1)], ids=lambda s: "Co%dC%dk%d" % s)
def test_backward_weight_packing(lib, shape):
    from neuralsampleid_amd import ops
    Co, C, k = shape
    w = torch.randn(Co, C, k, k, generator=torch.Generator().manual_seed(Co + k))
    wt = ops.pack_conv_bwd(w)
    assert wt.shape == (C, k * k * Co) and wt.is_contiguous()
    assert torch.equal(wt.view(C, k, k, Co).permute(3, 0, 1, 2), w)
    dwp = torch.randn(Co, k * k * C, generator=torch.Generator().manual_seed(1))
    assert torch.equal(ops.unpack_conv_wgrad(dwp, C, k), dwp.view(Co, k, k, C).permute(0, 3, 1, 2))
    assert torch.equal(ops.pack_conv_bn(ops.unpack_conv_wgrad(dwp, C, k))[0], dwp)      # the forward's layout


def test_new_ops_refuse_cpu_tensors(lib):
    from neuralsampleid_amd import ops
    x = torch.zeros(20, 128)
    f = torch.zeros(64)
    aff = ops.BNAffine(f, f, f, f)
    calls = [lambda: ops.conv2d_bwd_data(x, 1, 4, 5, 128, torch.zeros(128, 9 * 128), 128, 3, 1),
             lambda: ops.conv2d_bwd_weight(x, x, torch.zeros(128, 9 * 128), 1, 4, 5, 128, 128, 3, 1),
             lambda: ops.col_stat(x, 20, 128),
             lambda: ops.ibn_relu_bwd(x, x, 1, 20, 128, f, f, aff, f, f, f, f),
             lambda: ops.bn_add_relu_fwd(x, ops.BNAffine(torch.zeros(128), torch.zeros(128)), x),
             lambda: ops.relu_bwd(x, x)]
    for c in calls:
        with pytest.raises(RuntimeError, match="no CPU path"):
            c()


def test_workspace_of_the_new_ops(lib):
    from neuralsampleid_amd import _lib
    ws = _lib.lib.nsid_workspace_bytes
    M, welems = 8 * 21 * 54, 128 * 9 * 128
    splits = _lib.lib.nsid_conv2d_wgrad_splits(M, welems)
    assert 1 < splits <= 64 and ws(b"conv2d_bwd_weight", M, welems) == splits * welems * 4
    assert _lib.lib.nsid_conv2d_wgrad_splits(8 * 6 * 14, 1024 * 9 * 1024) == 1 and ws(b"conv2d_bwd_weight", 8 * 6 * 14, 1024 * 9 * 1024) == 0
    assert ws(b"ibn_relu_bwd", 3, 256) == (2 * 3 * 256 + 256) * 4
    for op in (b"conv2d_bwd_data", b"col_stat", b"bn_add_relu", b"relu_bwd"):
        assert ws(op, 1000, 128) == 0


def test_training_mode_forward_still_raises_and_train_rows_needs_the_gpu(lib):
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN, ResidualBlock, ResidualIBN
    from neuralsampleid_amd.simclr.triplet import BaselineModel
    model = BaselineModel({}, ResNetIBN())
    with pytest.raises(NotImplementedError, match="eval"):
        model.train()(torch.zeros(1, 84, 216), torch.zeros(1, 84, 216))
    with pytest.raises(NotImplementedError, match="eval"):
        ResidualBlock(64, 128).train()(torch.zeros(1, 64, 4, 4))
    with pytest.raises(NotImplementedError, match="CPU"):
        ResidualIBN(64, 128).train_rows(torch.zeros(12, 64), 1, 3, 4)
    with pytest.raises(NotImplementedError, match="CPU"):
        model.encoder.trunk_train(torch.zeros(12, 64), 1, 3, 4)
