"""GPU: ResidualIBN.train_rows and ResNetIBN.trunk_train (encoder/resnet_ibn.py) against the fp64 oracle of
tests/resnet_train_oracle.py and the reference's goldens (tests/golden/make_resnet_train_golden.py).

A block is measured with the kernel's two ReLU masks forced on the oracle (a mask bit that differs at a pre-activation of rounding
size would otherwise move a gradient by a whole element), after a check that those masks are the fp64 masks wherever the fp64
pre-activation is further than 1e-4 (fp32) / 2^-5 (bf16) of its rms from zero, which may leave out at most 0.1 % / 5 % of the elements.
Bounds, relative L2 per tensor: fp32 20 x the oracle's own fp32-vs-fp64 distance (the margin test_model_fp32_vs_reference gives
stacked layers); bf16 4 x the deviation of the oracle's bf16-storage emulation from fp64 (as test_model_bf16_vs_reference). The
emulation runs in fp32 arithmetic, as the kernels do between their bf16 stores: in fp64 arithmetic it has no error at all in a
quantity that storage rounding does not reach (bn3.bias's gradient is a plain sum of the masked upstream gradient), and no fp32
accumulation can stay within a multiple of zero.
One floor deviates from that, under bf16 storage only: the gradient of bn3.bias (and of downsample.1.bias, which is the same sum) is
a plain sum of bf16-representable values, which torch's pairwise fp32 sum in the emulation gets nearly exact (measured floors 1.3e-9 and 2.5e-9
relative in the (64, 128, 1) and (128, 128, 1) cases at 6 x 7, against 1.0e-8 for the kernels, itself a sixth of fp32's 2^-24; the other seven
cases and the trunk pass without it). For these two tensors the floor is not taken below 2^-24,
half a unit in the last place of the fp32 format they are returned in; each use is printed. Every other tensor, and every tensor
under fp32 storage, has the bound as stated.
bn2.bias has an exactly zero gradient (a per-channel constant in front of conv3 is removed by bn3's mean subtraction): all sides hold
rounding noise there, which is measured against the norm of bn2.weight's gradient.

The trunk (test_trunk_vs_oracle) is measured the same way with all sixteen kernel masks forced on tests/resnet_train_oracle.py's
trunk_reference, each block's masks checked on the input that block really received, and every tensor compared: h, the gradient of
the input rows, every parameter gradient behind the stem, every running statistic and counter. Under bf16 storage the emulation
itself is 5-30 % from fp64 in the deep gradients (layer 4 normalises over 4 or 12 pixels), so there this bound only catches gross
errors; what pins the bf16 trunk is test_trunk_is_the_composition_of_its_blocks (the trunk against its own blocks run one at a time,
bit for bit wherever no atomics are involved) together with the block test over all eight (Cin, Cout, stride) of the model.

Measured multiples of the floor (worst tensor per case) are printed; DESIGN.md 3a records them."""
import copy

import pytest
import torch

import resnet_train_oracle as O
from compare import relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 3
# all eight (Cin, Cout, stride) of the model; (128, 128, 1) also at 11 x 13 = 429 rows, where conv2's weight gradient splits its rows
CASES = [(64, 128, 1, 6, 7), (128, 128, 1, 6, 7), (128, 128, 1, 11, 13), (128, 256, 1, 6, 7), (256, 256, 1, 6, 7), (256, 512, 2, 6, 7),
         (512, 512, 1, 6, 7), (512, 1024, 2, 11, 13), (1024, 1024, 1, 6, 7)]
BAND = O.BAND
MULT = {torch.float32: 20.0, torch.bfloat16: 4.0}
ULP32 = 2.0 ** -24


@pytest.fixture
def restore():
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops
    ops.set_gemm_precision("fp32")
    yield
    F_.set_activation_dtype(torch.float32)
    ops.set_gemm_precision("fp32")


def _rows(x4, dt):
    b, c, h, w = x4.shape
    return x4.permute(0, 2, 3, 1).reshape(b * h * w, c).to(dt).contiguous()


def _bchw(rows, b, h, w):
    return rows.detach().double().view(b, h, w, -1).permute(0, 3, 1, 2).cpu()


def _block(cin, cout, stride):
    from synth import synth_state
    from neuralsampleid_amd.encoder.resnet_ibn import ResidualIBN
    tag = f"c{cin}_{cout}_s{stride}"
    blk = ResidualIBN(cin, cout, stride)
    sd = synth_state(blk.state_dict(), prefix=tag + ".")
    blk.load_state_dict(sd)
    return tag, blk.to(DEV).train(), sd


def _kernel_mask1(blk, rows, H, W):
    """the mask of the block's first ReLU as the kernels compute it: conv1, the BatchNorm half's batch statistics, IBN + ReLU"""
    from neuralsampleid_amd import ops
    cin, cout = blk.conv1.in_channels, blk.conv1.out_channels
    M, half = rows.shape[0], cout // 2
    with torch.no_grad():
        r1, _ = ops.linear_fwd(rows, ops.w2d(blk.conv1.weight), None, M, cout, cin)
        bn = blk.bn1.BN
        aff = ops.bn_finalize(ops.col_stat(r1[:, half:], M, cout - half), M, bn.weight, bn.bias, None, None, None, bn.momentum, bn.eps)
        y1 = ops.ibn_relu_fwd(r1, B, H * W, cout, blk.bn1.IN.weight, blk.bn1.IN.bias, aff, blk.bn1.IN.eps)
    return _bchw(y1, B, H, W) > 0


def _run_block(blk, x, dout, dt, H, W):
    """-> dict(out, dx, grads, running, nbt, masks) of one train_rows call and its backward"""
    rows = _rows(x, dt).to(DEV).requires_grad_(True)
    mask1 = _kernel_mask1(blk, rows.detach(), H, W)
    out, Ho, Wo = blk.train_rows(rows, B, H, W)
    assert out.dtype == dt and tuple(out.shape) == (B * Ho * Wo, blk.conv1.out_channels)
    out.backward(_rows(dout, dt).to(DEV))
    sd = blk.state_dict()
    return dict(out=_bchw(out, B, Ho, Wo), dx=_bchw(rows.grad, B, H, W), hw=(Ho, Wo),
                grads={k: p.grad.detach().double().cpu() for k, p in blk.named_parameters()},
                running={k: v.double().cpu() for k, v in sd.items() if k.endswith(("running_mean", "running_var"))},
                nbt=[int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")],
                masks={"relu1": mask1, "relu2": _bchw(out, B, Ho, Wo) > 0})


def _check_masks(got, free64, dt):
    thr, cap = BAND[dt]
    for name, pre in (("relu1", free64["pre1"]), ("relu2", free64["pre2"])):
        share, clear = O.band_share(pre, thr)
        flips = int((got["masks"][name] != (pre > 0)).sum())
        print(f"  {name}: {share:.2e} of the elements within the band, {flips} mask bits differ from fp64")
        assert torch.equal(got["masks"][name][clear], (pre > 0)[clear]), name
        assert share <= cap, (name, share)


def _compare(got, ref64, floor_ref, mult, what, half_ulp=False, first="out"):
    """every tensor of `got` (first, dx, grads, running) against ref64 within mult x the distance of floor_ref from ref64; names
    may carry a block prefix (the trunk); returns the worst multiple"""
    worst, bad = 0.0, []

    def one(name, a, r, f):
        nonlocal worst
        if name.endswith("bn2.bias"):             # an exactly zero gradient: noise, against the norm of that block's bn2.weight gradient
            wnorm64 = float(ref64["grads"][name[len("grad."):-len("bias")] + "weight"].norm())
            err, floor = float((a - r).norm()) / wnorm64, float((f.double() - r).norm()) / wnorm64
        else:
            err, floor = relerr(a, r), relerr(f, r)
            if half_ulp and name.endswith(("bn3.bias", "downsample.1.bias")) and err > mult * floor:
                print(f"  {what} {name}: rel {err:.3e} exceeds {mult:g} x the emulation's {floor:.3e}: NEEDS the half-ulp floor {ULP32:.3e}")
                floor = max(floor, ULP32)
        m = err / max(floor, 1e-30)
        worst = max(worst, m)
        print(f"  {what} {name}: rel {err:.3e} = {m:.2f} x the floor {floor:.3e} (allowed {mult:g} x)")
        if not err <= mult * floor:
            bad.append((name, err, floor))

    assert set(got["grads"]) == set(ref64["grads"]) and set(got["running"]) == set(ref64["running"])
    one(first, got[first], ref64[first], floor_ref[first])
    one("dx", got["dx"], ref64["dx"], floor_ref["dx"])
    for k, r in ref64["grads"].items():
        one("grad." + k, got["grads"][k], r, floor_ref["grads"][k])
    for k, r in ref64["running"].items():
        one(k, got["running"][k], r, floor_ref["running"][k])
    print(f"  {what}: worst multiple of the floor {worst:.2f}")
    assert not bad, bad
    return worst


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "c%d_%d_s%d_%dx%d" % c)
def test_block_train_vs_oracle(case, dt, restore):
    from synth import synth_randn
    cin, cout, stride, H, W = case
    tag, blk, sd = _block(cin, cout, stride)
    assert (blk.downsample is None) == (cin == cout and stride == 1)
    x = synth_randn(f"{tag}_{H}x{W}", B, cin, H, W)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dout = synth_randn(f"{tag}_{H}x{W}_dout", B, cout, Ho, Wo)
    got = _run_block(blk, x, dout, dt, H, W)
    assert got["hw"] == (Ho, Wo) and got["nbt"] == [1] * len(got["nbt"]) and len(got["nbt"]) == (4 if blk.downsample is not None else 3)
    bf = dt == torch.bfloat16
    xin = x.to(dt).double()                      # the stored input is the oracle's input
    print(f"block {tag} {H}x{W} {dt}")
    _check_masks(got, O.block_reference(xin, sd, stride, dout.to(dt), torch.float64), dt)
    ref64 = O.block_reference(xin, sd, stride, dout.to(dt), torch.float64, masks=got["masks"])
    if bf:
        floor_ref = O.block_reference(xin, sd, stride, dout, torch.float32, bf16=True, masks=got["masks"])
    else:
        floor_ref = O.block_reference(xin, sd, stride, dout, torch.float32, masks=got["masks"])
    _compare(got, ref64, floor_ref, MULT[dt], f"{tag} {dt}", half_ulp=bf)
    # a second block with the same state gives the same bits where no atomics are involved: output and running statistics
    _, blk2, _ = _block(cin, cout, stride)
    out2, _, _ = blk2.train_rows(_rows(x, dt).to(DEV), B, H, W)
    assert torch.equal(_bchw(out2, B, Ho, Wo), got["out"])


@pytest.mark.parametrize("blk", [(64, 128, 1), (128, 256, 2)], ids=lambda b: "c%d_%d_s%d" % b)
def test_block_train_vs_reference_golden(golden, blk, restore):
    """fp32 storage against the reference's own fp64 run: its masks must be the kernel's at these inputs (then forcing changes nothing)"""
    from synth import synth_randn
    cin, cout, stride = blk
    H, W = 6, 7
    tag, mod, sd = _block(cin, cout, stride)
    gold = golden("resnet_train_" + tag)
    x = synth_randn(tag, B, cin, H, W)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dout = synth_randn(tag + "_dout", B, cout, Ho, Wo)
    got = _run_block(mod, x, dout, torch.float32, H, W)
    ref64 = O.block_reference(x, sd, stride, dout, torch.float64)
    ref32 = O.block_reference(x, sd, stride, dout, torch.float32)
    for name, pre in (("relu1", ref64["pre1"]), ("relu2", ref64["pre2"])):
        assert torch.equal(got["masks"][name], pre > 0), f"{name}: a mask bit differs from the reference's at these inputs"
    assert got["nbt"] == list(gold["nbt"])
    wnorm = gold.t("grad.bn2.weight").norm()
    for name, a, f in ([("out", got["out"], ref32["out"]), ("dx", got["dx"], ref32["dx"])]
                       + [("grad." + k, got["grads"][k], ref32["grads"][k]) for k in ref64["grads"]]
                       + [("state." + k, got["running"][k], ref32["running"][k]) for k in ref64["running"]]):
        g = gold.t(name)
        if name == "grad.bn2.bias":
            r = ref64["grads"]["bn2.bias"]
            err, floor = float((a - r).norm()) / wnorm, float((f.double() - r).norm()) / wnorm
        else:
            err, floor = relerr(a, g), relerr(f, g)
        print(f"  golden {tag} {name}: rel {err:.3e}, allowed 20 x {floor:.3e}")
        assert err <= 20.0 * floor, (name, err, floor)


def _trunk_model(p=2.5):
    from synth import synth_state
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    model = ResNetIBN()
    sd = synth_state(model.state_dict())
    sd["global_pool.p"] = torch.full((1,), p)
    model.load_state_dict(sd)
    return model.to(DEV), sd


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_trunk_train(dt, restore):
    from synth import synth_randn
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    F_.set_activation_dtype(dt)
    model, sd = _trunk_model()
    H, W = 6, 7
    x = synth_randn("trunk_train", B, 64, H, W).abs()              # like the stem's output: behind a ReLU and a max-pool
    dh = synth_randn("trunk_train_dh", B, 2048) / 32
    clip = synth_randn("trunk_train_clip", 2, 84, 100).abs().to(DEV) * 2
    with torch.no_grad():
        h_before = model.eval()(clip).clone()
    model.train()
    rows = _rows(x, dt).to(DEV).requires_grad_(True)
    h = model.trunk_train(rows, B, H, W)
    assert tuple(h.shape) == (B, 2048) and h.dtype == torch.float32
    h.backward(dh.to(DEV))
    for k in ("conv1.weight", "bn1.weight", "bn1.bias"):           # the stem has no backward; everything behind it: test_trunk_vs_oracle
        assert model.get_parameter(k).grad is None, k
    bf = dt == torch.bfloat16
    xin = x.to(dt).double()
    ref64 = O.trunk_reference(xin, sd, dh, torch.float64)
    floor_ref = O.trunk_reference(xin, sd, dh, torch.float32, bf16=True) if bf else O.trunk_reference(xin, sd, dh, torch.float32)
    mult = MULT[dt]
    for name, a, r, f in (("h", h, ref64["h"], floor_ref["h"]),
                          ("d global_pool.p", model.global_pool.p.grad, ref64["grads"]["global_pool.p"], floor_ref["grads"]["global_pool.p"])):
        err, floor = relerr(a.detach().cpu(), r), relerr(f, r)
        print(f"  trunk {dt} {name}: rel {err:.3e} = {err / max(floor, 1e-30):.2f} x the floor {floor:.3e} (allowed {mult:g} x)")
        assert err <= mult * floor, (name, err, floor)
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == (0 if k == "bn1.num_batches_tracked" else 1), k
    # eval-mode extraction sees the updated running statistics, and is what a fresh model with this state computes
    with torch.no_grad():
        h_after = model.eval()(clip).clone()
        fresh = ResNetIBN().to(DEV)
        fresh.load_state_dict(model.state_dict())
        h_fresh = fresh.eval()(clip)
    assert not torch.equal(h_after, h_before) and relerr(h_after.cpu(), h_before.cpu()) > 1e-3
    assert torch.equal(h_after, h_fresh)


# ---------------------------------------------------------------------------------------------- the whole trunk, every tensor
ROW_GEMM_WGRAD = ("conv1.weight", "conv3.weight", "layer1.0.downsample.0.weight", "layer2.0.downsample.0.weight")


def _blocks_of(model):
    return [(prefix, stride, model.get_submodule(prefix[:-1])) for prefix, stride in O.LAYERS]


def _first_pass(model, rows, H, W):
    """the eight blocks, in order, on a copy of the model (the model under test keeps its statistics): per block its stored input
    rows, their map, the two kernel masks and the output rows; then the head -> (blocks, h)"""
    walk, blocks = copy.deepcopy(model).train(), []
    with torch.no_grad():
        for prefix, stride, blk in _blocks_of(walk):
            mask1 = _kernel_mask1(blk, rows, H, W)
            out, Ho, Wo = blk.train_rows(rows, B, H, W)
            blocks.append(dict(prefix=prefix, stride=stride, x=rows, hw=(H, W), out=out, hwo=(Ho, Wo),
                               masks={"relu1": mask1, "relu2": _bchw(out, B, Ho, Wo) > 0}))
            rows, H, W = out, Ho, Wo
        h = walk.head_train(rows, B, H * W)
    return blocks, h, walk


def _trunk_run(model, rows, dh, H, W):
    """trunk_train and its backward on the model under test -> dict(h, head_rows, dx, grads, running, nbt); head_rows are the rows
    the head received (the last block's output)"""
    seen, head_train = {}, model.head_train

    def spy(r, b, hw):
        seen["rows"] = r.detach()
        return head_train(r, b, hw)
    model.head_train = spy
    try:
        h = model.trunk_train(rows, B, H, W)
    finally:
        del model.head_train
    assert tuple(h.shape) == (B, 2048) and h.dtype == torch.float32
    h.backward(dh)
    sd = model.state_dict()
    return dict(h=h.detach(), head_rows=seen["rows"], dx=rows.grad,
                grads={k: p.grad.detach() for k, p in model.named_parameters() if p.grad is not None},
                running={k: v.clone() for k, v in sd.items() if k.endswith(("running_mean", "running_var"))},
                nbt={k: int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")})


def _trunk_setup(dt, hw):
    from neuralsampleid_amd import functional as F_
    F_.set_activation_dtype(dt)
    H, W = hw
    sd, x, dh = O.trunk_case(H, W)
    model, sd_model = _trunk_model()
    assert all(torch.equal(sd[k], v) for k, v in sd_model.items())
    rows = _rows(x, dt).to(DEV).requires_grad_(True)
    return model.train(), sd, x, dh, rows


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hw", O.TRUNK_MAPS, ids=lambda s: "%dx%d" % s)
def test_trunk_vs_oracle(hw, dt, restore):
    """every tensor trunk_train and its backward produce against the fp64 oracle with the sixteen kernel masks forced. 6 x 7: every
    launch a single 128-row tile, layer 4 on 2 x 2; 11 x 13: 429 rows in layers 1-2 (several row tiles, a ragged last one, conv2's
    weight gradient split in two), layer 3 on 6 x 7, layer 4 on 3 x 4.
    The masks are the kernels' own, checked per block on the input that block really received (a free fp64 run of that block: equal
    outside the band, the share inside within the cap): under bf16 storage a deep block's input is further from a trunk-wide fp64
    run's than the band is wide.
    The first pass runs on a copy, so the model under test moves its statistics once; the run under test must repeat the first
    pass's rows into the head bit for bit (no kernel of the eight blocks accumulates with atomics in the forward). h itself is the
    head's split-K product (ResNetIBN.head_train: four partial sums per element meet in fp32 atomics), so it repeats to the
    summation-order bound tests/test_reproducible_gpu.py gives atomics (1e-5 of the largest entry); the number of differing
    elements is printed."""
    H, W = hw
    model, sd, x, dh, rows = _trunk_setup(dt, hw)
    bf = dt == torch.bfloat16
    blocks, h_first, walk = _first_pass(model, rows.detach(), H, W)
    got = _trunk_run(model, rows, dh.to(DEV), H, W)
    print(f"trunk {H}x{W} {dt}")
    # a. the run under test is the first pass again
    assert torch.equal(got["head_rows"], blocks[-1]["out"]), "the rows into the head differ from the first pass's"
    ndiff = int((got["h"] != h_first).sum())
    print(f"  h: {ndiff} of {h_first.numel()} elements differ from the first pass's (split-K atomics in the head)")
    assert float((got["h"] - h_first).abs().max()) <= 1e-5 * float(h_first.abs().max())
    walked = walk.state_dict()
    for k, v in got["running"].items():
        assert torch.equal(v, walked[k]), k
    # the masks, per block, on the input the block received
    kmasks = {}
    s64 = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    for b in blocks:
        xin = _bchw(b["x"], B, *b["hw"])
        with torch.no_grad():
            free64 = O.block_forward(xin, O.sub_state(s64, b["prefix"]), b["stride"])
        print(f" {b['prefix']} on {b['hw'][0]}x{b['hw'][1]}")
        _check_masks(b, free64, dt)
        kmasks[b["prefix"]] = b["masks"]
    # b. values
    xin = x.to(dt).double()
    ref64 = O.trunk_reference(xin, sd, dh, torch.float64, masks=kmasks)
    floor_ref = O.trunk_reference(xin, sd, dh, torch.float32, bf16=bf, masks=kmasks)
    cpu = lambda t: t.detach().double().cpu()
    res = dict(h=cpu(got["h"]), dx=_bchw(got["dx"], B, H, W), grads={k: cpu(v) for k, v in got["grads"].items()},
               running={k: cpu(v) for k, v in got["running"].items() if not k.startswith("bn1.")})
    _compare(res, ref64, floor_ref, MULT[dt], f"trunk {H}x{W} {dt}", half_ulp=bf, first="h")
    # the stem is not part of the trunk: its statistics and counter stay, every other counter moved once
    assert torch.equal(got["running"]["bn1.running_mean"].cpu(), sd["bn1.running_mean"])
    assert torch.equal(got["running"]["bn1.running_var"].cpu(), sd["bn1.running_var"])
    assert len(got["nbt"]) == 1 + len(ref64["running"]) // 2
    for k, v in got["nbt"].items():
        assert v == (0 if k == "bn1.num_batches_tracked" else 1), k


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hw", O.TRUNK_MAPS, ids=lambda s: "%dx%d" % s)
def test_trunk_is_the_composition_of_its_blocks(hw, dt, restore):
    """trunk_train against the head and the eight blocks run one at a time, from layer4.1 down to layer1.0, on fresh modules with
    the same initial state: each on a cloned leaf of the input it had in the trunk, with the dx of the module above as its upstream
    gradient. With every block configuration checked against fp64 (test_block_train_vs_oracle), this pins the trunk under bf16
    storage as tightly as a block, and a block that writes into a tensor a neighbour saved shows as a difference.
    Bit for bit: the input gradient, every BatchNorm / IBN gradient, conv2.weight, the stride-2 downsample.0.weight, global_pool.p,
    embedding_head.bias (one row tile: a single addition onto zero) and embedding_head.weight (fp32, three rows: one split). The
    row-GEMM weight gradients of the blocks (conv1, conv3, the stride-1 downsamples) add their row splits with atomics: under fp32
    storage 429 rows or fewer are ONE split (csrc/gemm.hip: splits of 512 rows), a single addition onto zero, so they are bit for
    bit as well; under bf16 storage they agree to the bound test_weight_gradients_repeat_to_atomics_noise gives that kernel
    (1e-5 of the largest entry).
    fp32-storage backward-data GEMMs with a reduction of 1024 or more and a handful of tiles (the head's, layer 4's) split their
    reduction into fp32 atomics by default (tuning key bwd_split_max_tiles); that changes the last bit of everything below them from
    run to run, so both sides of this comparison run with the split off. test_trunk_vs_oracle runs the default dispatch."""
    from neuralsampleid_amd import ops
    H, W = hw
    model, sd, x, dh, rows = _trunk_setup(dt, hw)
    dh = dh.to(DEV)
    parts = copy.deepcopy(model).train()
    blocks, _, _ = _first_pass(model, rows.detach(), H, W)
    ops.set_tuning("bwd_split_max_tiles", 0)
    try:
        got = _trunk_run(model, rows, dh, H, W)
        Hl, Wl = blocks[-1]["hwo"]
        leaf = blocks[-1]["out"].clone().requires_grad_(True)
        parts.head_train(leaf, B, Hl * Wl).backward(dh)
        up = leaf.grad
        for b, (prefix, stride, blk) in zip(reversed(blocks), reversed(_blocks_of(parts))):
            leaf = b["x"].clone().requires_grad_(True)
            out, _, _ = blk.train_rows(leaf, B, *b["hw"])
            assert torch.equal(out, b["out"]), prefix
            out.backward(up)
            up = leaf.grad
    finally:
        ops.reset_tuning()
    alone = {k: p.grad for k, p in parts.named_parameters() if p.grad is not None}
    assert set(alone) == set(got["grads"])
    print(f"trunk against its blocks {H}x{W} {dt}")
    assert torch.equal(got["dx"], up), "the gradient of the input rows"
    nexact = 0
    for k, g in got["grads"].items():
        if dt == torch.bfloat16 and k.endswith(ROW_GEMM_WGRAD):
            d, top = float((g - alone[k]).abs().max()), float(alone[k].abs().max())
            print(f"  {k}: max |difference| {d:.3e} = {d / top:.2e} of the largest entry (allowed 1e-5)")
            assert d <= 1e-5 * top, k
        else:
            nexact += 1
            assert torch.equal(g, alone[k]), k
    print(f"  {nexact} of {len(alone)} parameter gradients and the input gradient are bit for bit the blocks' own")
