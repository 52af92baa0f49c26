"""GPU: BaselineModel.train()(x_i, x_j) on the ResNet-IBN baseline (simclr/triplet.py, encoder/resnet_ibn.py): the whole training
forward and backward, on (3, 84, 100) pairs (layer 4 on 6 x 7), under both activation storages.

Composition (test_training_call_is_the_composition_of_its_parts): the call against the parts run by hand per view on a deep copy of
the model (the counters then agree): stem_train, trunk_train on the detached rows, l2norm, ops.stem7_bwd on rows.grad.
h is the head's split-K product (ResNetIBN.head_train: four partial sums per element meet in fp32 atomics, see test_trunk_vs_oracle),
so h and z of two runs agree to summation-order noise only: they are held to the bound tests/test_reproducible_gpu.py gives atomics,
1e-5 of the largest entry. That noise must not enter the backward comparison: under bf16 storage every stored gradient is rounded,
a last-bit difference at the top flips roundings below it, and forty storage points later the two runs differ by bf16 rounding noise
itself (measured: 9e-3 of the largest entry of conv1.weight's gradient when each side normalised its own h). So the hand side takes its
l2norm backward at the h of the call; both backward passes then start from the same bits. With that, bit for bit: the stem's rows
of both views, every BatchNorm's state, the three stem gradients (the sum of the two views; also against ops.stem7_bwd on the very
gradient the call's trunk handed down), and every other parameter gradient except the row-GEMM weight gradients (conv1, conv3, the
stride-1 downsamples), which add their row splits with atomics at 1 575 rows and are held to the 1e-5 bound as
test_trunk_is_the_composition_of_its_blocks holds them. Both sides run with the fp32 split of the deep backward-data GEMMs off, as
that test does.

Against the fp64 oracle (tests/stem_train_oracle.py: the stem oracle + resnet_train_oracle's blocks, free masks, view j on the running
statistics view i left): h_i and h_j within 20 x the fp32 oracle's distance from fp64 (fp32 storage) / 4 x the bf16 emulation's (bf16
storage); z rows of unit norm; every num_batches_tracked 2; bn1's running statistics after two updates within 20 x the fp32 oracle's
distance (they never pass through bf16).

Against the reference's golden (tests/golden/make_stem_train_golden.py) at (2, 84, 40), fp32 storage: h, z and the two loss parts
within 20 x the fp32 oracle's distance from the golden, the form of the bound test_block_train_vs_reference_golden uses (free masks at
this depth: the oracle's own fp32 run is the measure of what fp32 arithmetic can reach). The loss parts are scalars returned in fp32:
their floor is not taken below 2^-23, one unit in the last place.

One step: baseline_objective backward and a FusedClipAdam(ds_prep=False, direct_grads=False) step change every parameter, the next
eval forward sees the new weights, and ten steps on one fixed batch of 4 pairs at lr 1e-3 lower the loss. The lr was chosen on the CPU
with torch's fp32 oracle (tests/stem_train_oracle.py's encoder, torch.optim.Adam, clip_grad_norm_ at 1.0) on this batch: at 1e-3 its
loss goes 2.1486, 2.1758, 2.1602, 2.1537, 2.1493, 2.1471, 2.1463, 2.1462, 2.1461, 2.1460 (lower by 2.6e-3); at 1e-4 it ends at
2.1504 and at 3e-5 at 2.1476, so those were not taken. The synthesized model starts next to the collapsed plateau
log(2 B - 1) + margin = 2.1459 (all embeddings nearly parallel), and ten steps take it onto that plateau: the drop is small but three
orders above fp32 noise in the loss."""
import copy
import functools

import pytest
import torch

import stem_train_oracle as S
from compare import relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, H, W = 3, 84, 100
MULT = {torch.float32: 20.0, torch.bfloat16: 4.0}
DTYPES = pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
LR = 1e-3
ROW_GEMM_WGRAD = ("conv1.weight", "conv3.weight", "layer1.0.downsample.0.weight", "layer2.0.downsample.0.weight")


@pytest.fixture
def restore():
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops
    ops.set_gemm_precision("fp32")
    yield
    F_.set_activation_dtype(torch.float32)
    ops.set_gemm_precision("fp32")
    ops.reset_tuning()


@functools.lru_cache(maxsize=None)
def _state():
    from synth import synth_state
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    sd = synth_state(ResNetIBN().state_dict())
    sd["global_pool.p"] = torch.full((1,), 2.5)
    return sd


def _model(sd=None):
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    from neuralsampleid_amd.simclr.triplet import BaselineModel
    enc = ResNetIBN()
    enc.load_state_dict(_state() if sd is None else sd)
    return BaselineModel({}, enc).to(DEV).train()


def _pair(b=B, h=H, w=W, tag="baseline_train"):
    return S.stem_input(b, h, w, f"{tag}_i"), S.stem_input(b, h, w, f"{tag}_j")


@functools.lru_cache(maxsize=None)
def _oracles():
    x_i, x_j = _pair()
    sd = _state()
    return (S.baseline_forward(x_i, x_j, sd, torch.float64), S.baseline_forward(x_i, x_j, sd, torch.float32),
            S.baseline_forward(x_i, x_j, sd, torch.float32, bf16=True))


@DTYPES
def test_training_call_is_the_composition_of_its_parts(dt, restore):
    from synth import synth_randn
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.simclr.triplet import NORM_EPS
    F_.set_activation_dtype(dt)
    x_i, x_j = (t.to(DEV) for t in _pair())
    dz = [(synth_randn(f"baseline_train_dz{v}", B, 2048) / 32).to(DEV) for v in "ij"]
    whole, parts = _model(), _model()
    ops.set_tuning("bwd_split_max_tiles", 0)
    # the call, with the rows the stem handed to the trunk and the gradient the trunk handed back recorded per view
    seen, trunk_train = [], whole.encoder.trunk_train

    def spy(rows, *a):
        rec = {"rows": rows.detach()}
        rows.register_hook(lambda g: rec.__setitem__("drows", g.detach().clone()))
        seen.append(rec)
        return trunk_train(rows, *a)
    whole.encoder.trunk_train = spy
    try:
        h_i, h_j, z_i, z_j = whole(x_i, x_j)
    finally:
        del whole.encoder.trunk_train
    assert all(t.requires_grad and t.dtype == torch.float32 for t in (h_i, h_j, z_i, z_j))
    torch.autograd.backward([z_i, z_j], dz)
    # the parts, by hand, view after view
    enc = parts.encoder
    w49, hand, stem_sum = ops.w2d(enc.conv1.weight.detach()), [], None
    for x, d, hc in zip((x_i, x_j), dz, (h_i, h_j)):
        with torch.no_grad():
            stat, tiles, N = ops.stem7_stat(x, w49)
            aff = ops.bn_finalize(stat, N, enc.bn1.weight.detach(), enc.bn1.bias.detach(), None, None, None, tiles=tiles)
            rows, Hp, Wp = enc.stem_train(x)
        leaf = rows.detach().requires_grad_(True)
        h = enc.trunk_train(leaf, B, Hp, Wp)
        z, norm = ops.l2norm_fwd(h.detach(), NORM_EPS)
        zc, normc = ops.l2norm_fwd(hc.detach(), NORM_EPS)           # the backward starts at the h of the call (module docstring)
        h.backward(ops.l2norm_bwd(d, zc, normc, NORM_EPS))
        g = ops.stem7_bwd(leaf.grad, x, w49, aff, enc.bn1.weight.detach())
        stem_sum = [t.clone() for t in g] if stem_sum is None else [a + b for a, b in zip(stem_sum, g)]
        hand.append(dict(rows=rows, h=h.detach(), z=z, aff=aff))
    # bit for bit: the stem's rows, bn1's state, the stem gradients of the call from the gradient its own trunk handed down
    stem_names = ("conv1.weight", "bn1.weight", "bn1.bias")
    own = None
    for rec, hd, x in zip(seen, hand, (x_i, x_j)):
        assert torch.equal(rec["rows"], hd["rows"]) and rec["rows"].dtype == dt
        g = ops.stem7_bwd(rec["drows"], x, w49, hd["aff"], enc.bn1.weight.detach())
        own = [t.clone() for t in g] if own is None else [a + b for a, b in zip(own, g)]
    for name, g in zip(stem_names, own):
        assert torch.equal(whole.encoder.get_parameter(name).grad.reshape(-1), g.reshape(-1)), name
    sw, sp = whole.state_dict(), parts.state_dict()
    for k in sw:
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            assert torch.equal(sw[k], sp[k]), k
    # to summation-order noise: h, z, the row-GEMM weight gradients; everything else bit for bit
    def near(name, a, b):
        d, top = float((a - b).abs().max()), float(b.abs().max())
        print(f"  {name}: max |difference| {d:.3e} = {d / max(top, 1e-30):.2e} of the largest entry (allowed 1e-5)")
        assert d <= 1e-5 * top, name
    print(f"training call against its parts, {dt}")
    for name, a, b in (("h_i", h_i, hand[0]["h"]), ("h_j", h_j, hand[1]["h"]), ("z_i", z_i, hand[0]["z"]), ("z_j", z_j, hand[1]["z"])):
        near(name, a.detach(), b)
    gw = {k: p.grad for k, p in whole.encoder.named_parameters()}
    gp = {k: p.grad for k, p in parts.encoder.named_parameters()}
    assert all(g is not None for g in gw.values()) and all(gp[k] is not None for k in gp if k not in stem_names)
    for name, g in zip(stem_names, stem_sum):
        assert torch.equal(gw[name].reshape(-1), g.reshape(-1)), name
    nexact, inexact = 3, []
    for k, g in gw.items():
        if k in stem_names:
            continue
        if k.endswith(ROW_GEMM_WGRAD):
            near("grad." + k, g, gp[k])
        elif torch.equal(g, gp[k]):
            nexact += 1
        else:
            inexact.append(k)
    print(f"  {nexact} of {len(gw)} parameter gradients are bit for bit the parts' own")
    assert not inexact, inexact


@DTYPES
def test_training_call_vs_oracle_and_eval_after_it(dt, restore):
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    F_.set_activation_dtype(dt)
    bf = dt == torch.bfloat16
    ref64, ref32, emul = _oracles()
    floor_ref = emul if bf else ref32
    x_i, x_j = (t.to(DEV) for t in _pair())
    model = _model()
    clip = S.stem_input(2, 84, 100, "baseline_train_clip").to(DEV)
    with torch.no_grad():
        h_before = model.eval()(clip, clip)[0].clone()
    h_i, h_j, z_i, z_j = model.train()(x_i, x_j)
    print(f"training call against the fp64 oracle, {dt}")
    bad = []
    for name, a, mult, fl in (("h_i", h_i, MULT[dt], floor_ref), ("h_j", h_j, MULT[dt], floor_ref)):
        err, floor = relerr(a.detach().double().cpu(), ref64[name]), relerr(fl[name].double(), ref64[name])
        print(f"  {name}: rel {err:.3e} = {err / floor:.2f} x the floor {floor:.3e} (allowed {mult:g} x)")
        if not err <= mult * floor:
            bad.append((name, err, floor))
    sd = model.state_dict()
    for k in ("bn1.running_mean", "bn1.running_var"):
        a, r, f = sd["encoder." + k].double().cpu(), ref64["state"][k], ref32["state"][k].double()
        err, floor = relerr(a, r), relerr(f, r)
        print(f"  {k}: rel {err:.3e} = {err / floor:.2f} x the floor {floor:.3e} (allowed 20 x)")
        if not err <= 20.0 * floor:
            bad.append((k, err, floor))
    assert not bad, bad
    for z in (z_i, z_j):
        assert float((z.detach().double().norm(dim=1) - 1).abs().max()) < 1e-6
    nbt = [int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")]
    assert len(nbt) == 29 and set(nbt) == {2}
    # eval after the training call: the running statistics are seen, and a fresh model with this state computes the same
    with torch.no_grad():
        h_after = model.eval()(clip, clip)[0].clone()
        fresh = _model(model.encoder.state_dict())
        h_fresh = fresh.eval()(clip, clip)[0]
    assert relerr(h_after.cpu(), h_before.cpu()) > 1e-3
    assert torch.equal(h_after, h_fresh)


def test_training_call_vs_reference_golden(golden, restore):
    import baseline_loss_oracle as L
    from synth import synth_state
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    from neuralsampleid_amd.simclr.triplet import baseline_objective
    gold = golden("stem_train_golden")
    sd = synth_state(ResNetIBN().state_dict())
    x_i, x_j = S.stem_input(2, 84, 40, "stem_train_golden_i"), S.stem_input(2, 84, 40, "stem_train_golden_j")
    ref32 = S.baseline_forward(x_i, x_j, sd, torch.float32)
    model = _model(sd)
    h_i, h_j, z_i, z_j = model(x_i.to(DEV), x_j.to(DEV))
    loss, cls, trip = baseline_objective(z_i, z_j, margin=0.2)
    bad = []
    for name, a in (("h_i", h_i), ("h_j", h_j), ("z_i", z_i), ("z_j", z_j)):
        err, floor = relerr(a.detach().double().cpu(), gold.t(name)), relerr(ref32[name].double(), gold.t(name))
        print(f"  golden {name}: rel {err:.3e}, allowed 20 x {floor:.3e}")
        if not err <= 20.0 * floor:
            bad.append((name, err, floor))
    obj32 = L.objective64(ref32["z_i"], ref32["z_j"], margin=0.2)
    for name, a, f, g in (("loss_cls", cls, obj32["cls"], gold["loss"][0]), ("loss_trip", trip, obj32["trip"], gold["loss"][1])):
        err, floor = abs(float(a) - float(g)) / float(g), max(abs(float(f) - float(g)) / float(g), 2.0 ** -23)
        print(f"  golden {name}: rel {err:.3e}, allowed 20 x {floor:.3e}")
        if not err <= 20.0 * floor:
            bad.append((name, err, floor))
    assert not bad, bad
    assert [int(v) for k, v in model.state_dict().items() if k.endswith("num_batches_tracked")] == list(gold["nbt"])


@DTYPES
def test_one_step_changes_every_parameter_and_ten_lower_the_loss(dt, restore):
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.optim import FusedClipAdam
    from neuralsampleid_amd.simclr.triplet import baseline_objective
    F_.set_activation_dtype(dt)
    direct = F_.DIRECT_GRADS
    model = _model()
    x_i, x_j = (t.to(DEV) for t in _pair(4, 84, 100, "baseline_step"))
    clip = S.stem_input(2, 84, 100, "baseline_train_clip").to(DEV)
    with torch.no_grad():
        h0 = model.eval()(clip, clip)[0].clone()
    model.train()
    opt = FusedClipAdam(model.parameters(), lr=LR, max_norm=1.0, direct_grads=False, ds_prep=False)
    assert F_.DIRECT_GRADS == direct
    conv2 = {p.data_ptr() for k, p in model.named_parameters() if k.endswith("conv2.weight")}
    assert len(conv2) == 8 and not conv2 & set(ops.DS_PREP.entries)      # ds_prep=False: the Downsample preparation holds none of them
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    losses = []
    for step in range(10):
        opt.zero_grad()
        _, _, z_i, z_j = model(x_i, x_j)
        loss, cls, trip = baseline_objective(z_i, z_j, margin=0.2)
        loss.backward()
        opt.step()
        losses.append(float(loss))
        if step == 0:
            same = [k for k, p in model.named_parameters() if torch.equal(p.detach(), before[k])]
            assert not same, same
            assert float(opt.grad_norm) > 0
            with torch.no_grad():
                h1 = model.eval()(clip, clip)[0].clone()
                fresh = _model(model.encoder.state_dict())
                assert torch.equal(fresh.eval()(clip, clip)[0], h1)         # the folded / packed weight caches were refreshed
            model.train()
            assert not torch.equal(h1, h0)
    print(f"  ten steps on one batch, {dt}: loss " + " ".join(f"{v:.4f}" for v in losses))
    assert all(v == v for v in losses) and losses[-1] < losses[0]
