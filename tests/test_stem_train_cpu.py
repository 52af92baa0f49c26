"""CPU: the training-mode stem oracle (tests/stem_train_oracle.py) composed with the trunk oracle pinned to the reference's golden of
one whole training call (tests/golden/make_stem_train_golden.py), the closed form of the stem backward pinned to autograd, the band
condition of the GPU tests' inputs, the refusals of the new ops and their workspace entries."""
import pytest
import torch

import stem_train_oracle as S
from compare import relerr


@pytest.fixture(scope="module")
def lib():
    from neuralsampleid_amd.build import build_lib
    return build_lib(verbose=False)


def golden_case():
    from synth import synth_state
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    sd = synth_state(ResNetIBN().state_dict())
    return sd, S.stem_input(2, 84, 40, "stem_train_golden_i"), S.stem_input(2, 84, 40, "stem_train_golden_j")


def test_oracle_matches_the_reference_golden(golden):
    """both views through the stem oracle + the trunk oracle's blocks in fp64, the running statistics updated view after view, the
    gradient of the reference's two losses (tests/baseline_loss_oracle.py) by autograd"""
    import baseline_loss_oracle as L
    gold = golden("stem_train_golden")
    sd, x_i, x_j = golden_case()
    res = S.baseline_forward(x_i, x_j, sd, torch.float64, grad=True)
    obj = L.objective64(res["z_i"].detach(), res["z_j"].detach(), margin=0.2)
    B = x_i.shape[0]
    names = ("conv1.weight", "bn1.weight", "bn1.bias", "embedding_head.bias", "global_pool.p")
    grads = torch.autograd.grad([res["z_i"], res["z_j"]], [res["params"][k] for k in names], [obj["dz"][:B], obj["dz"][B:]])
    errs = {k: relerr(res[k].detach(), gold.t(k)) for k in ("h_i", "h_j", "z_i", "z_j")}
    errs.update({"grad." + k: relerr(g, gold.t("grad." + k)) for k, g in zip(names, grads)})
    errs.update({"state." + k: relerr(res["state"][k], gold.t("state." + k)) for k in ("bn1.running_mean", "bn1.running_var")})
    errs["loss_cls"] = abs(float(obj["cls"]) - float(gold["loss"][0])) / float(gold["loss"][0])
    errs["loss_trip"] = abs(float(obj["trip"]) - float(gold["loss"][1])) / float(gold["loss"][1])
    for k, e in errs.items():
        print(f"  {k}: rel {e:.2e}")
    assert max(errs.values()) < 1e-9, errs
    nbt = [int(v) for k, v in res["state"].items() if k.endswith("num_batches_tracked")]
    assert nbt == list(gold["nbt"]) and set(nbt) == {2} and len(nbt) == 29


@pytest.mark.parametrize("shape", S.SHAPES + ((2, 9, 6), (3, 5, 2)), ids=lambda s: "%dx%dx%d" % s)
def test_closed_form_is_autograd(shape):
    from synth import synth_randn
    B, H, W = shape
    sd = {k: v.double() for k, v in S.stem_state().items()}
    x = S.stem_input(B, H, W).double()
    y = S.stem_forward(x, sd)["y"]
    dy = synth_randn(f"stem_train_d_{B}x{H}x{W}", *y.shape).double()
    ref = S.stem_reference(x, sd, dy, torch.float64)
    dW, dg, db = S.stem_closed_form(x, sd, dy)
    errs = (relerr(dW, ref["grads"]["conv1.weight"]), relerr(dg, ref["grads"]["bn1.weight"]), relerr(db, ref["grads"]["bn1.bias"]))
    print(f"  {shape}: dW {errs[0]:.1e} dgamma {errs[1]:.1e} dbeta {errs[2]:.1e}")
    assert max(errs) < 1e-12, errs


@pytest.mark.parametrize("shape", S.SHAPES + ((2, 84, 216),), ids=lambda s: "%dx%dx%d" % s)
def test_inputs_keep_the_band_thin(shape):
    """the GPU tests zero the upstream gradient at the entries of stem_band(pre64, 1e-4): at most 1e-3 of the entries (a condition:
    a share above it is answered by another input seed, never by another cap); with them zeroed, torch's fp32 run picks the fp64 window
    winners and ReLU masks at every entry that still carries a gradient"""
    B, H, W = shape
    sd = S.stem_state()
    x = S.stem_input(B, H, W)
    s64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        f64 = S.stem_forward(x.double(), s64)
        f32 = S.stem_forward(x, sd)
    band = S.stem_band(f64["pre"], S.BAND_THR)
    share = float(band.double().mean())
    live = ~band & (f64["y"] > 0)
    print(f"  {shape}: {int(band.sum())} of {band.numel()} entries in the band ({share:.2e})")
    assert share <= S.BAND_CAP
    assert torch.equal(f32["idx"][live], f64["idx"][live]) and torch.equal((f32["y"] > 0)[~band], (f64["y"] > 0)[~band])


def test_new_ops_refuse_cpu_tensors(lib):
    from neuralsampleid_amd import ops
    x, w, f = torch.zeros(2, 9, 6), torch.zeros(64, 49), torch.zeros(64)
    aff = ops.BNAffine(f, f, f, f)
    for c in (lambda: ops.stem7_stat(x, w), lambda: ops.stem7_pool_train_fwd(x, w, aff),
              lambda: ops.stem7_bwd(torch.zeros(2 * 3 * 2, 64), x, w, aff, f)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            c()


def test_training_forward_on_cpu_tensors_names_the_eval_forward(lib):
    from neuralsampleid_amd.encoder.resnet_ibn import ResNetIBN
    model = ResNetIBN().train()
    with pytest.raises(NotImplementedError, match="eval-mode forward, the training-mode forward has no CPU path"):
        model.stem_train(torch.zeros(1, 84, 40))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        model(torch.zeros(1, 84, 40))


def test_workspace_of_the_stem_ops(lib):
    from neuralsampleid_amd import _lib
    ws, parts = _lib.lib.nsid_workspace_bytes, _lib.lib.nsid_stem7_partials
    set_floats = _lib.lib.nsid_stem7_bwd_set_floats()
    assert set_floats == 2 * 49 * 64 + 3 * 64                           # A, X, a, b, S (padded to 64)
    for B, Hp, Wp in ((3, 10, 18), (3, 1, 1), (256, 21, 54)):
        tiles = B * Hp * ((Wp + 15) // 16)
        nstat, nbwd = parts(B * Hp, Wp, 0), parts(B * Hp, Wp, 1)
        assert nstat == min(tiles, 1024) and nbwd == min(tiles, 256)       # bounded however large the batch
        assert ws(b"stem7_stat", B * Hp, Wp) == 2 * nstat * 64 * 4
        assert ws(b"stem7_bwd", B * Hp, Wp) == nbwd * set_floats * 4
    assert ws(b"stem7_pool_train", 1000, 64) == 0


def test_clip_adam_can_leave_the_downsample_preparation_alone():
    """FusedClipAdam(ds_prep=False) is a keyword of the constructor, True by default (the GNN's Downsample weights)"""
    import inspect
    from neuralsampleid_amd.optim import FusedClipAdam
    p = inspect.signature(FusedClipAdam.__init__).parameters
    assert p["ds_prep"].default is True and p["direct_grads"].default is True
