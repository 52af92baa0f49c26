"""The float64 oracle harness (tests/oracle64.py) on the CPU: it reproduces what tests/test_oracle_golden.py pins, every committed seed keeps
its decisions away from a flip, and the every-element comparison catches what the compact form of a fixture tensor lets through."""
import pytest
import torch

import oracle64 as O
from compare import STRIDE, absmax, maxerr
from conftest import from_rows, to_rows
from oracle import ref_torch as R

torch.set_num_threads(8)


def _block_like_the_golden_test(g, C, k, d):
    """tests/test_oracle_golden.py::test_block's own computation (its search, no tape)"""
    P = O.synth_P(O.block_shapes(C), "blk.")
    x = to_rows(g.t("x"))
    y_eval = R.ffn(R.grapher(x, P, "0.", k, d, False, None), P, "1.", False, None)
    keys = R.trainable_keys(P)
    for key in keys:
        P[key].requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    st = R.BNState()
    y = R.ffn(R.grapher(xg, P, "0.", k, d, True, st), P, "1.", True, st)
    y.backward(to_rows(g.t("gout")))
    out = {"y_eval": y_eval, "y_train": y.detach(), "dx": xg.grad}
    out.update({"grad." + key: P[key].grad for key in keys})
    out.update({"post." + key: v for key, v in st.updates.items() if v.is_floating_point()})
    return out


@pytest.mark.parametrize("tag,C,k,d", [("c512n32_k3d1", 512, 3, 1), ("c64n256_k4d2", 64, 4, 2)])
def test_harness_fp32_is_the_pinned_oracle_bit_for_bit(golden, tag, C, k, d):
    g = golden("block_" + tag)
    want = _block_like_the_golden_test(g, C, k, d)
    P = O.synth_P(O.block_shapes(C), "blk.")
    x, gout = to_rows(g.t("x")), to_rows(g.t("gout"))
    run = O.run_block(P, x, gout, O.block_ids(P, x, k, d), torch.float32, k, d)
    assert set(run) == set(want)
    for name, v in want.items():
        assert torch.equal(run[name], v), name
    assert len(run.relu) == 2 and len(run.cand) == 1 and R.DECISIONS is None and R.TAPE is None


def test_harness_modules_match_the_fixtures(golden):
    """MRConv2d, mr_aggregate, Downsample and NT-Xent of the harness in fp32 against their fixtures, with test_oracle_golden.py's bounds"""
    from compare import allclose
    g = golden("mrconv_c64n256")
    run = O.run_mrconv(O.synth_P(O.mrconv_shapes(64, 128), "mr."), to_rows(g.t("x")), to_rows(g.t("gout")), g.t("idx"), torch.float32)
    assert allclose(from_rows(run["y_train"]), g.t("y"), atol=2e-5) and allclose(from_rows(run["dx"]), g.t("dx"), atol=2e-5)
    assert allclose(from_rows(run["u"]), g.t("u"), atol=0.0, rtol=0.0) and allclose(run["grad.nn.0.weight"], g.t("dweight"), atol=2e-4)
    g = golden("mragg_c64n256")
    run = O.run_mragg(to_rows(g.t("x")), to_rows(g.t("gu")), g.t("idx"), torch.float32)
    assert torch.equal(from_rows(run["u"]), g.t("u")) and allclose(from_rows(run["dx"]), g.t("dx"), atol=1e-6)
    g = golden("downsample_c64n256")
    run = O.run_downsample(O.synth_P(O.downsample_shapes(64, 128), "ds."), to_rows(g.t("x")), to_rows(g.t("gout")), torch.float32)
    assert allclose(from_rows(run["y_eval"]), g.t("y_eval"), atol=2e-5) and allclose(from_rows(run["y_train"]), g.t("y_train"), atol=2e-5)
    assert allclose(from_rows(run["dx"]), g.t("dx"), atol=2e-5) and allclose(run["grad.conv.0.weight"], g.t("dweight"), atol=2e-4)
    g = golden("ntxent_b256")
    run = O.run_ntxent(g.t("z_i"), g.t("z_j"), float(g["tau"]), torch.float32)
    assert abs(float(run["loss"]) - float(g["loss"][0])) < 2e-6 and allclose(run["dz_i"], g.t("dz_i"), atol=1e-6)
    assert allclose(run["dz_j"], g.t("dz_j"), atol=1e-6)


@pytest.mark.parametrize("shape", list(O.BLOCK_SEEDS))
def test_committed_block_seeds_keep_every_decision_away_from_a_flip(shape):
    pair = O.block_case(*shape, O.BLOCK_SEEDS[shape][0], want_grad=False, want_eval=False)[-1]
    print(shape, pair.relu_margin(), pair.top2_margin(), pair.error(), pair.ratio())
    assert pair.ratio() >= O.MIN_RATIO, (shape, pair.margin(), pair.error())


def test_committed_mrconv_seeds_keep_every_decision_away_from_a_flip():
    assert O.MRCONV_SEEDS and O.MRAGG_SEEDS
    for shape, (seed, *_) in O.MRCONV_SEEDS.items():
        pair = O.mrconv_case(*shape, seed, want_grad=False)[-1]
        assert len(pair.r64.relu) == 1 and len(pair.r64.cand) == 1
        assert pair.ratio() >= O.MIN_RATIO, ("mrconv", shape, pair.margin(), pair.error())
    for shape, (seed, *_) in O.MRAGG_SEEDS.items():
        pair = O.mragg_case(*shape, seed, want_grad=False)[-1]
        assert pair.ratio() >= O.MIN_RATIO, ("mragg", shape, pair.margin(), pair.error())


def test_fixture_inputs_are_too_close_to_a_flip_for_elementwise_gradients(golden):
    """why the gradient checks run on synthetic inputs: on a fixture's own input the smallest ReLU pre-activation is within a few of the
    oracle's own fp32 errors of zero, so a kernel that rounds differently may legitimately take the other branch there"""
    g = golden("block_c512n32_k3d1")
    P = O.synth_P(O.block_shapes(512), "blk.")
    x, gout = to_rows(g.t("x")), to_rows(g.t("gout"))
    pair = O.Pair(O.run_block, P, x, gout, O.block_ids(P, x, 3, 1), k=3, d=1, want_grad=False, want_eval=False)
    assert 0 < pair.margin() and pair.ratio() < O.MIN_RATIO, (pair.margin(), pair.error())


@pytest.fixture(scope="module")
def c512(golden):
    g = golden("block_c512n32_k3d1")
    P = O.synth_P(O.block_shapes(512), "blk.")
    x, gout = to_rows(g.t("x")), to_rows(g.t("gout"))
    return g, O.Pair(O.run_block, P, x, gout, O.block_ids(P, x, 3, 1), k=3, d=1, want_eval=False)


def _block_bound(ref):
    return 1e-4 * max(1.0, float(ref.abs().max()))


def test_one_wrong_unsampled_element_passes_the_compact_form_and_fails_here(c512):
    g, pair = c512
    ref, y = pair.ref("y_train"), pair.r32["y_train"].clone()
    O.every_element(y, ref, _block_bound(ref), "y_train")                   # the oracle's own fp32 passes
    flat = 5 * STRIDE * 100 + 3
    assert flat % STRIDE != 0
    y.view(-1)[flat] += 0.01
    with pytest.raises(AssertionError, match=f"flat {flat} "):
        O.every_element(y, ref, _block_bound(ref), "y_train")
    gold = g.t("y_train")                                                    # the hole: the same tensor passes today's check of the fixture
    assert maxerr(from_rows(y), gold) < 1e-4 * max(1.0, absmax(gold))


def test_one_wrong_edge_row_fails_here_whatever_the_compact_form_sees_of_it(c512):
    g, pair = c512
    ref, gold = pair.ref("y_train"), g.t("y_train")
    y = pair.r32["y_train"].clone()
    y[1, -1, :] *= 1.02                                                       # the last node row of one clip, 2 % off
    with pytest.raises(AssertionError, match=r"index \(1, 31, "):
        O.every_element(y, ref, _block_bound(ref), "y_train")
    # measured: the compact form does see THIS one, 0.098 against a bound of 7.6e-4, because 73 of the row's 512 elements are sampled
    # (and the other 439, 2 % off, still move a projection by 1.8e-3). What it lets through is the same row off by 0.5 % where the
    # sample does not look: 439 wrong elements, each 10 bounds out, show as 4.4e-4.
    assert maxerr(from_rows(y), gold) > 1e-4 * max(1.0, absmax(gold))
    y4 = from_rows(pair.r32["y_train"].clone())
    flat = torch.arange(y4.numel()).reshape(y4.shape)[1, :, -1, 0]
    y4[1, :, -1, 0] = torch.where(flat % STRIDE != 0, y4[1, :, -1, 0] * 1.005, y4[1, :, -1, 0])
    with pytest.raises(AssertionError, match=r"index \(1, 31, "):
        O.every_element(to_rows(y4), ref, _block_bound(ref), "y_train")
    assert maxerr(y4, gold) < 1e-4 * max(1.0, absmax(gold))                   # the hole


def test_a_zeroed_gradient_row_fails_the_floor_rule(c512):
    _, pair = c512
    dx = pair.r32["dx"].clone()
    assert O.check_grad(dx, pair, "dx", "dx") <= 1.0                          # the oracle's own fp32 is one floor away by definition
    dx[0, 17, :] = 0.0
    with pytest.raises(AssertionError, match=r"index \(0, 17, "):
        O.check_grad(dx, pair, "dx", "dx")
    w = pair.r32["grad.1.fc1.0.weight"].clone()                               # and one output row of a wide weight gradient
    w[1234] = 0.0
    with pytest.raises(AssertionError, match=r"index \(1234, "):
        O.check_grad(w, pair, "grad.1.fc1.0.weight", "dW")
    zero = pair.ref("grad.0.fc1.0.bias")                                      # a conv bias in front of a BatchNorm: analytically zero
    assert float(zero.abs().max()) < O.ZERO_GRAD and O.check_grad(torch.full_like(zero, 5e-4), pair, "grad.0.fc1.0.bias", "db") is None
