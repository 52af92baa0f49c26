"""Every element of the module-level tensors (Grapher+FFN blocks, MRConv2d, mr_aggregate, Downsample, NT-Xent) against the oracle in
float64 (tests/oracle64.py). The fixtures pin the fp32 oracle to the reference through a sample and projections; here the kernels are
pinned to the oracle with no element left out, so an error confined to one pad row, tile edge or element cannot hide.

  forward tensors and running statistics: on the fixtures' own inputs and on the synthetic cases, with the bounds tests/test_e2e_gpu.py
      applies to the sample (1e-4 max(1, absmax) for blocks, 5e-5 for MRConv2d / Downsample, 1e-5 / 1e-6 for running statistics);
  gradients: max |g - g64| <= 16 floors (oracle64.check_grad), on inputs where no ReLU / max decision can fall differently
      (Downsample and NT-Xent have none: the fixture inputs; blocks, MRConv2d, mr_aggregate: oracle64.BLOCK_SEEDS / MRCONV_SEEDS at row
      counts M = B N below one GEMM tile and ragged). The ratio margin / error of every such case is recomputed and asserted, never skipped.

Each test prints `ratio <case> <tensor> err floor err/floor` lines (docs/experiments.md holds the measured table)."""
import pytest
import torch
import torch.nn as nn

import oracle64 as O
from conftest import from_rows, to_rows
from synth import synth_state

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _reset_tape():
    yield
    from neuralsampleid_amd import functional as F_
    F_.TAPE = None
    O.R.TAPE = None
    O.R.DECISIONS = None


def rows_of(y4):
    """a module's (B, C, N, 1) output -> the oracle's (B, N, C), on the CPU"""
    return to_rows(y4.detach().cpu())


def module_grads(module, run, into):
    for name, p in module.named_parameters():
        if p.grad is not None:
            into["grad." + name] = p.grad.detach().cpu().reshape(run["grad." + name].shape)
    for name, b in module.named_buffers():
        if b.is_floating_point():
            into["post." + name] = b.detach().cpu()


def check_forward(case, got, pair, names, bound, stat_bound):
    for name in names:
        ref = pair.ref(name)
        b = bound * max(1.0, float(ref.abs().max())) if case.startswith("block") else bound
        err = O.every_element(got[name], ref, b, f"{case} {name}")
        print(f"fwd {case} {name} err {err:.3e} bound {b:.3e} floor {pair.floor(name):.3e}")
    for name in [n for n in pair.names() if n.startswith("post.")]:
        O.every_element(got[name], pair.ref(name), stat_bound, f"{case} {name}")


def check_grads(case, got, pair):
    print(f"decisions {case} margin {pair.margin():.3e} error {pair.error():.3e} ratio {pair.ratio():.2f}")
    assert pair.ratio() >= O.MIN_RATIO, (case, pair.margin(), pair.error())
    names = [n for n in pair.names() if n.startswith(("dx", "dz", "grad."))]
    assert set(names) <= set(got), sorted(set(names) - set(got))
    for name in names:
        r = O.check_grad(got[name], pair, name, f"{case} {name}")
        if r is not None:
            err = r * pair.floor(name)
            print(f"ratio {case} {name} err {err:.3e} floor {pair.floor(name):.3e} err/floor {r:.2f}")


# ------------------------------------------------------------------ Grapher + FFN blocks
def gpu_block(C, N, k, d, x, gout, ids, run):
    """Seq(Grapher, FFN) through the reference-layout forward, the oracle's ids forced: eval, train forward, backward, running statistics"""
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd.encoder.gcn_lib.torch_vertex import Grapher
    from neuralsampleid_amd.encoder.graph_encoder import FFN
    blk = nn.Sequential(Grapher(C, k, d, "mr", "relu", "batch", True, False, 0.2, 1, n=N, drop_path=0.0, relative_pos=True),
                        FFN(C, 4 * C, C, act="relu", drop_path=0.0))
    blk.load_state_dict(synth_state(blk.state_dict(), "blk."))
    blk.to(DEV)
    got = {}
    x4 = from_rows(x).to(DEV)
    blk.eval()
    F_.TAPE = F_.KnnTape(replay=[ids[0]])
    with torch.no_grad():
        got["y_eval"] = rows_of(blk(x4))
    blk.train()
    F_.TAPE = F_.KnnTape(replay=[ids[1]])
    xg = x4.clone().requires_grad_(True)
    y = blk(xg)
    y.backward(from_rows(gout).to(DEV))
    F_.TAPE = None
    got["y_train"], got["dx"] = rows_of(y), rows_of(xg.grad)
    module_grads(blk, run, got)
    return got


BLOCK_FIXTURES = [("c64n256_k3d1", 64, 256, 3, 1), ("c64n256_k4d2", 64, 256, 4, 2), ("c128n128_k5d1", 128, 128, 5, 1),
                  ("c512n32_k3d1", 512, 32, 3, 1), ("c64n256_k18d3", 64, 256, 18, 3), ("c256n64_k18d3", 256, 64, 18, 3)]


@pytest.mark.parametrize("tag,C,N,k,d", BLOCK_FIXTURES)
def test_block_forward_on_fixture_inputs(golden, tag, C, N, k, d):
    """y_eval, y_train and the running statistics, every element. (The gradients of these inputs have ReLU pre-activations within the
    oracle's own fp32 error of zero, so a flip in the kernels would be legitimate: test_block_every_gradient uses inputs without.)"""
    g = golden("block_" + tag)
    P = O.synth_P(O.block_shapes(C), "blk.")
    x, gout = to_rows(g.t("x")), to_rows(g.t("gout"))
    ids = O.block_ids(P, x, k, d)
    pair = O.Pair(O.run_block, P, x, gout, ids, k=k, d=d)
    got = gpu_block(C, N, k, d, x, gout, ids, pair.r64)
    check_forward("block_" + tag, got, pair, ["y_eval", "y_train"], 1e-4, 1e-5)


@pytest.mark.parametrize("B,C,N,k,d", list(O.BLOCK_SEEDS))
def test_block_every_gradient(B, C, N, k, d):
    """dx and every parameter gradient, every element, at M = B N below one tile (B = 1) and ragged (B = 3); forward tensors too"""
    seed = O.BLOCK_SEEDS[B, C, N, k, d][0]
    P, x, gout, ids, pair = O.block_case(B, C, N, k, d, seed)
    case = f"block_b{B}c{C}n{N}k{k}d{d}"
    got = gpu_block(C, N, k, d, x, gout, ids, pair.r64)
    check_forward(case, got, pair, ["y_eval", "y_train"], 1e-4, 1e-5)
    check_grads(case, got, pair)


# ------------------------------------------------------------------ MRConv2d and mr_aggregate
def gpu_mrconv(C, x, gout, idx, run):
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.encoder.gcn_lib.torch_vertex import MRConv2d
    m = MRConv2d(C, 2 * C, "relu", "batch", True)
    m.load_state_dict(synth_state(m.state_dict(), "mr."))
    m.to(DEV)
    B, N, _ = x.shape
    got = {}
    x4 = from_rows(x).to(DEV)
    ei = torch.stack((idx.long(), torch.zeros_like(idx).long())).to(DEV)
    m.eval()
    with torch.no_grad():
        got["y_eval"] = rows_of(m(x4, ei))
    m.train()
    xg = x4.clone().requires_grad_(True)
    y = m(xg, ei)
    y.backward(from_rows(gout).to(DEV))
    got["y_train"], got["dx"] = rows_of(y), rows_of(xg.grad)
    module_grads(m, run, got)
    # the aggregation the module feeds its grouped conv with (mrconv_forward's first step)
    u, _ = ops.mr_aggregate_fwd(x.reshape(B * N, C).contiguous().to(DEV), idx.to(torch.int32).contiguous().to(DEV), B, N, C)
    got["u"] = u.cpu().reshape(B, N, 2 * C)
    return got


def gpu_mragg(x, gu, idx):
    from neuralsampleid_amd import ops
    B, N, C = x.shape
    idx_d = idx.to(torch.int32).contiguous().to(DEV)
    u, amax = ops.mr_aggregate_fwd(x.reshape(B * N, C).contiguous().to(DEV), idx_d, B, N, C)
    dy = ops.mr_aggregate_bwd(gu.reshape(B * N, 2 * C).contiguous().to(DEV), idx_d, amax, B, N, C)
    return {"u": u.cpu().reshape(B, N, 2 * C), "dx": dy.cpu().reshape(B, N, C)}


def test_mrconv_forward_on_fixture_inputs(golden):
    g = golden("mrconv_c64n256")
    P = O.synth_P(O.mrconv_shapes(64, 128), "mr.")
    x, gout, idx = to_rows(g.t("x")), to_rows(g.t("gout")), g.t("idx")
    pair = O.Pair(O.run_mrconv, P, x, gout, idx)
    got = gpu_mrconv(64, x, gout, idx, pair.r64)
    check_forward("mrconv_c64n256", got, pair, ["u", "y_eval", "y_train"], 5e-5, 1e-6)


def test_mragg_forward_on_fixture_inputs(golden):
    g = golden("mragg_c64n256")
    x, gu, idx = to_rows(g.t("x")), to_rows(g.t("gu")), g.t("idx")
    pair = O.Pair(O.run_mragg, x, gu, idx)
    check_forward("mragg_c64n256", gpu_mragg(x, gu, idx), pair, ["u"], 5e-5, 1e-6)


@pytest.mark.parametrize("B,N,C,k", list(O.MRCONV_SEEDS))
def test_mrconv_every_gradient(B, N, C, k):
    seed = O.MRCONV_SEEDS[B, N, C, k][0]
    P, x, gout, idx, pair = O.mrconv_case(B, N, C, k, seed)
    case = f"mrconv_b{B}n{N}c{C}k{k}"
    got = gpu_mrconv(C, x, gout, idx, pair.r64)
    check_forward(case, got, pair, ["u", "y_eval", "y_train"], 5e-5, 1e-6)
    check_grads(case, got, pair)


@pytest.mark.parametrize("B,N,C,k", list(O.MRAGG_SEEDS))
def test_mragg_every_gradient(B, N, C, k):
    seed = O.MRAGG_SEEDS[B, N, C, k][0]
    x, gu, idx, pair = O.mragg_case(B, N, C, k, seed)
    case = f"mragg_b{B}n{N}c{C}k{k}"
    got = gpu_mragg(x, gu, idx)
    check_forward(case, got, pair, ["u"], 5e-5, 1e-6)
    check_grads(case, got, pair)


# ------------------------------------------------------------------ Downsample and NT-Xent: no decisions, the fixture inputs serve
def test_downsample_every_element(golden):
    from neuralsampleid_amd.encoder.graph_encoder import Downsample
    g = golden("downsample_c64n256")
    P = O.synth_P(O.downsample_shapes(64, 128), "ds.")
    x, gout = to_rows(g.t("x")), to_rows(g.t("gout"))
    pair = O.Pair(O.run_downsample, P, x, gout)
    assert not pair.r64.relu and not pair.r64.cand
    ds = Downsample(64, 128)
    ds.load_state_dict(synth_state(ds.state_dict(), "ds."))
    ds.to(DEV)
    got = {}
    x4 = from_rows(x).to(DEV)
    ds.eval()
    with torch.no_grad():
        got["y_eval"] = rows_of(ds(x4))
    ds.train()
    xg = x4.clone().requires_grad_(True)
    y = ds(xg)
    y.backward(from_rows(gout).to(DEV))
    got["y_train"], got["dx"] = rows_of(y), rows_of(xg.grad)
    module_grads(ds, pair.r64, got)
    check_forward("downsample_c64n256", got, pair, ["y_eval", "y_train"], 5e-5, 1e-6)
    check_grads("downsample_c64n256", got, pair)


def test_ntxent_b256_every_gradient(golden):
    from neuralsampleid_amd import ops
    g = golden("ntxent_b256")
    tau = float(g["tau"])
    pair = O.Pair(O.run_ntxent, g.t("z_i"), g.t("z_j"), tau)
    loss, dzi, dzj = ops.ntxent_fwd_bwd(g.t("z_i").to(DEV), g.t("z_j").to(DEV), tau)
    assert abs(float(loss.detach()) - float(pair.ref("loss"))) < 2e-6 * max(1.0, abs(float(pair.ref("loss"))))
    check_grads("ntxent_b256", {"dz_i": dzi.cpu(), "dz_j": dzj.cpu()}, pair)
