"""The 256x256-tile class of the deferred weight-gradient phase (csrc/wgrad256.hip, tuning key wgrad256): every wide layer of the 't'
encoder (Nout % 256 == 0 and K % 256 == 0), plain and with the producer affine + ReLU on x, one and two row segments (views), both
settings of its rows per work item, the capped (max_workgroups) launch; against fp64 of the same bf16 operands and against the
128x128 class on the same problems.

Reference sites: the backward of every conv at encoder/gcn_lib/torch_vertex.py:152-162, encoder/graph_encoder.py:74-77,
encoder/gcn_lib/torch_nn.py:56 (autograd's dW = dY^T X)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (Nout, K, affine + ReLU on x): the wide layers of the 't' encoder (stages C = 256 and C = 512: Grapher fc1 / fc2, FFN fc1 / fc2)
WIDE = [(256, 256, False), (256, 512, True), (1024, 256, False), (256, 1024, True), (512, 512, False), (2048, 512, False),
        (512, 2048, True)]
M_VIEW = 8192        # rows per view: 2 / 1 items per segment at 4096 / 8192 rows per item


@pytest.fixture()
def bf16_mode():
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops
    ops.set_gemm_precision("bf16")
    F_.set_activation_dtype("bf16")
    yield
    ops.reset_tuning()
    ops.set_gemm_precision("fp32")
    F_.set_activation_dtype("fp32")


def _problems(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    probs = []
    for li, (N, K, aff) in enumerate(WIDE):
        views = 1 if li == 2 else 2
        segs = []
        for _ in range(views):
            dout = (0.5 * torch.randn(M_VIEW, N, generator=g, device=DEV)).to(torch.bfloat16)
            x = torch.randn(M_VIEW, K, generator=g, device=DEV).to(torch.bfloat16)
            sc = (1 + 0.2 * torch.randn(K, generator=g, device=DEV)) if aff else None
            sh = (0.3 * torch.randn(K, generator=g, device=DEV)) if aff else None
            segs.append((dout, x, sc, sh))
        probs.append((N, K, aff, segs))
    return probs


def _ref(N, K, aff, segs):
    """fp64 of what the kernel computes: x as the MFMA sees it (affine + ReLU in fp32, rounded to bf16), dout as stored"""
    dw = torch.zeros(N, K, dtype=torch.float64, device=DEV)
    for dout, x, sc, sh in segs:
        xf = x.double()
        if aff:
            xf = torch.relu((x.double() * sc.double() + sh.double()).float()).to(torch.bfloat16).double()
        dw += dout.double().t() @ xf
    return dw


def _run(probs, max_workgroups=0):
    from neuralsampleid_amd import ops
    items, outs = [], []
    for N, K, aff, segs in probs:
        dw = torch.zeros(N, K, device=DEV)
        outs.append(dw)
        for dout, x, sc, sh in segs:
            items.append((dout, x, dw, M_VIEW, N, K, 1, sc, sh, ops.ACT_RELU if aff else ops.ACT_NONE))
    ops.launch_counters(reset=True)
    ops.linear_bwd_weight_batch(items, max_workgroups=max_workgroups)
    torch.cuda.synchronize()
    return outs, ops.launch_counters()


@pytest.mark.parametrize("rows", [4096, 8192])
def test_wgrad256_matches_fp64_and_the_128_class(bf16_mode, rows):
    from neuralsampleid_amd import ops
    probs = _problems(700 + rows)
    refs = [_ref(*p) for p in probs]
    ops.set_tuning("wgrad256", 0)
    w3, cnt3 = _run(probs)
    assert cnt3["wgrad_grouped_256"] == 0 and cnt3["wgrad_grouped_w3"] >= 1, cnt3
    ops.set_tuning("wgrad256", 1)
    ops.set_tuning("wgg_rows256", rows)
    w4, cnt = _run(probs)
    # the new class ran, and only it: every problem here fits it (plain and affine problems in one launch)
    assert cnt["wgrad_grouped_256"] == 1 and cnt["wgrad_grouped_w3"] == 0 and cnt["gemm_bwd_weight"] == 0, cnt
    for (N, K, aff, segs), dw, dw3, ref in zip(probs, w4, w3, refs):
        scale = float(ref.abs().max())
        e = float((dw.double() - ref).abs().max()) / scale
        e3 = float((dw3.double() - ref).abs().max()) / scale
        d = float((dw - dw3).abs().max()) / scale
        # fp32 accumulation of bf16 products over <= 16 384 rows (tests/test_wgrad_grouped_gpu.py): with the affine the fp64 restatement
        # rounds an operand to the other bf16 neighbour now and then, for both classes alike
        assert e < (2e-4 if aff else 2e-5) and e < 1.5 * e3 + 2e-6 and d < 1e-5, ((N, K, aff, len(segs)), e, e3, d)


def test_wgrad256_capped_launch(bf16_mode):
    """max_workgroups: every workgroup walks several items with a static stride (the data-parallel pieces of the phase); the sums
    are those of the uncapped launch up to the order of the fp32 atomics"""
    from neuralsampleid_amd import ops
    probs = _problems(901)
    ops.set_tuning("wgrad256", 1)
    ops.set_tuning("wgg_rows256", 4096)
    full, _ = _run(probs)
    capped, cnt = _run(probs, max_workgroups=24)
    assert cnt["wgrad_grouped_256"] == 1, cnt
    for a, b in zip(full, capped):
        assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max()) + 1e-6


def test_wgrad256_leaves_other_shapes_to_the_other_classes(bf16_mode):
    """problems with Nout or K not a multiple of 256 stay on the 128x128 (and smaller) classes in the same batch"""
    from neuralsampleid_amd import ops
    g = torch.Generator(device=DEV).manual_seed(3)
    ops.set_tuning("wgrad256", 1)
    items, outs = [], []
    for (M, N, K) in ((2048, 512, 512), (2048, 128, 512), (2048, 512, 128), (2048, 64, 64)):
        dout = (0.5 * torch.randn(M, N, generator=g, device=DEV)).to(torch.bfloat16)
        x = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
        dw = torch.zeros(N, K, device=DEV)
        items.append((dout, x, dw, M, N, K, 1, None, None, ops.ACT_NONE))
        outs.append((dw, dout.double().t() @ x.double()))
    ops.launch_counters(reset=True)
    ops.linear_bwd_weight_batch(items)
    torch.cuda.synchronize()
    cnt = ops.launch_counters()
    assert cnt["wgrad_grouped_256"] == 1 and cnt["wgrad_grouped_w3"] == 1, cnt
    for dw, ref in outs:
        assert float((dw.double() - ref).abs().max()) / float(ref.abs().max()) < 2e-5
