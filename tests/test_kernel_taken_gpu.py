"""The kernel a profiled op books its time under is the one the library launched (include/nsid.h nsid_debug_last_kernel, NSID_DECLINED).

Two independent mechanisms must agree for every call: the name in ops.PROFILE.records (the library's nsid_took at the point of decision)
and the library's launch counters (nsid_count, beside the launch). The expected names are written out from the launch rules of
csrc/gemm.hip, wsgemm.hip, wgrad.hip, knn.hip and mr.hip; they are the kernel table's keys, i.e. what bench.rocprof_family makes of the
kernel's demangled name. Tuning keys steer the rules so that the shapes stay at one or a few tiles. bf16 storage with registered bf16
weight shadows throughout, so that a call records its own launches and no conversion pass."""
import pytest
import torch

from synth import synth_randn

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture()
def ops():
    from neuralsampleid_amd import ops as o
    prec = o.get_gemm_precision()
    o.set_gemm_precision("bf16")
    before = (o.PROFILE, o.FUSE_BN_BWD_APPLY)
    try:
        yield o
    finally:
        o.PROFILE, o.FUSE_BN_BWD_APPLY = before
        o.set_gemm_precision(prec)
        o.reset_tuning()


def taken(ops, fn, **tuning):
    """(names recorded, counters that moved, result) of one call under its own profile, with the tuning keys given"""
    for key, value in tuning.items():
        ops.set_tuning(key, value)
    ops.launch_counters(reset=True)
    ops.PROFILE = ops.KernelProfile()
    try:
        out = fn()
        names = [rec[0] for rec in ops.PROFILE.records]
    finally:
        ops.PROFILE = None
        ops.reset_tuning()
    torch.cuda.synchronize()
    return names, {k: v for k, v in ops.launch_counters().items() if v}, out


def acts(tag, rows, cols):
    return synth_randn("taken:" + tag, rows, cols).to(BF).to(DEV)


def weight(ops, tag, rows, cols):
    """an fp32 weight matrix with a fresh bf16 shadow: the GEMM under test converts nothing"""
    w = (synth_randn("taken:" + tag, rows, cols) * cols ** -0.5).to(DEV)
    ops.SHADOWS.register(w, ops.f32_to_bf16(w), owner=w, fresh=True)
    return w


def bn_affine(ops, r):
    mean, var = r.float().mean(0), r.float().var(0, unbiased=False)
    invstd = 1 / torch.sqrt(var + 1e-5)
    return ops.BNAffine(invstd.contiguous(), (-mean * invstd).contiguous(), mean.contiguous(), invstd.contiguous())


# (tuning, kernel, the counter of that kernel). Forward: M = 128, out = x w^T. (64, 64) is a layer of the weight-stationary table,
# (K = 128, Nout = 256) is not and is one row tile: the heuristic narrows it (fewer than 128 tiles), fwd_narrow overrides the heuristic.
FWD = [(64, 64, {}, "ws_fwd_kernel", "ws_fwd"),
       (64, 64, {"ws_gemm": 0}, "gemm_kernel<128,64,true,true>", "gemm_fwd"),
       (256, 128, {}, "gemm_kernel<128,64,true,true>", "gemm_fwd"),
       (256, 128, {"fwd_narrow": 0}, "gemm_kernel<128,128,true,true>", "gemm_fwd"),
       (256, 128, {"fwd_narrow": 1}, "gemm_kernel<128,64,true,true>", "gemm_fwd")]


@pytest.mark.parametrize("Nout,K,tuning,kernel,counter", FWD)
def test_forward_records_the_kernel_the_library_took(ops, Nout, K, tuning, kernel, counter):
    M = 128
    x, w = acts("fx", M, K), weight(ops, "fw", Nout, K)
    names, cnt, _ = taken(ops, lambda: ops.linear_fwd(x, w, None, M, Nout, K), **tuning)
    assert names == [kernel] and cnt[counter] == 1, (names, cnt)
    assert ("ws_fwd" in cnt) == (kernel == "ws_fwd_kernel") and ("gemm_fwd" in cnt) == (kernel != "ws_fwd_kernel"), cnt


# backward-data: din (M, K) = dout (M, Nout) w. (Nout = 256, K = 256) is no layer of the table; one row tile of it is narrowed as above.
BWD = [(64, 64, {}, "ws_bwd_kernel", "ws_bwd_data"),
       (64, 64, {"ws_gemm": 0}, "gemm_kernel<128,64,true,false>", "gemm_bwd_data"),
       (256, 256, {}, "gemm_kernel<128,64,true,false>", "gemm_bwd_data"),
       (256, 256, {"bwd_narrow": 0}, "gemm_kernel<128,128,true,false>", "gemm_bwd_data"),
       (256, 256, {"bwd_narrow": 1}, "gemm_kernel<128,64,true,false>", "gemm_bwd_data")]


@pytest.mark.parametrize("Nout,K,tuning,kernel,counter", BWD)
def test_backward_data_records_the_kernel_the_library_took(ops, Nout, K, tuning, kernel, counter):
    M = 128
    dout, w = acts("bd", M, Nout), weight(ops, "bw", Nout, K)
    names, cnt, _ = taken(ops, lambda: ops.linear_bwd_data(dout, w, M, Nout, K), **tuning)
    assert names == [kernel] and cnt[counter] == 1, (names, cnt)
    assert ("ws_bwd_data" in cnt) == (kernel == "ws_bwd_kernel") and ("gemm_bwd_data" in cnt) == (kernel != "ws_bwd_kernel"), cnt


def _fused_backward(ops, K, tuning, fuse):
    M, Nout = 128, 64
    dy, r, w = acts("qy", M, Nout), acts("qr", M, Nout), weight(ops, "qw", Nout, K)
    aff = bn_affine(ops, r)
    dg, db = torch.zeros(Nout, device=DEV), torch.zeros(Nout, device=DEV)
    ops.FUSE_BN_BWD_APPLY = fuse
    return taken(ops, lambda: ops.bn_backward_linear_bwd_data(dy, r, aff, ops.ACT_RELU, dg, db, None, w, M, Nout, K), **tuning)


def test_fused_backward_on_a_weight_stationary_layer(ops):
    names, cnt, _ = _fused_backward(ops, 64, {}, False)        # a layer of the table: fused at every call site
    assert names == ["col_reduce_kernel", "bn_bwd_finalize_kernel", "ws_bwd_kernel +bn_apply_load"], names
    assert cnt["ws_bwd_bnapply"] == 1 and "gemm_bwd_data" not in cnt and "bn_bwd_apply" not in cnt, cnt


def test_fused_backward_on_the_tile_kernel(ops):
    names, cnt, _ = _fused_backward(ops, 64, {"ws_gemm": 0}, True)
    assert names == ["col_reduce_kernel", "bn_bwd_finalize_kernel", "gemm_kernel<128,64,true,false> +bn_apply_load"], names
    assert cnt["gemm_bn_apply_load"] == 1 and cnt["gemm_bwd_data"] == 1 and "bn_bwd_apply" not in cnt and "ws_bwd_bnapply" not in cnt, cnt


def test_unfusable_backward_records_the_unfused_pair(ops):
    names, cnt, _ = _fused_backward(ops, 96, {"ws_gemm": 0}, True)      # K = 96 is no whole number of 64-wide tiles
    assert names[-2:] == ["bn_bwd_apply_kernel", "gemm_kernel<128,64,true,false>"] and not any("+bn_apply_load" in n for n in names), names
    assert cnt["bn_bwd_apply"] == 1 and cnt["gemm_bwd_data"] == 1 and "gemm_bn_apply_load" not in cnt, cnt


# weight gradient dw (Nout, K) += dout^T x. One 128x64 tile over 1 024 rows is below the rectangular form's workgroup floor
# (wgrad_rect_min) until the floor is lowered; one 128x128 tile is below the 8-wave form's (w3_min_tiles) likewise.
WGRAD = [(1024, 128, 64, {"wgrad_rect_min": 1}, "gemm_kernel<128,64,false,false>", "wgrad_rect"),
         (1024, 128, 64, {"wgrad_rect": 0}, "gemm_kernel<64,64,false,false>", "wgrad_square"),
         (1024, 128, 64, {}, "gemm_kernel<64,64,false,false>", "wgrad_square"),
         (128, 128, 128, {"w3_min_tiles": 1}, "wgrad3_kernel", "wgrad3")]


@pytest.mark.parametrize("M,Nout,K,tuning,kernel,counter", WGRAD)
def test_weight_gradient_records_the_kernel_the_library_took(ops, M, Nout, K, tuning, kernel, counter):
    dout, x = acts("wd", M, Nout), acts("wx", M, K)
    dw = torch.zeros(Nout, K, device=DEV)
    names, cnt, _ = taken(ops, lambda: ops.linear_bwd_weight(dout, x, dw, M, Nout, K), **tuning)
    assert names == [kernel] and cnt[counter] == 1, (names, cnt)
    assert sum(cnt.get(c, 0) for c in ("wgrad_rect", "wgrad_square", "wgrad3")) == 1, cnt


# kNN at B = 2, N = 64, C = 64: (k, affine on the load, tuning, kernel, counter)
KNN = [(3, True, {}, "knn2_kernel", "knn2"),
       (3, False, {"knn_pair_min": 1}, "knn2_raw_kernel", "knn2_raw"),       # plain bf16 features in a launch of "many" clips
       (3, True, {"knn_pair_min": 1}, "knn2_pair_kernel", "knn2_pair"),      # the same with an affine: two workgroups per CU
       (9, True, {"knn_sel_min_n": 64}, "knn_sel_kernel", "knn_sel"),
       (9, True, {}, "knn_rank_kernel", "knn_rank"),
       (9, True, {"knn_strips": 1}, "knn_kernel", "knn_strips")]


@pytest.mark.parametrize("k,affine,tuning,kernel,counter", KNN)
def test_knn_records_the_kernel_the_library_took(ops, k, affine, tuning, kernel, counter):
    B, N, C = 2, 64, 64
    r = acts("kr", B * N, C)
    aff = ops.BNAffine((1 + 0.2 * synth_randn("taken:ks", C)).to(DEV), (0.3 * synth_randn("taken:kh", C)).to(DEV)) if affine else None
    names, cnt, idx = taken(ops, lambda: ops.knn_graph(r, B, N, C, k, 1, aff), **tuning)
    assert names == [kernel] and cnt[counter] == 1, (names, cnt)
    others = {"knn2_raw", "knn2_pair", "knn_sel", "knn_rank", "knn_strips", "knn_big"} - {counter}
    assert not others & set(cnt), cnt
    assert tuple(idx.shape) == (B, N, k) and int(idx.min()) >= 0 and int(idx.max()) < N


def test_aggregation_backward_with_and_without_the_column_sums(ops):
    """The degree-ranked kernel emits the BatchNorm column sums; with the kernel switched off nsid_mr_aggregate_bwd_bn declines, which
    leaves no record, and the plain kernel runs. Both kernels form, per output element, the same fp32 sum in an order set by LDS atomics:
    du here lies on a grid of 1/8 with |du| <= 4, so every partial sum of the at most 1 + N k terms is exact in fp32 and the one
    rounding to bf16 sees the same value whatever the order: dy is equal bit for bit."""
    B, N, C, k = 2, 256, 64, 3
    g = torch.Generator().manual_seed(3)
    r = acts("mr", B * N, C)
    idx = torch.randint(0, N, (B, N, k), generator=g, dtype=torch.int32).to(DEV)
    du = (torch.randint(-32, 33, (B * N, 2 * C), generator=g).float() / 8).to(BF).to(DEV)
    aff = bn_affine(ops, r)
    _, amax = ops.mr_aggregate_fwd(r, idx, B, N, C)
    call = lambda: ops.mr_aggregate_bwd(du, idx, amax, B, N, C, bn=(r, aff, ops.ACT_RELU))
    names, cnt, (dy, part) = taken(ops, call)
    assert names == ["mr_bwd_sorted_kernel +bn_sums"] and cnt["mr_bwd_sorted"] == 1, (names, cnt)
    assert part is not None and tuple(part.shape) == (2, B, C)
    names0, cnt0, (dy0, part0) = taken(ops, call, mr_bwd_sorted_min_k=0)
    assert names0 == ["mr_bwd_kernel"] and "mr_bwd_sorted" not in cnt0, (names0, cnt0)
    assert part0 is None and torch.equal(dy0, dy)
    names1, cnt1, dy1 = taken(ops, lambda: ops.mr_aggregate_bwd(du, idx, amax, B, N, C))
    assert names1 == ["mr_bwd_sorted_kernel"] and cnt1["mr_bwd_sorted"] == 1 and torch.equal(dy1, dy), (names1, cnt1)


def test_a_declined_fused_form_leaves_no_record(ops):
    """tests/test_bf16_storage_gpu.py's two "is None" cases (C = 32 is outside both fused eval-mode forms): nothing is recorded for them,
    and the valid call behind each is recorded under its own name"""
    M, B, k = 128, 2, 3
    x, x32 = acts("dx", M, 64), acts("dx32", M, 32)
    w1, w2, w1s, w2s = weight(ops, "d1", 256, 64), weight(ops, "d2", 64, 256), weight(ops, "d1s", 128, 32), weight(ops, "d2s", 32, 128)
    b1, b2 = torch.zeros(256, device=DEV), torch.zeros(64, device=DEV)
    y, y32 = acts("dy", B * 256, 64), acts("dy32", B * 256, 32)
    idx = torch.randint(0, 256, (B, 256, k), generator=torch.Generator().manual_seed(5), dtype=torch.int32).to(DEV)
    wg, wgs, bg = weight(ops, "dg", 128, 32), weight(ops, "dgs", 64, 16), torch.zeros(128, device=DEV)
    ops.launch_counters(reset=True)
    ops.PROFILE = ops.KernelProfile()
    try:
        rec = ops.PROFILE.records
        assert ops.ffn_fused_fwd(x32, w1s, b1[:128], w2s, b2[:32], M, 32, 128) is None and len(rec) == 0
        assert ops.ffn_fused_fwd(x, w1, b1, w2, b2, M, 64, 256) is not None and [q[0] for q in rec] == ["ffn_fused_kernel"]
        assert ops.mrconv_fused_fwd(y32, idx, B, 256, 32, wgs, bg[:64]) is None and len(rec) == 1
        assert ops.mrconv_fused_fwd(y, idx, B, 256, 64, wg, bg) is not None
        assert [q[0] for q in rec] == ["ffn_fused_kernel", "mrconv_fused_kernel"]
    finally:
        ops.PROFILE = None
    torch.cuda.synchronize()
    cnt = ops.launch_counters()
    assert cnt["ffn_fused"] == 1 and cnt["mrconv_fused"] == 1, cnt
