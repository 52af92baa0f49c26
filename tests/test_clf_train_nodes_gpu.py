"""Classifier training on node matrices of 33 .. 128 nodes on the MI355X (the multi-tile kernels of csrc/clf_train.hip through
ops.clf_attn_fwd_n / clf_attn_bwd_n / clf_seg_reduce_n and downstream.clf_train_scores_n): parity of the scores and of all eight
parameter gradients with an fp64 nn.MultiheadAttention restatement of the reference module, the reference's own training steps
(tests/golden/clf_train_nodes.npz), launch counters and the N <= 32 dispatch, consistency with the evaluation path, bitwise
reproducibility and pair independence, reads that stay inside the data, the multi-tile entries against the one-tile ones at N = 32,
the 256-mel encoder end to end, and refusals that launch nothing.

Bounds: 1e-5 absolute on scores, 1e-5 relative (L2) per gradient, the project's bound at N <= 32. The reference module's own fp32
against its fp64 on the parity cases below, measured on the CPU (the cases are built on the CPU from seeds, parity_case):
  C = 512, the six (B, N) cases: at most 2.4e-7 on a score and 8.7e-7 on a gradient (fc.3.bias at (8, 33));
  C = 640 (4, 128) 1.4e-7 / 6.5e-7, C = 640 (4, 33) 2.4e-7 / 8.1e-7, C = 768 (4, 128) 1.1e-7 / 6.7e-7, C = 1024 (4, 128) 6.4e-8 / 8.5e-7.
None exceeds 1e-6, so every case keeps the bound 1e-5. The fp64 scores spread over [0.10, 0.89]. The dropout masks come from seeded generators and keep the one-element
fc.3.bias gradient well conditioned (conditioned_keep, the rule of tests/test_clf_wide_gpu.py); no test here depends on the state
of torch's global generators."""
import io

import numpy as np
import pytest
import torch

from test_clf_wide_gpu import GRAD_NAMES, Ref64, bce, make_clf, rel, rule_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
ONE_TILE = ("clf_attn_fwd", "clf_attn_bwd", "clf_seg_reduce", "clf_node_rows")
MULTI = ("clf_attn_fwd_n", "clf_attn_bwd_n", "clf_seg_reduce_n", "clf_node_rows_n")


def _mods():
    from neuralsampleid_amd import downstream, ops
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    return downstream, ops, CrossAttentionClassifier


@pytest.fixture(autouse=True)
def own_rng():
    with torch.random.fork_rng(devices=[torch.cuda.current_device()]):
        torch.manual_seed(33)
        yield


# ------------------------------------------------------------------------------------------------ cases, built on the CPU
def features_cpu(seed, B, C, N, d=128):
    g = torch.Generator().manual_seed(seed)
    ni = torch.randn(B, C, N, generator=g)
    nj = ni + 0.5 * torch.randn(B, C, N, generator=g)
    zi = torch.nn.functional.normalize(torch.randn(B, d, generator=g), dim=1)
    zj = torch.nn.functional.normalize(zi + 0.6 * torch.randn(B, d, generator=g), dim=1)
    return ni.contiguous(), nj.contiguous(), zi, zj


def mined_pairs(zi, zj, B, k=3):
    """ranks 1..k of z_i z_all^T (fp64, stable) as downstream.pair_lists orders them, one candidate forced to serve many pairs"""
    sim = zi.double() @ torch.cat([zi, zj]).double().T
    hn = torch.argsort(-sim, dim=1, stable=True)[:, 1:k + 1]
    ar = torch.arange(B)
    qi, ci = torch.cat([ar, ar.repeat(k)]), torch.cat([ar + B, hn.reshape(-1)])
    ci[B + 1: B + 1 + min(2 * B, k * B - 1)] = 0
    return qi, ci


def conditioned_keep(state, nq, nc, qi, ci, B, seed, p=0.3):
    """(P, 128) keep mask / (1 - p) from a seeded generator, on the CPU; the seed moves on until kappa of fc.3.bias's sum over the
    pairs is <= 14, computed from the fp64 module alone (tests/test_clf_wide_gpu.py conditioned_keep states the reasoning)"""
    m = Ref64(state)
    P = qi.numel()
    y = torch.cat([torch.ones(B), torch.zeros(P - B)]).double()
    w = torch.cat([torch.full((B,), 1.0 / B), torch.full((P - B,), 1.0 / (P - B))]).double()
    with torch.no_grad():
        h = m.hidden(nq.double()[qi], nc.double()[ci])
        for seed in range(seed, seed + 64):
            keep = torch.empty(P, 128).bernoulli_(1.0 - p, generator=torch.Generator().manual_seed(seed)).div_(1.0 - p)
            t = w * (m.head(h, keep.double())[:, 0] - y)
            if float(t.abs().sum() / t.sum().abs()) <= 14.0:
                return keep
    raise AssertionError("no well-conditioned dropout mask in 64 seeds")


def parity_case(C, B, N, pos_embed, num_nodes):
    """(state, query nodes, candidate nodes, q_idx, c_idx, keep) of one parity case, CPU tensors from seeds"""
    state = rule_state(900 + C + B + N, C, pos_embed, num_nodes)
    ni, nj, zi, zj = features_cpu(C + B * 64 + N, B, C, N)
    qi, ci = mined_pairs(zi, zj, B)
    nc = torch.cat([ni, nj])
    keep = conditioned_keep(state, ni, nc, qi, ci, B, seed=1000 + C + B + N)
    return state, ni, nc, qi, ci, keep


def ref_step(state, nq, nc, qi, ci, keep, B, dtype=torch.float64):
    """scores and the eight parameter gradients of BCE(pos) + BCE(neg) from the reference module's restatement in dtype"""
    m = Ref64(state).to(dtype)
    s = m(nq.to(dtype)[qi], nc.to(dtype)[ci], keep.to(dtype))
    bce(s, B).backward()
    return s.detach(), {n: p.grad for n, p in m.named_parameters()}


def grad_errors(g, g64, C):
    """{name: relative L2 error}; attn.in_proj_bias over its Q and V parts (its K part is zero in exact arithmetic, the softmax
    being shift-invariant), and the K part's largest element under 'K'"""
    out = {}
    for n in GRAD_NAMES:
        if n == "attn.in_proj_bias":
            out[n] = max(rel(g[n][:C], g64[n][:C]), rel(g[n][2 * C:], g64[n][2 * C:]))
            out["K"] = float(g[n][C:2 * C].abs().max())
        else:
            out[n] = rel(g[n], g64[n])
    return out


def step_grads_n(clf, nq, nc, qi, ci, keep, B):
    downstream, _, _ = _mods()
    clf.zero_grad(set_to_none=True)
    s = downstream.clf_train_scores_n(clf, nq, nc, qi, ci, keep)
    loss = bce(s, B)
    loss.backward()
    return s.detach(), loss.detach(), {n: p.grad for n, p in clf.named_parameters()}


PARITY = [(512, 8, 33, True, 128), (512, 4, 64, False, 128), (512, 4, 97, True, 128), (512, 8, 128, True, 128),
          (512, 8, 100, True, 100), (512, 3, 65, True, 128),
          (640, 4, 128, True, 128), (768, 4, 128, True, 128), (1024, 4, 128, True, 128), (640, 4, 33, True, 128)]


# ------------------------------------------------------------------------------------------------ 1. fp64 parity
@pytest.mark.parametrize("C,B,N,pos_embed,num_nodes", PARITY)
def test_fp64_parity(C, B, N, pos_embed, num_nodes):
    """Scores within 1e-5 and every parameter gradient within 1e-5 relative (L2) of the fp64 module. The reference module's own
    fp32 against that fp64, measured on the CPU on these very cases (the module docstring lists them): at most 2.4e-7 / 8.7e-7
    (scores / gradients) over the C = 512 cases and 2.4e-7 / 8.5e-7 over the four cases at 640, 768 and 1024: all below 1e-6, so
    the bound of the wider widths is 1e-5 too."""
    state, ni, nc, qi, ci, keep = parity_case(C, B, N, pos_embed, num_nodes)
    clf = make_clf(state, C, pos_embed, num_nodes)
    s, _, g = step_grads_n(clf, ni.to(DEV), nc.to(DEV), qi, ci, keep.to(DEV), B)
    s64, g64 = ref_step(state, ni, nc, qi, ci, keep, B)
    es = float((s.double().cpu() - s64).abs().max())
    errs = grad_errors({n: v.cpu() for n, v in g.items()}, g64, C)
    print(f"C {C} B {B} N {N}: scores {es:.3g} (std {float(s.std()):.3g}), gradients "
          + ", ".join(f"{n} {e:.3g}" for n, e in errs.items()))
    assert float(s.std()) > 1e-3
    assert es < TOL
    for n in GRAD_NAMES:
        assert errs[n] < TOL, (n, errs[n])
    assert errs["K"] < TOL * float(g64["attn.in_proj_bias"].abs().max()) + 1e-9
    if pos_embed:
        assert clf.positional_embedding.grad is None and not clf.positional_embedding.requires_grad


# ------------------------------------------------------------------------------------------------ 2. the reference's own steps
@pytest.fixture(scope="module")
def nodes_golden():
    from make_clf_train_nodes_golden import load_golden_inputs
    return load_golden_inputs()


@pytest.mark.parametrize("case", ["n128", "n70"])
def test_golden_train_steps(nodes_golden, case):
    from make_clf_train_golden import PARAM_NAMES, sample_index
    downstream, ops, _ = _mods()
    z, cases = nodes_golden
    p, steps, state = cases[case]
    z = {key[len(case) + 1:]: v for key, v in z.items() if key.startswith(case + "/")}
    B, k, nsteps, C = p["B"], p["k"], p["steps"], p["C"]
    clf = make_clf(state, C, True, p["num_nodes"])
    opt = torch.optim.Adam(clf.parameters(), lr=p["clf_lr"])
    grads0 = {}

    def pre_hook(o, args, kwargs):
        if not grads0:
            grads0.update({n: q.grad.detach().clone() for n, q in clf.named_parameters()})
    opt.register_step_pre_hook(pre_hook)
    P = (1 + k) * B
    keeps = [torch.from_numpy(np.unpackbits(z["keep_bits"][s], axis=-1)[:, :128].astype(np.float32)) for s in range(nsteps)]
    masks = iter([kb.to(DEV).div_(1.0 - p["p_drop"]) for kb in keeps])
    feats = iter(steps)

    def encode(model, x_i, x_j):
        st = next(feats)
        return tuple(torch.from_numpy(st[n]).to(DEV) for n in ("nodes_i", "nodes_j", "z_i", "z_j"))
    rec = []
    loader = [(torch.zeros(B, 1), torch.zeros(B, 1))] * nsteps
    ops.lib.nsid_debug_counters_reset()
    mean = downstream.train({"clf_lr": p["clf_lr"]}, loader, None, clf, opt, None, encode=encode,
                            draw_mask=lambda n, pd, dev: next(masks), on_step=lambda i, st: rec.append(st))
    cnt = ops.launch_counters()
    assert cnt["clf_attn_fwd_n"] == cnt["clf_attn_bwd_n"] == cnt["clf_seg_reduce_n"] == nsteps and cnt["clf_attn_fwd"] == 0
    for s, st in enumerate(rec):
        assert np.array_equal(st.hn.cpu().numpy(), z["hn"][s]), s
        q_ref = np.concatenate([np.arange(B), np.tile(np.arange(B), k)])
        c_ref = np.concatenate([np.arange(B) + B, z["hn"][s].reshape(-1)])
        assert np.array_equal(st.q_idx.numpy(), q_ref) and np.array_equal(st.c_idx.numpy(), c_ref)
        assert st.keep.shape == (P, 128)
        el, es = abs(float(st.loss) - float(z["losses"][s])), np.abs(st.scores.cpu().numpy().reshape(-1) - z["scores"][s]).max()
        print(f"{case} step {s}: loss |d| {el:.3g}, scores |d| {es:.3g}")
        assert el < TOL and es < TOL
    assert abs(mean - float(z["mean_loss"])) < TOL
    final = {n: q.detach().double().cpu() for n, q in clf.named_parameters()}
    for n in PARAM_NAMES:
        g = grads0[n].double().cpu()
        m = g.reshape(g.shape[0], -1) if g.dim() > 1 else g.reshape(1, -1)
        idx = sample_index(int(z["seed"]), tuple(g.shape), p)
        for part, got in (("rows", m.sum(1)), ("cols", m.sum(0)), ("samples", g.reshape(-1)[idx])):
            e = rel(got, z[f"grad0/{n}/{part}"])
            print(f"{case} {n}/{part}: {e:.3g}")
            assert e < TOL, (n, part, e)
        assert abs(float(g.norm()) / float(z[f"grad0/{n}/l2"][0]) - 1) < TOL, n
        # tests/test_clf_train_gpu.py's Adam rule: Adam's first steps move a weight by about lr sign(g); where |g_ref| is at
        # rounding level (below 1e-6 of the tensor's largest sampled gradient) that sign is noise and the element is bounded by 2 lr
        # steps; elsewhere within 1e-6
        g_ref = np.abs(z[f"grad0/{n}/samples"])
        noisy = g_ref < 1e-6 * g_ref.max()
        d = np.abs(final[n].reshape(-1)[idx].numpy() - z[f"final/{n}/samples"])
        assert (d[~noisy] <= 1e-6).all(), (n, d[~noisy].max())
        assert (d[noisy] <= 2 * p["clf_lr"] * nsteps).all(), n


# ------------------------------------------------------------------------------------------------ 3. counters and the dispatch
def _small_case(seed, B, N, C=512, num_nodes=128):
    state = rule_state(seed, C, True, num_nodes)
    ni, nj, zi, zj = features_cpu(seed, B, C, N)
    qi, ci = mined_pairs(zi, zj, B)
    keep = torch.empty(qi.numel(), 128).bernoulli_(0.7, generator=torch.Generator().manual_seed(seed)).div_(0.7)
    return state, ni.to(DEV), torch.cat([ni, nj]).to(DEV), qi, ci, keep.to(DEV)


def test_counters_at_64_nodes():
    _, ops, _ = _mods()
    B, N = 4, 64
    state, ni, nc, qi, ci, keep = _small_case(61, B, N)
    clf = make_clf(state, 512, True, 128)
    ops.lib.nsid_debug_counters_reset()
    step_grads_n(clf, ni, nc, qi, ci, keep, B)
    cnt = ops.launch_counters()
    assert [cnt[n] for n in MULTI] == [1, 1, 1, 2], cnt
    assert all(cnt[n] == 0 for n in ONE_TILE), cnt


@pytest.mark.parametrize("N", [32, 7])
def test_small_n_runs_the_one_tile_entries_bitwise(N):
    downstream, ops, _ = _mods()
    B = 4
    state, ni, nc, qi, ci, keep = _small_case(62 + N, B, N, num_nodes=32)
    clf = make_clf(state, 512, True, 32)
    ops.lib.nsid_debug_counters_reset()
    s_n, _, g_n = step_grads_n(clf, ni, nc, qi, ci, keep, B)
    g_n = {n: v.clone() for n, v in g_n.items()}
    cnt = ops.launch_counters()
    assert [cnt[n] for n in ONE_TILE] == [1, 1, 1, 2], cnt
    assert all(cnt[n] == 0 for n in MULTI), cnt
    clf.zero_grad(set_to_none=True)
    s = downstream.clf_train_scores(clf, ni, nc, qi, ci, keep)
    bce(s, B).backward()
    assert torch.equal(s.detach(), s_n)
    for n, q in clf.named_parameters():
        assert torch.equal(q.grad, g_n[n]), n


# ------------------------------------------------------------------------------------------------ 4. consistency with evaluation
@pytest.mark.parametrize("N,num_nodes", [(128, 128), (70, 100)])
def test_ones_mask_matches_pair_scores(N, num_nodes):
    downstream, _, _ = _mods()
    B = 4
    state, ni, nc, qi, ci, _ = _small_case(70 + N, B, N, num_nodes=num_nodes)
    clf = make_clf(state, 512, True, num_nodes)
    s = downstream.clf_train_scores_n(clf, ni, nc, qi, ci, torch.ones(qi.numel(), 128, device=DEV)).detach()
    clf.eval()
    with torch.no_grad():
        full = clf.pair_scores(ni, nc)
    e = float((s.view(-1) - full[qi, ci]).abs().max())
    print(f"N {N}: ones mask against pair_scores {e:.3g}")
    assert e < TOL


def test_trained_state_loads_into_rerank():
    downstream, ops, CAC = _mods()
    B, N = 4, 128
    state = rule_state(75, 512, True, 128)
    clf = make_clf(state, 512, True, 128)
    ni, nj, zi, zj = (t.to(DEV) for t in features_cpu(75, B, 512, N))
    clf.eval()
    with torch.no_grad():
        before = clf.pair_scores(ni, nj).clone()
    opt = torch.optim.Adam(clf.parameters(), lr=1e-3)
    ops.lib.nsid_debug_counters_reset()
    downstream.train_step(clf, opt, None, ni, nj, zi, zj)
    cnt = ops.launch_counters()
    assert cnt["clf_attn_fwd_n"] == 1 and cnt["clf_attn_bwd_n"] == 1 and cnt["clf_attn_fwd"] == 0
    clf.eval()
    with torch.no_grad():
        after = clf.pair_scores(ni, nj)
    assert not torch.equal(before, after)
    buf = io.BytesIO()
    torch.save(clf.state_dict(), buf)
    buf.seek(0)
    fresh = CAC(512, num_nodes=128).to(DEV)
    fresh.load_state_dict(torch.load(buf), strict=True)
    fresh.eval()
    with torch.no_grad():
        assert torch.equal(fresh.pair_scores(ni, nj), after)


# ------------------------------------------------------------------------------------------------ 5.-7. the ops functions
def _qkv(seed, Sq, Sc, N, C, pad_rows=0):
    """projected rows by rule: q (Sq N, C), kv (Sc N, 2 C), the leading rows of NaN-filled buffers when pad_rows > 0"""
    g = torch.Generator().manual_seed(seed)
    q, kv = torch.randn(Sq * N, C, generator=g), torch.randn(Sc * N, 2 * C, generator=g)
    if pad_rows:
        qf, kf = torch.full((Sq * N + pad_rows, C), float("nan")), torch.full((Sc * N + pad_rows, 2 * C), float("nan"))
        qf[:Sq * N], kf[:Sc * N] = q, kv
        return qf.to(DEV)[:Sq * N], kf.to(DEV)[:Sc * N]
    return q.to(DEV), kv.to(DEV)


def _run_n(ops, q, kv, N, qt, ct, dob, Sq, Sc):
    ob, attn, ab = ops.clf_attn_fwd_n(q, kv, N, qt, ct)
    dq, dk = ops.clf_attn_bwd_n(dob, attn, q, kv, N, qt, ct)
    seg = ops.clf_seg_reduce_n(dq, dk, ab, dob, qt, ct, N, Sq, Sc)
    return ob, attn, dq, dk, ab, seg[0], seg[1]


def _lists(Sq, Sc, P, seed):
    """P pairs: the last query and candidate segments in use, query 1 and candidate 2 in none, pairs 3 and 10 the same pair"""
    g = torch.Generator().manual_seed(seed)
    qi = torch.randint(0, Sq, (P,), generator=g)
    ci = torch.randint(0, Sc, (P,), generator=g)
    qi[qi == 1], ci[ci == 2] = 0, 3
    qi[0], ci[0] = Sq - 1, Sc - 1
    qi[10], ci[10] = qi[3], ci[3]
    return qi.to(torch.int32).to(DEV), ci.to(torch.int32).to(DEV)


@pytest.mark.parametrize("N", [97, 128])
def test_bitwise_reproducible_and_pair_independent(N):
    _, ops, _ = _mods()
    C, Sq, Sc, P = 512, 5, 6, 23
    nT = (N + 31) // 32
    q, kv = _qkv(80 + N, Sq, Sc, N, C)
    qt, ct = _lists(Sq, Sc, P, 81 + N)
    dob = torch.randn(P, C, generator=torch.Generator().manual_seed(82)).to(DEV)
    a, b = _run_n(ops, q, kv, N, qt, ct, dob, Sq, Sc), _run_n(ops, q, kv, N, qt, ct, dob, Sq, Sc)
    assert a[0].shape == (P, C) and a[1].shape == (P, 4, nT, nT, 16, 64) and a[2].shape == a[3].shape == (P, N, C)
    assert a[4].shape == (P, 4, 128) and a[5].shape == (Sq * N, C) and a[6].shape == (Sc * N, 2 * C)
    for x, y in zip(a, b):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    sub = torch.arange(5, P, 7)
    c = _run_n(ops, q, kv, N, qt[sub].contiguous(), ct[sub].contiguous(), dob[sub].contiguous(), Sq, Sc)
    for x, y in zip(c[:4], a[:4]):
        assert torch.equal(x, y[sub])                   # obar, attn, dq, dk: alone as inside the larger list
    # a repeated (query, candidate) pair: identical rows (dq, dk depend on dobar, which differs: compare obar, attn and abar)
    for x in (a[0], a[1], a[4]):
        assert torch.equal(x[3], x[10])
    same = dob.clone()
    same[10] = same[3]
    d = _run_n(ops, q, kv, N, qt, ct, same, Sq, Sc)
    assert torch.equal(d[2][3], d[2][10]) and torch.equal(d[3][3], d[3][10])
    # a segment with no pair gets exact zeros from the reduce; one with pairs does not
    assert float(a[5].view(Sq, N, C)[1].abs().max()) == 0.0 and float(a[6].view(Sc, N, 2 * C)[2].abs().max()) == 0.0
    assert float(a[5].view(Sq, N, C)[Sq - 1].abs().max()) > 0 and float(a[6].view(Sc, N, 2 * C)[Sc - 1].abs().max()) > 0
    # abar is a distribution over the N keys, zero past N; the rows of the saved attention sum to 1 per query
    assert float((a[4][..., :N].sum(-1) - 1).abs().max()) < 1e-5 and float(a[4][..., N:].abs().sum()) == 0.0
    assert abs(float(a[1][0, 0].sum()) - N) < 1e-3


@pytest.mark.parametrize("N", [33, 97])
def test_no_read_past_the_data(N):
    """q and kv are the leading rows of NaN-filled buffers that extend 160 rows further; the last query and candidate segments end
    at the last valid row. A read of any row at or beyond nq_seg N / nc_seg N would meet NaN."""
    _, ops, _ = _mods()
    C, Sq, Sc, P = 512, 5, 6, 23
    qt, ct = _lists(Sq, Sc, P, 91 + N)
    dob = torch.randn(P, C, generator=torch.Generator().manual_seed(92)).to(DEV)
    plain = _run_n(ops, *_qkv(90 + N, Sq, Sc, N, C), N, qt, ct, dob, Sq, Sc)
    q, kv = _qkv(90 + N, Sq, Sc, N, C, pad_rows=160)
    assert q.is_contiguous() and kv.is_contiguous() and q.shape == (Sq * N, C)
    padded = _run_n(ops, q, kv, N, qt, ct, dob, Sq, Sc)
    for x, y in zip(padded, plain):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)


@pytest.mark.parametrize("C", [512, 640])
def test_multi_tile_entries_at_32_nodes_match_the_one_tile_entries(C):
    _, ops, _ = _mods()
    N, Sq, Sc, P = 32, 5, 6, 23
    q, kv = _qkv(95 + C, Sq, Sc, N, C)
    qt, ct = _lists(Sq, Sc, P, 96)
    dob = torch.randn(P, C, generator=torch.Generator().manual_seed(97)).to(DEV)
    ops.lib.nsid_debug_counters_reset()
    ob_n, _, dq_n, dk_n, ab_n, dqs_n, dkvs_n = _run_n(ops, q, kv, N, qt, ct, dob, Sq, Sc)
    ob, attn, ab = ops.clf_attn_fwd(q, kv, N, qt, ct)
    dq, dk = ops.clf_attn_bwd(dob, attn, q, kv, N, qt, ct)
    dqs, dkvs = ops.clf_seg_reduce(dq, dk, ab, dob, qt, ct, N, Sq, Sc)
    cnt = ops.launch_counters()
    assert all(cnt[n] == 1 for n in MULTI[:3] + ONE_TILE[:3]), cnt
    for name, x, y in (("obar", ob_n, ob), ("abar", ab_n[..., :32], ab), ("dq", dq_n, dq), ("dk", dk_n, dk), ("dq_seg", dqs_n, dqs),
                       ("dkv_seg", dkvs_n, dkvs)):
        e = rel(x, y)
        print(f"C {C} {name}: {e:.3g}")
        assert e < TOL, (name, e)


# ------------------------------------------------------------------------------------------------ 8. the 256-mel encoder end to end
def test_256_mel_encoder_trains_end_to_end():
    from synth import GRAFP_CFG, synth_randn, synth_state
    from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
    from neuralsampleid_amd.simclr.simclr import SimCLR
    downstream, ops, CAC = _mods()
    cfg = dict(GRAFP_CFG, n_mels=256)
    model = SimCLR(cfg, GraphEncoder(cfg, in_channels=cfg["n_filters"], k=3, size="t"))
    model.load_state_dict(synth_state(model.state_dict()))
    model = model.to(DEV)
    x = (synth_randn("clftrainnodes_x", 8, 256, cfg["n_frames"]) * 20 - 40).to(DEV)
    x_i, x_j = x[:4].contiguous(), x[4:].contiguous()
    ni, nj, zi, zj = downstream.encode_pairs(model, x_i, x_j)
    assert ni.shape == nj.shape == (4, 512, 128) and ni.dtype == torch.float32 and bool(torch.isfinite(ni).all())
    clf = CAC(512, num_nodes=128).to(DEV)
    w0 = {n: p.detach().clone() for n, p in clf.named_parameters()}
    opt = torch.optim.Adam(clf.parameters(), lr=1e-4)
    ops.lib.nsid_debug_counters_reset()
    loss = downstream.train({"clf_lr": 1e-4}, [(x_i, x_j), (x_j, x_i)], model, clf, opt, None)
    cnt = ops.launch_counters()
    assert np.isfinite(loss)
    assert all(not torch.equal(w0[n], p) for n, p in clf.named_parameters())
    assert cnt["clf_attn_fwd"] == cnt["clf_attn_bwd"] == cnt["clf_seg_reduce"] == 0, cnt
    assert cnt["clf_attn_fwd_n"] == cnt["clf_attn_bwd_n"] == cnt["clf_seg_reduce_n"] == 2, cnt


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_launch_nothing():
    downstream, ops, CAC = _mods()
    B = 2
    clf128 = make_clf(rule_state(98, 512, True, 128), 512, True, 128)
    clf64 = make_clf(rule_state(99, 512, True, 64), 512, True, 64)
    clf576 = CAC(576, num_nodes=128).to(DEV)
    z = lambda S, C, N: torch.zeros(S, C, N, device=DEV)
    x64, x100, x129, x576 = z(B, 512, 64), z(B, 512, 100), z(B, 512, 129), z(B, 576, 64)
    qi, ci = np.arange(B), np.arange(B)
    keep = torch.ones(B, 128, device=DEV)
    it = torch.zeros(2, dtype=torch.int32, device=DEV)
    f = downstream.clf_train_scores_n
    ops.lib.nsid_debug_counters_reset()
    bad = [
        lambda: f(clf128, x129, x129, qi, ci, keep),                              # N = 129
        lambda: f(clf128, x64, x100, qi, ci, keep),                               # query N != candidate N
        lambda: f(clf64, x100, x100, qi, ci, keep),                               # num_nodes = 64 with N = 100
        lambda: f(clf576, x576, x576, qi, ci, keep),                              # width 576
        lambda: f(clf128, x64.clone().requires_grad_(True), x64, qi, ci, keep),
        lambda: f(clf128, x64, x64.clone().requires_grad_(True), qi, ci, keep),
        lambda: f(clf128, x64, x64, qi, ci + B, keep),
        lambda: f(clf128, x64, x64, qi - 1, ci, keep),
        lambda: f(clf128, x64, x64, qi[:1], ci, keep),
        lambda: f(clf128, x64, x64, qi.astype(np.float32), ci, keep),
        lambda: f(clf128, x64, x64, [], [], keep[:0]),
        lambda: f(clf128, x64, x64, qi, ci, keep[:1]),
        lambda: f(clf128, x64, x64, qi, ci, torch.ones(B, 64, device=DEV)),
        lambda: f(clf128, x64, x64, qi, ci, keep.double()),
        lambda: f(clf128, x64.double(), x64, qi, ci, keep),
        lambda: f(clf128, x64.cpu(), x64, qi, ci, keep),
        lambda: f(CAC(512, num_heads=8, num_nodes=128).to(DEV), x64, x64, qi, ci, keep),
        # the one-tile ops functions keep their bound
        lambda: ops.clf_attn_fwd(torch.zeros(2 * 33, 512, device=DEV), torch.zeros(2 * 33, 1024, device=DEV), 33, it, it),
        lambda: ops.clf_attn_bwd(torch.zeros(2, 512, device=DEV), torch.zeros(2, 4, 16, 64, device=DEV),
                                 torch.zeros(2 * 33, 512, device=DEV), torch.zeros(2 * 33, 1024, device=DEV), 33, it, it),
        lambda: ops.clf_seg_reduce(torch.zeros(2, 33, 512, device=DEV), torch.zeros(2, 33, 512, device=DEV),
                                   torch.zeros(2, 4, 32, device=DEV), torch.zeros(2, 512, device=DEV), it, it, 33, 2, 2),
        # and the multi-tile ones refuse N = 129 and a width outside the four
        lambda: ops.clf_attn_fwd_n(torch.zeros(2 * 129, 512, device=DEV), torch.zeros(2 * 129, 1024, device=DEV), 129, it, it),
        lambda: ops.clf_attn_fwd_n(torch.zeros(2 * 64, 576, device=DEV), torch.zeros(2 * 64, 1152, device=DEV), 64, it, it),
        lambda: ops.clf_seg_reduce_n(torch.zeros(2, 129, 512, device=DEV), torch.zeros(2, 129, 512, device=DEV),
                                     torch.zeros(2, 4, 128, device=DEV), torch.zeros(2, 512, device=DEV), it, it, 129, 2, 2),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises((ValueError, RuntimeError, NotImplementedError, TypeError)):
            fn()
        counters = ops.launch_counters()
        assert all(v == 0 for key, v in counters.items() if key.startswith("clf_")), (i, counters)
    with pytest.raises(ValueError, match="training"):
        downstream.clf_train_scores(clf128, x64, x64, qi, ci, keep)
    assert sum(ops.launch_counters().values()) == 0
