"""Stage-2 classifier at in_dim 640, 768 and 1024 on the MI355X (csrc/rerank.hip, csrc/clf_train.hip through classifier.py,
downstream.py and ops.py): the reference's own scores, training step and gradients (tests/golden/clf_wide.npz), parity of the eval
re-rank and of training with an fp64 nn.MultiheadAttention restatement of the reference module, consistency between the two paths,
bitwise reproducibility and pair independence, a size-'s' encoder end to end, and refusals that launch nothing.

The bound 1e-5 (scores absolute, gradients relative L2) is the one the project uses at 512: the reference module's own fp32 against
its fp64 is 5.5e-7 (scores) and 1.1e-6 (gradients) at worst over the four widths, so 1e-5 leaves about 10x for another fixed
summation order. The training cases draw their dropout masks from seeded generators and keep the one-element fc.3.bias
gradient well conditioned (conditioned_keep); no test here depends on, or changes, the state of torch's global generators."""
import io

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDE = (640, 768, 1024)
GRAD_NAMES = ["attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "fc.0.weight", "fc.0.bias",
              "fc.3.weight", "fc.3.bias"]


def _mods():
    from neuralsampleid_amd import downstream, ops
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    return downstream, ops, CrossAttentionClassifier


def rule_state(seed, C, pos_embed=True, num_nodes=32):
    rng = np.random.Generator(np.random.PCG64(seed))
    hid = 128
    n = lambda *s, scale: torch.from_numpy((rng.standard_normal(s) * scale).astype(np.float32))
    sd = {"attn.in_proj_weight": n(3 * C, C, scale=C ** -0.5), "attn.in_proj_bias": n(3 * C, scale=0.1),
          "attn.out_proj.weight": n(C, C, scale=C ** -0.5), "attn.out_proj.bias": n(C, scale=0.1),
          "fc.0.weight": n(hid, C, scale=2.0 * C ** -0.5), "fc.0.bias": n(hid, scale=0.1),
          "fc.3.weight": n(1, hid, scale=2.0 * hid ** -0.5), "fc.3.bias": n(1, scale=0.1)}
    if pos_embed:
        sd["positional_embedding"] = n(1, num_nodes, C, scale=0.5)
    return sd


def make_clf(state, C, pos_embed=True, num_nodes=32):
    _, _, CAC = _mods()
    clf = CAC(C, num_nodes=num_nodes, pos_embed=pos_embed)
    clf.load_state_dict(state, strict=True)
    return clf.to(DEV)


class Ref64(nn.Module):
    """the reference module (downstream.py:30-78) in fp64 on the CPU, with an explicit dropout keep mask (None: eval mode)"""

    def __init__(self, state):
        super().__init__()
        C = state["attn.out_proj.weight"].shape[0]
        self.pos = "positional_embedding" in state
        if self.pos:
            self.register_buffer("positional_embedding", torch.zeros(state["positional_embedding"].shape))
        self.attn = nn.MultiheadAttention(embed_dim=C, num_heads=4, batch_first=True)
        self.fc = nn.Sequential(nn.Linear(C, 128), nn.ReLU(), nn.Dropout(p=0.3), nn.Linear(128, 1), nn.Sigmoid())
        self.load_state_dict(state, strict=True)
        self.double()

    def forward(self, x_i, x_j, keep=None):
        return self.head(self.hidden(x_i, x_j), keep)

    def hidden(self, x_i, x_j):
        """the (P, 128) hidden activations after the ReLU, before the dropout"""
        x_i, x_j = x_i.permute(0, 2, 1), x_j.permute(0, 2, 1)
        if self.pos:
            pos = self.positional_embedding[:, :x_i.shape[1], :]
            x_i, x_j = x_i + pos, x_j + pos
        a, _ = self.attn(x_i, x_j, x_j)
        return self.fc[1](self.fc[0](a.mean(dim=1)))

    def head(self, h, keep=None):
        if keep is not None:
            h = h * keep
        return self.fc[4](self.fc[3](h))


def fp64_pair_scores(state, nm_q, nm_c):
    """(Sq, Sc) fp64 eval-mode scores of every pair"""
    m = Ref64(state)
    q, c = nm_q.double().cpu(), nm_c.double().cpu()
    Sq, Sc = q.shape[0], c.shape[0]
    qi, ci = np.divmod(np.arange(Sq * Sc), Sc)
    with torch.no_grad():
        return m(q[qi], c[ci])[:, 0].reshape(Sq, Sc)


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def nodes(seed, S, C, N):
    return torch.randn(S, C, N, generator=torch.Generator().manual_seed(seed)).to(DEV).contiguous()


def features(seed, B, C, N, d=128):
    g = torch.Generator().manual_seed(seed)
    ni = torch.randn(B, C, N, generator=g)
    nj = ni + 0.5 * torch.randn(B, C, N, generator=g)
    zi = torch.nn.functional.normalize(torch.randn(B, d, generator=g), dim=1)
    zj = torch.nn.functional.normalize(zi + 0.6 * torch.randn(B, d, generator=g), dim=1)
    return [t.to(DEV).contiguous() for t in (ni, nj, zi, zj)]


@pytest.fixture(autouse=True)
def own_rng():
    """every test here runs on a fixed seed and hands torch's generators (host and device) back as it found them, so neither
    its own draws nor those of the tests that run after this file depend on the order of the run"""
    with torch.random.fork_rng(devices=[torch.cuda.current_device()]):
        torch.manual_seed(20)
        yield


def conditioned_keep(state, nq, nc, qi, ci, B, seed, p=0.3):
    """(P, 128) dropout keep mask / (1 - p) from a seeded generator; the seed moves on until the step is well conditioned.

    fc.3.bias has one element: its gradient is g = sum_p w_p (s_p - y_p), w = 1/B on the B positives and 1/(P - B) on the
    negatives, terms of both signs around +-0.5 w_p that cancel. An fp32 score carries an error d_p however it is summed (the
    reference module's own fp32 against its fp64: up to 5.5e-7), so g is off by sum_p w_p d_p and its relative error is that times
    the condition number kappa = sum_p |w_p (s_p - y_p)| / |g|: measured on the reference module's fp32 at these cases, about
    7e-8 times kappa at B = 8 (3.4e-6 at kappa = 45). The bound 1e-5 is meant to leave about 10x over the reference's own rounding, 1e-6,
    which holds up to kappa = 1e-6 / 7e-8 = 14; masks with kappa > 14 (about half of them at B = 8, none at B = 2) test the draw,
    not the kernels. kappa comes from the fp64 module alone, as the golden generators' margins do."""
    m = Ref64(state)
    qi, ci = torch.as_tensor(qi), torch.as_tensor(ci)
    P = qi.numel()
    y = torch.cat([torch.ones(B), torch.zeros(P - B)]).double()
    w = torch.cat([torch.full((B,), 1.0 / B), torch.full((P - B,), 1.0 / (P - B))]).double()
    with torch.no_grad():
        h = m.hidden(nq.double().cpu()[qi], nc.double().cpu()[ci])
        for seed in range(seed, seed + 64):
            keep = torch.empty(P, 128).bernoulli_(1.0 - p, generator=torch.Generator().manual_seed(seed)).div_(1.0 - p)
            t = w * (m.head(h, keep.double())[:, 0] - y)
            kappa = float(t.abs().sum() / t.sum().abs())
            if kappa <= 14.0:
                print(f"keep mask seed {seed}: kappa {kappa:.3g}")
                return keep.to(DEV)
    raise AssertionError("no well-conditioned dropout mask in 64 seeds")


def bce(s, B):
    crit = nn.BCELoss()
    return crit(s[:B], torch.ones(B, 1, dtype=s.dtype, device=s.device)) + crit(
        s[B:], torch.zeros(s.shape[0] - B, 1, dtype=s.dtype, device=s.device))


def fp64_step(state, nq, nc, qi, ci, keep, B):
    m = Ref64(state)
    qi, ci = torch.as_tensor(qi), torch.as_tensor(ci)
    s = m(nq.double().cpu()[qi], nc.double().cpu()[ci], keep.double().cpu())
    bce(s, B).backward()
    return s.detach(), {n: p.grad for n, p in m.named_parameters()}


def step_grads(clf, nq, nc, qi, ci, keep, B):
    downstream, _, _ = _mods()
    clf.zero_grad(set_to_none=True)
    s = downstream.clf_train_scores(clf, nq, nc, qi, ci, keep)
    loss = bce(s, B)
    loss.backward()
    return s.detach(), loss.detach(), {n: p.grad for n, p in clf.named_parameters()}


def check_grads(g, g64, C):
    for n in GRAD_NAMES:
        if n == "attn.in_proj_bias":      # its K part is zero in exact arithmetic (softmax is shift-invariant): compare Q and V
            eq, ev = rel(g[n][:C], g64[n][:C]), rel(g[n][2 * C:], g64[n][2 * C:])
            print(f"C {C} {n}: Q {eq:.3g} V {ev:.3g} K max {float(g[n][C:2 * C].abs().max()):.3g}")
            assert eq < 1e-5 and ev < 1e-5, (n, eq, ev)
            assert float(g[n][C:2 * C].abs().max()) < 1e-5 * float(g64[n].abs().max()) + 1e-9
        else:
            e = rel(g[n], g64[n])
            print(f"C {C} {n}: {e:.3g}")
            assert e < 1e-5, (n, e)


# ------------------------------------------------------------------------------------------------ the reference's own numbers
@pytest.fixture(scope="module")
def wide_golden():
    from make_clf_wide_golden import load_golden_inputs
    return load_golden_inputs()


@pytest.mark.parametrize("C", WIDE)
def test_golden_eval_scores(wide_golden, C):
    z, cases = wide_golden
    p, ev, _, state = cases[C]
    clf = make_clf(state, C).eval()
    with torch.no_grad():
        s32 = clf.pair_scores(torch.from_numpy(ev[0]).to(DEV), torch.from_numpy(ev[1]).to(DEV)).cpu().numpy()
        s7 = clf.pair_scores(torch.from_numpy(ev[2]).to(DEV), torch.from_numpy(ev[3]).to(DEV)).cpu().numpy()
    e32, e7 = np.abs(s32 - z[f"{C}/eval_scores"]).max(), np.abs(s7 - z[f"{C}/eval7_scores"]).max()
    print(f"C {C}: eval |d| N=32 {e32:.3g}, N=7 {e7:.3g}")
    assert e32 < 1e-5 and e7 < 1e-5


@pytest.mark.parametrize("C", WIDE)
def test_golden_train_step(wide_golden, C):
    from make_clf_train_golden import PARAM_NAMES, sample_index
    downstream, _, _ = _mods()
    z, cases = wide_golden
    p, _, steps, state = cases[C]
    B, k, st = p["B"], p["k"], steps[0]
    clf = make_clf(state, C).train()
    ni, nj, zi, zj = (torch.from_numpy(st[n]).to(DEV) for n in ("nodes_i", "nodes_j", "z_i", "z_j"))
    hn = downstream.mine_hard_negatives(zi, zj, torch.cat([zi, zj]), num_negatives=k)
    assert np.array_equal(hn.cpu().numpy(), z[f"{C}/hn"])
    qi, ci = downstream.pair_lists(hn.cpu(), B)
    keep = torch.from_numpy(np.unpackbits(z[f"{C}/keep_bits"], axis=-1)[:, :128].astype(np.float32)).to(DEV).div_(1.0 - p["p_drop"])
    s, loss, g = step_grads(clf, ni, torch.cat([ni, nj]), qi, ci, keep, B)
    es, el = np.abs(s.cpu().numpy().reshape(-1) - z[f"{C}/scores"]).max(), abs(float(loss) - float(z[f"{C}/loss"]))
    print(f"C {C}: train scores |d| {es:.3g}, loss |d| {el:.3g}")
    assert es < 1e-5 and el < 1e-5
    for n in PARAM_NAMES:
        gn = g[n].double().cpu()
        m = gn.reshape(gn.shape[0], -1) if gn.dim() > 1 else gn.reshape(1, -1)
        idx = sample_index(int(z[f"{C}/seed"]), tuple(gn.shape), p)
        for part, got in (("rows", m.sum(1)), ("cols", m.sum(0)), ("samples", gn.reshape(-1)[idx])):
            e = rel(got, z[f"{C}/grad0/{n}/{part}"])
            print(f"C {C} {n}/{part}: {e:.3g}")
            assert e < 1e-5, (n, part, e)
        assert abs(float(gn.norm()) / float(z[f"{C}/grad0/{n}/l2"][0]) - 1) < 1e-5, n


# ------------------------------------------------------------------------------------------------ eval re-rank against fp64
@pytest.mark.parametrize("pos_embed", [True, False])
@pytest.mark.parametrize("N", [1, 7, 31, 32])
@pytest.mark.parametrize("C", WIDE)
def test_eval_fp64_parity(C, N, pos_embed):
    Sq, Sc = 5, 3
    state = rule_state(200 + C + N, C, pos_embed)
    clf = make_clf(state, C, pos_embed).eval()
    nq, nc = nodes(C + N, Sq, C, N), nodes(C + N + 1, Sc, C, N)
    ref = fp64_pair_scores(state, nq, nc)
    with torch.no_grad():
        s = clf.pair_scores(nq, nc)
        f = clf(nq[:Sc].contiguous(), nc)
    e = float((s.double().cpu() - ref).abs().max())
    ef = float((f.double().cpu().view(-1) - ref[:Sc].diagonal()).abs().max())
    print(f"C {C} N {N} pos {pos_embed}: pair_scores {e:.3g}, forward {ef:.3g}")
    assert s.shape == (Sq, Sc) and f.shape == (Sc, 1)
    assert e < 1e-5 and ef < 1e-5


@pytest.mark.parametrize("C", WIDE)
def test_eval_crosses_the_query_chunk(C):
    """65 query segments: two workgroups per candidate, the second with a single segment"""
    N = 32
    state = rule_state(300 + C, C)
    clf = make_clf(state, C).eval()
    nq, nc = nodes(C + 2, 65, C, N), nodes(C + 3, 2, C, N)
    with torch.no_grad():
        s = clf.pair_scores(nq, nc)
    e = float((s.double().cpu() - fp64_pair_scores(state, nq, nc)).abs().max())
    print(f"C {C}: 65 x 2 {e:.3g}")
    assert e < 1e-5


@pytest.mark.parametrize("C", WIDE)
def test_score_blocks_two_groups(C):
    N = 7
    state = rule_state(400 + C, C)
    clf = make_clf(state, C).eval()
    nq, nc = nodes(C + 4, 6, C, N), nodes(C + 5, 5, C, N)
    ref = fp64_pair_scores(state, nq, nc)
    with torch.no_grad():
        q, kp = clf.project_queries(nq), clf.project_candidates(nc)
        assert q.shape == (6 * N, C) and kp.shape == (5 * N, C + 512)
        # group 0: queries 0..3 x candidates (4, 1, 1); group 1: queries 4..5 x candidates (0, 2, 3, 4)
        out, off = clf.score_blocks(q, kp, N, [0, 4], [4, 2], [4, 1, 1, 0, 2, 3, 4], [0, 3], [3, 4])
    out = out.double().cpu()
    assert out.numel() == 4 * 3 + 2 * 4 and off.tolist() == [0, 12]
    g0, g1 = out[:12].view(4, 3), out[12:].view(2, 4)
    assert float((g0 - ref[:4][:, [4, 1, 1]]).abs().max()) < 1e-5
    assert float((g1 - ref[4:][:, [0, 2, 3, 4]]).abs().max()) < 1e-5
    assert torch.equal(g0[:, 1], g0[:, 2])                      # a repeated candidate: bitwise the same score


# ------------------------------------------------------------------------------------------------ training against fp64
@pytest.mark.parametrize("N", [1, 7, 32])
@pytest.mark.parametrize("B", [2, 8])
@pytest.mark.parametrize("C", WIDE)
def test_train_fp64_parity(C, B, N):
    downstream, _, _ = _mods()
    k = 3
    state = rule_state(500 + C + B + N, C)
    clf = make_clf(state, C)
    ni, nj, zi, zj = features(C + B * 64 + N, B, C, N)
    hn = downstream.mine_hard_negatives(zi, zj, torch.cat([zi, zj]), num_negatives=k)
    qi, ci = downstream.pair_lists(hn.cpu(), B)
    ci[B + 1: B + 1 + min(2 * B, k * B - 1)] = 0        # one candidate serves many pairs
    nc = torch.cat([ni, nj])
    keep = conditioned_keep(state, ni, nc, qi, ci, B, seed=600 + C + B + N)
    s, _, g = step_grads(clf, ni, nc, qi, ci, keep, B)
    s64, g64 = fp64_step(state, ni, nc, qi, ci, keep, B)
    es = float((s.double().cpu() - s64).abs().max())
    print(f"C {C} B {B} N {N}: scores {es:.3g}")
    assert es < 1e-5
    check_grads(g, g64, C)
    assert clf.positional_embedding.grad is None and not clf.positional_embedding.requires_grad


# ------------------------------------------------------------------------------------------------ consistency, reproducibility
def test_trained_640_loads_into_eval_and_matches_ones_mask():
    downstream, _, CAC = _mods()
    C, B, N = 640, 8, 32
    clf = make_clf(rule_state(21, C), C)
    ni, nj, zi, zj = features(21, B, C, N)
    opt = torch.optim.Adam(clf.parameters(), lr=1e-3)
    downstream.train_step(clf, opt, None, ni, nj, zi, zj)
    buf = io.BytesIO()
    torch.save(clf.state_dict(), buf)
    buf.seek(0)
    fresh = CAC(C, num_nodes=32).to(DEV)
    fresh.load_state_dict(torch.load(buf), strict=True)
    nc = torch.cat([ni, nj])
    qi, ci = downstream.pair_lists(downstream.mine_hard_negatives(zi, zj, torch.cat([zi, zj])).cpu(), B)
    s = downstream.clf_train_scores(fresh, ni, nc, qi, ci, torch.ones(qi.numel(), 128, device=DEV)).detach()
    fresh.eval()
    with torch.no_grad():
        full = fresh.pair_scores(ni, nc)
    e = float((s.view(-1) - full[qi, ci]).abs().max())
    print(f"ones mask vs pair_scores at 640: {e:.3g}")
    assert e < 1e-6


def test_bitwise_reproducible_and_pair_independent_1024():
    downstream, ops, _ = _mods()
    C, B, N = 1024, 8, 32
    clf = make_clf(rule_state(22, C), C)
    ni, nj, zi, zj = features(22, B, C, N)
    nc = torch.cat([ni, nj])
    qi, ci = downstream.pair_lists(downstream.mine_hard_negatives(zi, zj, torch.cat([zi, zj])).cpu(), B)
    P = qi.numel()
    pos = clf.positional_embedding[0]
    q = ops.linear_fwd(ops.clf_node_rows(ni, pos), clf.attn.in_proj_weight[:C], clf.attn.in_proj_bias[:C], B * N, C, C)[0]
    kv = ops.linear_fwd(ops.clf_node_rows(nc, pos), clf.attn.in_proj_weight[C:], clf.attn.in_proj_bias[C:], 2 * B * N, 2 * C, C)[0]
    qt, ct = qi.to(torch.int32).to(DEV), ci.to(torch.int32).to(DEV)
    dob = torch.randn(P, C, device=DEV)

    def run(qt, ct, dob):
        ob, attn, ab = ops.clf_attn_fwd(q, kv, N, qt, ct)
        dq, dk = ops.clf_attn_bwd(dob, attn, q, kv, N, qt, ct)
        seg = ops.clf_seg_reduce(dq, dk, ab, dob, qt, ct, N, B, 2 * B)
        return ob, dq, dk, seg
    a, b = run(qt, ct, dob), run(qt, ct, dob)
    assert a[0].shape == (P, C) and a[1].shape == (P, N, C) and a[3][0].shape == (B * N, C) and a[3][1].shape == (2 * B * N, 2 * C)
    for x, y in zip(a[:3] + a[3], b[:3] + b[3]):
        assert torch.equal(x, y)
    sub = torch.arange(2, P, 5)
    c = run(qt[sub].contiguous(), ct[sub].contiguous(), dob[sub].contiguous())
    for x, y in zip(c[:3], a[:3]):
        assert torch.equal(x, y[sub])                   # per-pair outputs: alone as inside the larger list
    keep = downstream.draw_keep(P, 0.3, DEV)
    assert torch.equal(downstream.clf_train_scores(clf, ni, nc, qi, ci, keep), downstream.clf_train_scores(clf, ni, nc, qi, ci, keep))
    # the eval path: a pair's score alone, in the full matrix, and in a second run
    clf.eval()
    with torch.no_grad():
        full, again = clf.pair_scores(ni, nc), clf.pair_scores(ni, nc)
        one = clf.pair_scores(ni[3:4].contiguous(), nc[5:6].contiguous())
    assert torch.equal(full, again) and torch.equal(one[0, 0], full[3, 5])


# ------------------------------------------------------------------------------------------------ end to end on a size-'s' encoder
def test_size_s_encoder_end_to_end():
    from synth import GRAFP_CFG, synth_clips, synth_state
    from neuralsampleid_amd.encoder.dgl.graph_encoder import GraphEncoderDGL
    from neuralsampleid_amd.fpdb import extract_node_matrices
    from neuralsampleid_amd.simclr.simclr import SimCLR
    torch.manual_seed(0)
    model = SimCLR(GRAFP_CFG, GraphEncoderDGL(cfg=GRAFP_CFG, in_channels=8, k=3, size="s"))
    model.load_state_dict(synth_state(model.state_dict()))
    model = model.to(DEV).eval()
    x, _ = synth_clips(4)
    nm = extract_node_matrices(model, x.to(DEV))
    assert nm.shape == (4, 640, 32) and nm.dtype == torch.float32
    state = rule_state(23, 640)
    clf = make_clf(state, 640).eval()
    with torch.no_grad():
        s = clf.pair_scores(nm, nm)
    e = float((s.double().cpu() - fp64_pair_scores(state, nm, nm)).abs().max())
    print(f"size 's' end to end: {e:.3g}")
    assert e < 1e-5


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    downstream, ops, CAC = _mods()
    clf640 = make_clf(rule_state(24, 640), 640).eval()
    clf768 = make_clf(rule_state(25, 768), 768).eval()
    clf576 = CAC(576, num_nodes=32).to(DEV).eval()
    x576, x512, x640 = nodes(1, 2, 576, 8), nodes(2, 2, 512, 32), nodes(3, 2, 640, 32)
    x768_33 = torch.zeros(2, 768, 33, device=DEV)
    tail = torch.zeros(257, device=DEV)
    q640 = torch.zeros(2 * 8, 640, device=DEV)
    keep = torch.ones(2, 128, device=DEV)
    ops.lib.nsid_debug_counters_reset()
    with torch.no_grad():
        bad = [
            (NotImplementedError, lambda: clf576.pair_scores(x576, x576)),
            (NotImplementedError, lambda: downstream.clf_train_scores(clf576, x576, x576, [0, 1], [0, 1], keep)),
            (ValueError, lambda: clf640.pair_scores(x512, x512)),
            (ValueError, lambda: clf640.pair_scores(x640, x512)),
            (ValueError, lambda: clf640(x640, x512)),
            (ValueError, lambda: downstream.clf_train_scores(clf640, x512, x512, [0, 1], [0, 1], keep)),
            (ValueError, lambda: clf768.pair_scores(x768_33, x768_33)),
            (ValueError, lambda: downstream.clf_train_scores(clf768, x768_33, x768_33, [0, 1], [0, 1], keep)),
            # kp of a width that matches no supported C for this q: 640 + 512 = 1152 is the only one
            (ValueError, lambda: ops.clf_pair_scores(q640, torch.zeros(2 * 8, 1024, device=DEV), 8, tail, [0], [2], [0, 1], [0], [2])),
            (ValueError, lambda: ops.clf_pair_scores(torch.zeros(16, 576, device=DEV), torch.zeros(16, 1088, device=DEV), 8, tail,
                                                     [0], [2], [0, 1], [0], [2])),
            (ValueError, lambda: ops.clf_attn_fwd(torch.zeros(16, 576, device=DEV), torch.zeros(16, 1152, device=DEV), 8,
                                                  torch.zeros(2, dtype=torch.int32, device=DEV),
                                                  torch.zeros(2, dtype=torch.int32, device=DEV))),
        ]
        for i, (exc, f) in enumerate(bad):
            with pytest.raises(exc):
                f()
            counters = ops.launch_counters()
            assert all(v == 0 for key, v in counters.items() if key.startswith("clf_")), (i, counters)
