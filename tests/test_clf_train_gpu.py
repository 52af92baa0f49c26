"""Classifier training on the MI355X (neuralsampleid_amd/downstream.py, csrc/clf_train.hip): the reference's own three training steps
(tests/golden/clf_train.npz), parity with an fp64 nn.MultiheadAttention classifier, hard-negative mining against an fp64 ranking,
consistency with the re-rank path, run-to-run and batch invariance, an end-to-end run on the encoder, and argument checks."""
import io

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR = 1e-4


def _mods():
    from neuralsampleid_amd import downstream, ops
    from neuralsampleid_amd.classifier import CrossAttentionClassifier
    return downstream, ops, CrossAttentionClassifier


def rule_state(seed, pos_embed=True, num_nodes=32, w_scale=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    C, hid = 512, 128
    n = lambda *s, scale: torch.from_numpy((rng.standard_normal(s) * scale).astype(np.float32))
    sd = {"attn.in_proj_weight": n(3 * C, C, scale=C ** -0.5), "attn.in_proj_bias": n(3 * C, scale=0.1),
          "attn.out_proj.weight": n(C, C, scale=C ** -0.5), "attn.out_proj.bias": n(C, scale=0.1),
          "fc.0.weight": n(hid, C, scale=2.0 * C ** -0.5), "fc.0.bias": n(hid, scale=0.1),
          "fc.3.weight": n(1, hid, scale=w_scale * 2.0 * hid ** -0.5), "fc.3.bias": n(1, scale=0.1)}
    if pos_embed:
        sd["positional_embedding"] = n(1, num_nodes, C, scale=0.5)
    return sd


def make_clf(state, pos_embed=True, num_nodes=32):
    _, _, CAC = _mods()
    clf = CAC(512, num_nodes=num_nodes, pos_embed=pos_embed)
    clf.load_state_dict(state, strict=True)
    return clf.to(DEV)


class Ref64(nn.Module):
    """fp64 training-mode forward of the reference module with an explicit dropout keep mask"""

    def __init__(self, state, dtype=torch.float64):
        super().__init__()
        self.pos = "positional_embedding" in state
        if self.pos:
            self.register_buffer("positional_embedding", torch.zeros(state["positional_embedding"].shape))
        self.attn = nn.MultiheadAttention(embed_dim=512, num_heads=4, batch_first=True)
        self.fc = nn.Sequential(nn.Linear(512, 128), nn.ReLU(), nn.Dropout(p=0.3), nn.Linear(128, 1), nn.Sigmoid())
        self.load_state_dict(state, strict=True)
        self.to(dtype)

    def forward(self, x_i, x_j, keep):
        x_i, x_j = x_i.permute(0, 2, 1), x_j.permute(0, 2, 1)
        if self.pos:
            pos = self.positional_embedding[:, :x_i.shape[1], :]
            x_i, x_j = x_i + pos, x_j + pos
        a, _ = self.attn(x_i, x_j, x_j)
        h = self.fc[1](self.fc[0](a.mean(dim=1))) * keep
        return self.fc[4](self.fc[3](h))


GRAD_NAMES = ["attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "fc.0.weight", "fc.0.bias",
              "fc.3.weight", "fc.3.bias"]


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def fp64_step(state, nq, nc, qi, ci, keep, B):
    """fp64 scores and the eight parameter gradients of BCE(pos) + BCE(neg)"""
    m = Ref64(state)
    qi, ci = torch.as_tensor(qi), torch.as_tensor(ci)
    s = m(nq.double().cpu()[qi], nc.double().cpu()[ci], keep.double().cpu())
    crit = nn.BCELoss()
    loss = crit(s[:B], torch.ones(B, 1, dtype=torch.float64)) + crit(s[B:], torch.zeros(s.shape[0] - B, 1, dtype=torch.float64))
    loss.backward()
    return s.detach(), {n: p.grad for n, p in m.named_parameters()}


def step_grads(clf, nq, nc, qi, ci, keep, B):
    downstream, _, _ = _mods()
    clf.zero_grad(set_to_none=True)
    s = downstream.clf_train_scores(clf, nq, nc, qi, ci, keep)
    crit = nn.BCELoss()
    loss = crit(s[:B], torch.ones(B, 1, device=DEV)) + crit(s[B:], torch.zeros(s.shape[0] - B, 1, device=DEV))
    loss.backward()
    return s.detach(), {n: p.grad for n, p in clf.named_parameters()}


def features(seed, B, N, d=128):
    g = torch.Generator().manual_seed(seed)
    ni = torch.randn(B, 512, N, generator=g)
    nj = ni + 0.5 * torch.randn(B, 512, N, generator=g)
    zi = torch.nn.functional.normalize(torch.randn(B, d, generator=g), dim=1)
    zj = torch.nn.functional.normalize(zi + 0.6 * torch.randn(B, d, generator=g), dim=1)
    return [t.to(DEV).contiguous() for t in (ni, nj, zi, zj)]


# ------------------------------------------------------------------------------------------------ the reference's own steps
def test_golden_train_steps():
    from make_clf_train_golden import PARAM_NAMES, load_golden_inputs, sample_index
    downstream, _, _ = _mods()
    z, p, steps, state = load_golden_inputs()
    B, k, nsteps = p["B"], p["k"], p["steps"]
    clf = make_clf(state)
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
    mean = downstream.train({"clf_lr": p["clf_lr"]}, loader, None, clf, opt, None, encode=encode,
                            draw_mask=lambda n, pd, dev: next(masks), on_step=lambda i, st: rec.append(st))
    for s, st in enumerate(rec):
        assert np.array_equal(st.hn.cpu().numpy(), z["hn"][s]), s
        q_ref = np.concatenate([np.arange(B), np.tile(np.arange(B), k)])
        c_ref = np.concatenate([np.arange(B) + B, z["hn"][s].reshape(-1)])
        assert np.array_equal(st.q_idx.numpy(), q_ref) and np.array_equal(st.c_idx.numpy(), c_ref)
        assert st.keep.shape == (P, 128)
        assert abs(float(st.loss) - float(z["losses"][s])) < 1e-5, (s, float(st.loss), z["losses"][s])
        assert np.abs(st.scores.cpu().numpy().reshape(-1) - z["scores"][s]).max() < 1e-5
    assert abs(mean - float(z["mean_loss"])) < 1e-5
    final = {n: q.detach().double().cpu() for n, q in clf.named_parameters()}
    for n in PARAM_NAMES:
        g = grads0[n].double().cpu()
        m = g.reshape(g.shape[0], -1) if g.dim() > 1 else g.reshape(1, -1)
        idx = sample_index(int(z["seed"]), tuple(g.shape), p)
        for part, got in (("rows", m.sum(1)), ("cols", m.sum(0)), ("samples", g.reshape(-1)[idx])):
            assert rel(got, z[f"grad0/{n}/{part}"]) < 1e-5, (n, part, rel(got, z[f"grad0/{n}/{part}"]))
        assert abs(float(g.norm()) / float(z[f"grad0/{n}/l2"][0]) - 1) < 1e-5, n
        # Adam's first steps move a weight by about lr sign(g): where |g_ref| is at rounding level (below 1e-6 of the tensor's
        # largest sampled gradient) that sign is noise and the element is bounded by 2 lr steps; elsewhere within 1e-6
        g_ref = np.abs(z[f"grad0/{n}/samples"])
        floor = 1e-6 * g_ref.max()
        d = np.abs(final[n].reshape(-1)[idx].numpy() - z[f"final/{n}/samples"])
        noisy = g_ref < floor
        assert (d[~noisy] <= 1e-6).all(), (n, d[~noisy].max())
        assert (d[noisy] <= 2 * p["clf_lr"] * nsteps).all(), n


# ------------------------------------------------------------------------------------------------ fp64 parity
@pytest.mark.parametrize("pos_embed", [True, False])
@pytest.mark.parametrize("N", [1, 7, 31, 32])
@pytest.mark.parametrize("B", [2, 8, 32, 256])
def test_fp64_parity(B, N, pos_embed):
    downstream, _, _ = _mods()
    state = rule_state(100 + B + N, pos_embed)
    clf = make_clf(state, pos_embed)
    ni, nj, zi, zj = features(B * 64 + N, B, N)
    k = 3
    hn = downstream.mine_hard_negatives(zi, zj, torch.cat([zi, zj]), num_negatives=k)
    qi, ci = downstream.pair_lists(hn.cpu(), B)
    ci[B + 1: B + 1 + min(2 * B, k * B - 1)] = 0        # one candidate serves many pairs
    nc = torch.cat([ni, nj])
    P = qi.numel()
    keep = downstream.draw_keep(P, 0.3, DEV)
    s, g = step_grads(clf, ni, nc, qi, ci, keep, B)
    s64, g64 = fp64_step(state, ni, nc, qi, ci, keep, B)
    assert float((s.double().cpu() - s64).abs().max()) < 1e-5
    for n in GRAD_NAMES:
        if n == "attn.in_proj_bias":      # its K part is zero in exact arithmetic (softmax is shift-invariant): compare Q and V
            assert rel(g[n][:512], g64[n][:512]) < 1e-5 and rel(g[n][1024:], g64[n][1024:]) < 1e-5, n
            assert float(g[n][512:1024].abs().max()) < 1e-5 * float(g64[n].abs().max()) + 1e-9
        else:
            assert rel(g[n], g64[n]) < 1e-5, (n, rel(g[n], g64[n]))
    if pos_embed:
        assert clf.positional_embedding.grad is None and not clf.positional_embedding.requires_grad


@pytest.mark.parametrize("b2", [50.0, -50.0])
def test_saturated_sigmoid(b2):
    """|logit| > 20 everywhere. b2 = +50: fp32 scores are exactly 1, the negatives' BCE is clamped at log 0 = -100 and every
    gradient is exactly 0 (BCE's eps-clamped backward times s (1 - s) = 0), as torch's fp32 eager path gives. b2 = -50: scores of
    about 2e-22, where BCE's backward eps dominates; the gradients follow torch's fp32 eager classifier."""
    downstream, _, _ = _mods()
    B, N = 8, 32
    state = rule_state(7)
    state["fc.3.bias"] = torch.tensor([b2])
    clf = make_clf(state)
    ni, nj, zi, zj = features(5, B, N)
    qi, ci = downstream.pair_lists(downstream.mine_hard_negatives(zi, zj, torch.cat([zi, zj])).cpu(), B)
    nc = torch.cat([ni, nj])
    keep = downstream.draw_keep(qi.numel(), 0.3, DEV)
    s, g = step_grads(clf, ni, nc, qi, ci, keep, B)
    ref = Ref64(state, torch.float32)
    sr = ref(ni.cpu()[qi], nc.cpu()[ci], keep.cpu())
    crit = nn.BCELoss()
    loss_ref = crit(sr[:B], torch.ones(B, 1)) + crit(sr[B:], torch.zeros(sr.shape[0] - B, 1))
    loss_ref.backward()
    loss = crit(s[:B], torch.ones(B, 1, device=DEV)) + crit(s[B:], torch.zeros(s.shape[0] - B, 1, device=DEV))
    assert abs(float(loss) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref))
    assert float(((s.cpu() - sr.detach()).abs() / sr.detach().abs()).max()) < 1e-5
    for n, q in ref.named_parameters():
        assert torch.isfinite(g[n]).all(), n
        if b2 > 0:
            assert float(sr.detach().min()) == 1.0 and float(s.min()) == 1.0
            assert float(g[n].abs().max()) == 0.0 and float(q.grad.abs().max()) == 0.0, n
        elif n != "attn.in_proj_bias":
            assert rel(g[n], q.grad) < 1e-4, (n, rel(g[n], q.grad))


# ------------------------------------------------------------------------------------------------ mining
@pytest.mark.parametrize("B", [2, 8, 256, 4096])
def test_mining_vs_fp64(B):
    downstream, _, _ = _mods()
    k = 3
    _, _, zi, zj = features(B, B, 1)
    za = torch.cat([zi, zj])
    hn = downstream.mine_hard_negatives(zi, zj, za, num_negatives=k).cpu().numpy()
    sim = zi.double().cpu().numpy() @ za.double().cpu().numpy().T
    order = np.argsort(-sim, axis=1, kind="stable")[:, :k + 2]
    srt = np.take_along_axis(sim, order, 1)
    ok = (np.diff(-srt, axis=1) > 1e-6).all(1)
    assert ok.mean() > 0.9
    assert np.array_equal(hn[ok], order[ok, 1:k + 1])


def test_mining_ties_to_smaller_index():
    """exact duplicate rows give bitwise equal dots: the smaller index ranks first"""
    downstream, _, _ = _mods()
    B = 16
    _, _, zi, _ = features(3, B, 1)
    zj = zi.clone()                     # every row's positive view is an exact duplicate of it
    zj[3] = zi[5]                       # and row 5 has a third copy at 16 + 3
    hn = downstream.mine_hard_negatives(zi, zj, torch.cat([zi, zj]), num_negatives=4).cpu().numpy()
    for i in range(B):
        if i not in (3, 5):
            assert hn[i][0] == B + i, (i, hn[i])      # rank 0 = i itself, rank 1 = its duplicate
    assert list(hn[5][:2]) == [B + 3, B + 5]


def test_mining_refuses_small_pool():
    downstream, ops, _ = _mods()
    _, _, zi, zj = features(1, 1, 1)
    ops.lib.nsid_debug_counters_reset()
    with pytest.raises(ValueError):
        downstream.mine_hard_negatives(zi, zj, torch.cat([zi, zj]), num_negatives=2)
    assert ops.launch_counters().get("clf_mine", 0) == 0


# ------------------------------------------------------------------------------------------------ consistency with other paths
def test_ones_mask_matches_pair_scores():
    downstream, _, _ = _mods()
    B, N = 32, 32
    clf = make_clf(rule_state(11))
    ni, nj, zi, zj = features(11, B, N)
    nc = torch.cat([ni, nj])
    qi, ci = downstream.pair_lists(downstream.mine_hard_negatives(zi, zj, torch.cat([zi, zj])).cpu(), B)
    s = downstream.clf_train_scores(clf, ni, nc, qi, ci, torch.ones(qi.numel(), 128, device=DEV)).detach()
    clf.eval()
    with torch.no_grad():
        full = clf.pair_scores(ni, nc)
    assert float((s.view(-1) - full[qi, ci]).abs().max()) < 1e-5


def test_trained_state_loads_into_rerank():
    downstream, _, CAC = _mods()
    B, N = 8, 32
    clf = make_clf(rule_state(12))
    ni, nj, zi, zj = features(12, B, N)
    clf.eval()
    with torch.no_grad():
        before = clf.pair_scores(ni, nj).clone()
    opt = torch.optim.Adam(clf.parameters(), lr=1e-3)
    downstream.train_step(clf, opt, None, ni, nj, zi, zj)
    clf.eval()
    with torch.no_grad():
        after = clf.pair_scores(ni, nj)          # folded() rebuilt after the in-place Adam update
    assert not torch.equal(before, after)
    buf = io.BytesIO()
    torch.save(clf.state_dict(), buf)
    buf.seek(0)
    fresh = CAC(512, num_nodes=32).to(DEV)
    fresh.load_state_dict(torch.load(buf), strict=True)
    fresh.eval()
    with torch.no_grad():
        assert torch.equal(fresh.pair_scores(ni, nj), after)


def test_grad_scaler_steps():
    downstream, _, _ = _mods()
    B, N = 8, 32
    clf = make_clf(rule_state(13))
    ni, nj, zi, zj = features(13, B, N)
    w0 = clf.fc[0].weight.detach().clone()
    opt = torch.optim.Adam(clf.parameters(), lr=1e-3)
    scaler = torch.amp.GradScaler("cuda")
    st = downstream.train_step(clf, opt, scaler, ni, nj, zi, zj)
    assert torch.isfinite(st.loss)
    assert scaler.get_scale() == 65536.0          # finite gradients: no back-off
    assert not torch.equal(w0, clf.fc[0].weight)


def test_bitwise_reproducible_and_pair_independent():
    downstream, ops, _ = _mods()
    B, N = 32, 32
    clf = make_clf(rule_state(14))
    ni, nj, zi, zj = features(14, B, N)
    nc = torch.cat([ni, nj])
    qi, ci = downstream.pair_lists(downstream.mine_hard_negatives(zi, zj, torch.cat([zi, zj])).cpu(), B)
    keep = downstream.draw_keep(qi.numel(), 0.3, DEV)
    q = ops.linear_fwd(ops.clf_node_rows(ni, clf.positional_embedding[0]), clf.attn.in_proj_weight[:512],
                       clf.attn.in_proj_bias[:512], B * N, 512, 512)[0]
    kv = ops.linear_fwd(ops.clf_node_rows(nc, clf.positional_embedding[0]), clf.attn.in_proj_weight[512:],
                        clf.attn.in_proj_bias[512:], 2 * B * N, 1024, 512)[0]
    qt, ct = qi.to(torch.int32).to(DEV), ci.to(torch.int32).to(DEV)
    dob = torch.randn(qi.numel(), 512, device=DEV)

    def run(qt, ct, dob):
        ob, attn, ab = ops.clf_attn_fwd(q, kv, N, qt, ct)
        dq, dk = ops.clf_attn_bwd(dob, attn, q, kv, N, qt, ct)
        seg = ops.clf_seg_reduce(dq, dk, ab, dob, qt, ct, N, B, 2 * B)
        return ob, dq, dk, seg
    a, b = run(qt, ct, dob), run(qt, ct, dob)
    for x, y in zip(a[:3] + a[3], b[:3] + b[3]):
        assert torch.equal(x, y)
    sub = torch.arange(5, qi.numel(), 7)
    c = run(qt[sub].contiguous(), ct[sub].contiguous(), dob[sub].contiguous())
    for x, y in zip(c[:3], a[:3]):
        assert torch.equal(x, y[sub])
    s1 = downstream.clf_train_scores(clf, ni, nc, qi, ci, keep)
    s2 = downstream.clf_train_scores(clf, ni, nc, qi, ci, keep)
    assert torch.equal(s1, s2)


# ------------------------------------------------------------------------------------------------ end to end on the encoder
def test_encode_pairs_and_train_e2e(golden):
    from synth import GRAFP_CFG, synth_state
    from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
    from neuralsampleid_amd.fpdb import extract_node_matrices
    from neuralsampleid_amd.simclr.simclr import SimCLR
    downstream, _, CAC = _mods()
    g = golden("e2e_b8_k3")
    model = SimCLR(GRAFP_CFG, GraphEncoder(GRAFP_CFG, in_channels=GRAFP_CFG["n_filters"], k=3, size="t"))
    model.load_state_dict(synth_state(model.state_dict()))
    model = model.to(DEV)
    x_i, x_j = g.t("x_i").to(DEV), g.t("x_j").to(DEV)
    ni, nj, zi, zj = downstream.encode_pairs(model, x_i, x_j)
    assert torch.equal(ni, extract_node_matrices(model, x_i)) and torch.equal(nj, extract_node_matrices(model, x_j))
    model.eval()
    with torch.no_grad():
        _, _, ezi, ezj = model(x_i, x_j)
    assert torch.equal(zi, ezi) and torch.equal(zj, ezj)
    torch.manual_seed(0)
    clf = CAC(512, num_nodes=32).to(DEV)
    w0 = {n: p.detach().clone() for n, p in clf.named_parameters()}
    opt = torch.optim.Adam(clf.parameters(), lr=1e-4)
    loss = downstream.train({"clf_lr": 1e-4}, [(x_i, x_j), (x_j, x_i)], model, clf, opt, None)
    assert np.isfinite(loss)
    assert all(not torch.equal(w0[n], p) for n, p in clf.named_parameters())


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    downstream, ops, CAC = _mods()
    B, N = 4, 8
    clf = make_clf(rule_state(15))
    ni, nj, zi, zj = features(15, B, N)
    nc = torch.cat([ni, nj])
    qi, ci = np.arange(B), np.arange(B) + B
    keep = torch.ones(B, 128, device=DEV)
    ops.lib.nsid_debug_counters_reset()
    bad = [
        lambda: downstream.clf_train_scores(clf, ni.double(), nc, qi, ci, keep),
        lambda: downstream.clf_train_scores(clf, ni.cpu(), nc, qi, ci, keep),
        lambda: downstream.clf_train_scores(clf, ni.transpose(1, 2).contiguous().transpose(1, 2), nc, qi, ci, keep),
        lambda: downstream.clf_train_scores(clf, ni.clone().requires_grad_(True), nc, qi, ci, keep),
        lambda: downstream.clf_train_scores(clf, ni[:, :256].contiguous(), nc, qi, ci, keep),
        lambda: downstream.clf_train_scores(clf, torch.zeros(B, 512, 33, device=DEV), nc, qi, ci, keep),
        lambda: downstream.clf_train_scores(clf, ni, nc, qi, ci + 100, keep),
        lambda: downstream.clf_train_scores(clf, ni, nc, qi - 1, ci, keep),
        lambda: downstream.clf_train_scores(clf, ni, nc, qi[:2], ci, keep),
        lambda: downstream.clf_train_scores(clf, ni, nc, qi, ci, keep[:2]),
        lambda: downstream.clf_train_scores(clf, ni, nc, qi, ci, keep.double()),
        lambda: downstream.clf_train_scores(CAC(256, num_nodes=32).to(DEV), ni, nc, qi, ci, keep),
        lambda: downstream.clf_train_scores(CAC(512, num_heads=8, num_nodes=32).to(DEV), ni, nc, qi, ci, keep),
        lambda: downstream.draw_keep(4, 1.0, DEV),
        lambda: downstream.draw_keep(4, -0.1, DEV),
        lambda: downstream.mine_hard_negatives(zi.double(), zj, torch.cat([zi, zj])),
        lambda: downstream.mine_hard_negatives(zi.cpu(), zj, torch.cat([zi, zj]).cpu()),
    ]
    for i, f in enumerate(bad):
        with pytest.raises((ValueError, RuntimeError, NotImplementedError, TypeError)):
            f()
        counters = ops.launch_counters()
        assert all(v == 0 for key, v in counters.items() if key.startswith("clf_")), (i, counters)
