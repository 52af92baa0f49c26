"""fp64 restatement of the baseline's training objective (simclr/triplet.py:6-61, baseline/train.py:66-77) in plain torch, and the
inputs of its tests. Not a test module: tests/test_baseline_loss_cpu.py checks it against tests/golden/baseline_loss.npz (written from
the reference's own functions by tests/golden/make_baseline_loss_golden.py), tests/test_baseline_loss_gpu.py uses both.

Definitions (M rows, S = E E^T):
  classifier_loss(z_i, z_j): z = cat(z_i, z_j), diagonal of S at -inf, target of row i = (i + B) mod M, mean cross-entropy.
  triplet_loss(E, labels, margin): pos[a] = max S_ab over b != a with equal labels (-inf if none, p* = first arg-max);
    neg[a] = min S_ab over unequal labels with S_ab > pos[a] - margin (n* = first arg-min); a is valid iff such b exists;
    loss = mean over valid a of relu(pos[a] - neg[a] + margin), 0 if no anchor is valid.
  objective: beta * classifier_loss(z_i, z_j) + gamma * triplet_loss(normalize(cat(z_i, z_j)), cat(arange(B), arange(B)), margin)."""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

MARGIN = 0.2
GAP_MIN = 1e-5          # anchors whose decision gap is below this may legitimately decide differently in another summation order

# name -> (kind, args). "pair": inputs (z_i, z_j) of the objective; "triplet": (embeddings, labels) of triplet_loss alone
CASES = {
    "r8x64": ("pair", dict(B=8, D=64, G=2, seed=1)),       # seed 0 leaves every anchor valid
    "r40x2048": ("pair", dict(B=40, D=2048, G=4, seed=0)),
    "r72x256": ("pair", dict(B=72, D=256, G=6, seed=0)),
    "b1": ("pair", dict(B=1, D=64, G=1, seed=0)),
    "b3x16": ("pair", dict(B=3, D=16, G=2, seed=0)),
    "novalid": ("pair", dict(B=8, D=64, G=0, seed=0)),
    "labels20": ("triplet", dict(M=20, D=64, seed=0)),
    "hand8": ("triplet", dict(M=8, D=16, seed=0)),
}
RECIPE = ("r8x64", "r40x2048", "r72x256")


def recipe(B, D, G, seed):
    """clustered pairs with per-clip noise scales: unstructured unit vectors at D = 2048 would make validity all-or-nothing"""
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(G, D, generator=g)
    sc = 0.2 + 0.7 * torch.rand(B, 1, generator=g)
    sv = 0.2 + 0.8 * torch.rand(B, 1, generator=g)
    base = c[torch.arange(B) % G] + sc * torch.randn(B, D, generator=g)
    z_i = F.normalize(base + sv * torch.randn(B, D, generator=g), dim=1)
    z_j = F.normalize(base + sv * torch.randn(B, D, generator=g), dim=1)
    return z_i.contiguous(), z_j.contiguous()


def make_case(name):
    """fp32 CPU inputs of a case: (z_i, z_j) or (embeddings, labels)"""
    kind, a = CASES[name]
    if name == "novalid":            # orthonormal clips, both views equal: pos = 1, every negative 0 <= pos - margin
        z = torch.eye(a["B"], a["D"])
        return z.clone(), z.clone()
    if kind == "pair":
        return recipe(a["B"], a["D"], a["G"], a["seed"])
    if name == "labels20":           # one class of three, a pair, fifteen singletons (anchors without a positive)
        z_i, z_j = recipe(10, a["D"], 3, a["seed"])
        labels = torch.tensor([7, 7, 7, 1, 1] + list(range(10, 25)), dtype=torch.int64)
        e = torch.cat([z_i, z_j])
        e[1] = F.normalize(e[0] + 0.5 * e[1], dim=0)
        e[2] = F.normalize(e[0] + 0.7 * e[2], dim=0)
        return e.contiguous(), labels
    if name == "hand8":
        # label pairs (0,1) (2,3) (4,5) (6,7). Anchor 0: pos = S01 = 0.1, its negatives are 0.9 (row 2: semi-hard, above pos + margin)
        # and -0.5 (not semi-hard): valid, hinge = 0.1 - 0.9 + 0.2 < 0. Every other anchor has a positive and no negative above
        # pos - margin (rows 2..7 are long: their positives are 3.65 and 9.5), so anchor 0 is the only valid one.
        e = torch.zeros(8, a["D"])
        e[0, 0] = 1.0
        e[1, 0], e[1, 1] = 0.1, 1.0
        e[2, 0], e[2, 1], e[2, 2] = 0.9, -0.2, 2.0
        e[3, 0], e[3, 1], e[3, 2] = -0.5, -0.5, 2.0
        for r, ax in ((4, 4), (5, 4), (6, 6), (7, 6)):
            e[r, 0], e[r, 1], e[r, ax] = -0.5, -0.5, 3.0
        e[5, 5] = 0.1
        e[7, 7] = 0.1
        return e, torch.tensor([0, 0, 1, 1, 2, 2, 3, 3], dtype=torch.int64)
    raise KeyError(name)


def input_digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.numpy()).tobytes())
    return h.hexdigest()


def pair_labels(B):
    return torch.cat([torch.arange(B), torch.arange(B)])


def mine(S, labels, margin=MARGIN):
    """the mining decisions on a similarity matrix of any precision: dict of valid, pidx, nidx (-1: none), pos, neg, gap"""
    M = S.shape[0]
    inf = float("inf")
    match = labels[:, None] == labels[None, :]
    mask_pos = match & ~torch.eye(M, dtype=torch.bool)
    pos_m = S.masked_fill(~mask_pos, -inf)
    pos, pidx = pos_m.max(dim=1)
    pidx = torch.where(mask_pos.any(1), pidx, torch.full_like(pidx, -1))
    thr = pos[:, None] - margin
    semi = (~match) & (S > thr)
    neg_m = S.masked_fill(~semi, inf)
    neg, nidx = neg_m.min(dim=1)
    valid = semi.any(1)
    nidx = torch.where(valid, nidx, torch.full_like(nidx, -1))
    # decision gap: distance of any negative from the threshold, of the two smallest semi-hard negatives, of the hinge from 0
    g1 = (S - thr).abs().masked_fill(match, inf).min(dim=1).values
    g1 = torch.where(torch.isinf(pos), torch.full_like(g1, inf), g1)
    two = torch.sort(neg_m, dim=1).values[:, :2] if M >= 2 else neg_m.new_full((M, 2), inf)
    g2 = torch.where(torch.isinf(two[:, 1]), torch.full_like(g1, inf), two[:, 1] - two[:, 0])
    hinge = pos - neg + margin
    g3 = torch.where(valid & ~torch.isinf(pos), hinge.abs(), torch.full_like(g1, inf))
    gap = torch.minimum(torch.minimum(g1, g2), g3)
    return dict(valid=valid, pidx=pidx, nidx=nidx, pos=pos, neg=neg, gap=gap, active=valid & (hinge > 0))


def classifier_loss64(z_i, z_j):
    z = torch.cat([z_i, z_j])
    M = z.shape[0]
    S = (z @ z.T).masked_fill(torch.eye(M, dtype=torch.bool), -float("inf"))
    tgt = (torch.arange(M) + M // 2) % M
    return (torch.logsumexp(S, dim=1) - S[torch.arange(M), tgt]).mean()


def triplet_loss64(E, labels, margin=MARGIN, decisions=None):
    """decisions: (valid, pidx, nidx) to evaluate the loss with (a kernel's choices at near ties); None: mined here in fp64"""
    S = E @ E.T
    d = mine(S.detach(), labels, margin)
    if decisions is not None:
        d = dict(d, valid=decisions[0].bool(), pidx=decisions[1].long(), nidx=decisions[2].long())
    rows = torch.nonzero(d["valid"]).flatten()
    if rows.numel() == 0:
        return E.sum() * 0.0, d
    has_pos = d["pidx"][rows] >= 0
    pos = torch.where(has_pos, S[rows, d["pidx"][rows].clamp(min=0)], S.new_full((rows.numel(),), -float("inf")))
    neg = S[rows, d["nidx"][rows]]
    return torch.relu(pos - neg + margin).mean(), d


def objective64(z_i, z_j, margin=MARGIN, beta=1.0, gamma=1.0, decisions=None):
    """fp64 evaluation of everything the tests compare: dict of cls, trip, loss, dcls, dtrip (gradient of trip through the
    normalisation), dz (of loss), n_valid and the mining decisions on the normalised rows"""
    zi = z_i.double().clone().requires_grad_(True)
    zj = z_j.double().clone().requires_grad_(True)
    B = zi.shape[0]
    cls = classifier_loss64(zi, zj)
    zn = F.normalize(torch.cat([zi, zj]), dim=1)
    trip, d = triplet_loss64(zn, pair_labels(B), margin, decisions)
    dcls = torch.cat(torch.autograd.grad(cls, (zi, zj), retain_graph=True))
    dtrip = torch.cat(torch.autograd.grad(trip, (zi, zj)))
    return dict(cls=cls.detach(), trip=trip.detach(), loss=(beta * cls + gamma * trip).detach(), dcls=dcls, dtrip=dtrip,
                dz=beta * dcls + gamma * dtrip, n_valid=int(d["valid"].sum()), mining=d)


def triplet64(E, labels, margin=MARGIN, decisions=None):
    e = E.double().clone().requires_grad_(True)
    trip, d = triplet_loss64(e, labels, margin, decisions)
    (de,) = torch.autograd.grad(trip, (e,))
    return dict(trip=trip.detach(), de=de, n_valid=int(d["valid"].sum()), mining=d)


# ---- compact storage of a gradient (M, D): whole when D <= 256, else four rows and eight fixed +-1 projections of every row
SAMPLE_ROWS = 4
N_PROJ = 8


def sample_rows(M):
    return np.unique(np.linspace(0, M - 1, SAMPLE_ROWS).round().astype(np.int64))


def proj_matrix(D):
    return torch.from_numpy(np.random.RandomState(1234).choice([-1.0, 1.0], size=(D, N_PROJ)))


def compact(t, whole):
    """t (M, D) float tensor -> dict of float64 arrays"""
    t = t.detach().double()
    if whole:
        return {"whole": t.numpy()}
    return {"rows": t[torch.from_numpy(sample_rows(t.shape[0]))].numpy(), "proj": (t @ proj_matrix(t.shape[1])).numpy()}


def compact_maxerr(t, ref):
    """max abs deviation of tensor t from a stored compact(): elementwise on what is stored; a projection over D elements of
    independent errors grows like sqrt(D), so it is scaled back by that"""
    t = t.detach().double().cpu()
    if "whole" in ref:
        return float((t - torch.from_numpy(ref["whole"])).abs().max())
    e_rows = (t[torch.from_numpy(sample_rows(t.shape[0]))] - torch.from_numpy(ref["rows"])).abs().max()
    e_proj = (t @ proj_matrix(t.shape[1]) - torch.from_numpy(ref["proj"])).abs().max() / np.sqrt(t.shape[1])
    return float(max(e_rows, e_proj))
