"""Mirror of downstream.py:82-140 (mine_hard_negatives, train): the stage-2 CrossAttentionClassifier trained on the node matrices of
the frozen encoder, on the MI355X (csrc/clf_train.hip).

    model = SimCLR(cfg, encoder=GraphEncoder(cfg, in_channels=cfg["n_filters"], k=5)).cuda()     # trained encoder weights loaded
    clf = CrossAttentionClassifier(in_dim=512, num_nodes=32).cuda()
    opt = torch.optim.Adam(clf.parameters(), lr=cfg["clf_lr"])
    loss = train(cfg, loader, model, clf, opt, torch.amp.GradScaler("cuda"), augment=gpu_augment)
    torch.save(clf.state_dict(), "checkpoint/clf_run_0.pth")                                     # loads into the re-rank path

Per batch, as the reference: the frozen encoder's pre-projection node matrices and normalised projections of both views (one eval
pass per view: encode_pairs), ranks 1..k of z_i z_all^T as hard negatives (mine_hard_negatives), B positive pairs (x_i[p], x_j[p])
and kB negative pairs (x_i[p mod B], x_all[hn.view(-1)[p]]) (pair_lists), the classifier's scores in training mode
(clf_train_scores_n), BCE(pos) + BCE(neg), backward, and the optimiser / GradScaler step. clf_train_scores_n takes up to 128 nodes
per segment; clf_train_scores is its N <= 32 form. The classifier's forward and backward run
as one autograd op over segments and pair lists: Q is projected once per query segment and [K | V] once per candidate segment, and
the per-pair attention, the head and their backward are HIP kernels; the projections and the tail's linears are the project's fp32
GEMMs. Training never goes through classifier(x_i, x_j), which stays the eval-mode re-rank forward (classifier.py)."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .classifier import CrossAttentionClassifier

__all__ = ["encode_pairs", "mine_hard_negatives", "pair_lists", "draw_keep", "clf_train_scores", "clf_train_scores_n", "train_step",
           "train"]


# ------------------------------------------------------------------------------------------------ features
def encode_pairs(model, x_i, x_j):
    """downstream.py:108-117 on the eval path: (nodes_i, nodes_j, z_i, z_j), the pre-projection node matrices (B, 512, N) and the
    normalised projections (B, d) of both views. The reference runs the encoder twice per view; in eval mode both passes give the same
    result, so each view runs once (model.encoder.forward_rows(..., return_nodes=True) returns the nodes and the embedding)."""
    from . import functional
    model.eval()
    if functional.ACT_DTYPE == torch.bfloat16:
        ops.register_weight_shadows(model)
    pe = model.peak_extractor
    out = []
    with torch.no_grad():
        for x in (x_i, x_j):
            x = x.contiguous()
            B, H, W = x.shape
            N = (H // pe.patch_bins) * (W // pe.patch_frames)
            rows, n_last, emb = model.encoder.forward_rows(pe.forward_rows(x), B, N, return_nodes=True)
            out.append((functional.from_rows(rows, B, n_last).float().contiguous(), model._project(emb)))
    (nodes_i, z_i), (nodes_j, z_j) = out
    return nodes_i, nodes_j, z_i, z_j


# ------------------------------------------------------------------------------------------------ mining and pairs
def mine_hard_negatives(z_i, z_j, negatives, num_negatives=3):
    """downstream.py:82-95: (B, num_negatives) int64 indices into `negatives`, ranks 1..k of z_i negatives^T in descending order
    (rank 0, usually the row itself, is skipped; rank 1 is often the row's own positive view). Ties go to the smaller index (argsort
    leaves them undefined). z_j is unused, as in the reference."""
    for t, name in ((z_i, "z_i"), (negatives, "negatives")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f"mine_hard_negatives: {name} must be a float32 tensor on the MI355X (cuda) device")
    if z_i.dim() != 2 or negatives.dim() != 2 or z_i.shape[1] != negatives.shape[1]:
        raise ValueError(f"mine_hard_negatives: expected (B, d) and (M, d), got {tuple(z_i.shape)}, {tuple(negatives.shape)}")
    k, M = int(num_negatives), negatives.shape[0]
    if k < 1 or M - 1 < k:
        raise ValueError(f"mine_hard_negatives: ranks 1..{k} need {k + 1} candidates, the pool has {M} (2B - 1 < k)")
    return ops.clf_mine_hard_negatives(z_i.contiguous(), negatives.contiguous(), k)


def pair_lists(hn, B: int):
    """downstream.py:123-126 as index lists into (query segments x_i, candidate segments x_all = cat(x_i, x_j)), pair p = score p of
    cat(logits_pos, logits_neg): positives (p, B + p) for p < B; negative p of the kB is x_i.repeat(k, 1, 1)[p] = x_i[p mod B] against
    x_all[hn.view(-1)[p]], so its query is NOT the anchor its candidate was mined for. Works on any device; returns int64 tensors."""
    hn = torch.as_tensor(hn)
    if hn.dim() != 2 or hn.shape[0] != B:
        raise ValueError(f"pair_lists: expected (B, k) = ({B}, k) mined indices, got {tuple(hn.shape)}")
    k, dev = hn.shape[1], hn.device
    ar = torch.arange(B, device=dev, dtype=torch.int64)
    q_idx = torch.cat([ar, ar.repeat(k)])
    c_idx = torch.cat([ar + B, hn.reshape(-1).to(torch.int64)])
    return q_idx, c_idx


def draw_keep(P: int, p: float, device) -> torch.Tensor:
    """the dropout keep mask of P pairs, (P, 128): bernoulli(1 - p) / (1 - p) from torch's generator, as nn.Dropout's noise"""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"draw_keep: dropout probability {p} is outside [0, 1)")
    keep = torch.empty((P, ops.CLF_HID), device=device, dtype=torch.float32)
    if p == 0.0:
        return keep.fill_(1.0)
    return keep.bernoulli_(1.0 - p).div_(1.0 - p)


# ------------------------------------------------------------------------------------------------ the classifier op
class _Fp32Gemm:
    def __enter__(self):
        self.prev = ops.get_gemm_precision()
        if self.prev != "fp32":
            ops.set_gemm_precision("fp32")

    def __exit__(self, *exc):
        if self.prev != "fp32":
            ops.set_gemm_precision(self.prev)


def _linear(x, w, b):
    return ops.linear_fwd(x, w, b, x.shape[0], w.shape[0], x.shape[1])[0]


def _wgrad(dout, x, Nout):
    """(dW (Nout, K), db (Nout,)) of out = x W^T + b on the fp32 weight-gradient GEMM and a column reduce"""
    dw = ops.fill_zero(torch.empty((Nout, x.shape[1]), device=x.device, dtype=torch.float32))
    db = ops.fill_zero(torch.empty((Nout,), device=x.device, dtype=torch.float32))
    ops.linear_bwd_weight(dout, x, dw, dout.shape[0], Nout, x.shape[1])
    ops.colsum_acc(dout, db)
    return dw, db


class _TrainScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nodes_q, nodes_c, qi, ci, keep, pos, w_in, b_in, w_o, b_o, w1, b1, w2, b2):
        C = w_o.shape[0]                    # the classifier's in_dim (checked by clf_train_scores)
        N = nodes_q.shape[2]
        wide = N > ops.CLF_MAX_N            # 33 .. 128 nodes: the multi-tile entries (clf_node_rows dispatches on N itself)
        attn_fwd = ops.clf_attn_fwd_n if wide else ops.clf_attn_fwd
        with _Fp32Gemm():
            xq = ops.clf_node_rows(nodes_q, pos)
            xc = ops.clf_node_rows(nodes_c, pos)
            q = _linear(xq, w_in[:C], b_in[:C])
            kv = _linear(xc, w_in[C:], b_in[C:])
            obar, attn, abar = attn_fwd(q, kv, N, qi, ci)
            m = _linear(obar, w_o, b_o)
            hid = _linear(m, w1, b1)
            s = ops.clf_head_fwd(hid, keep, w2.reshape(-1), b2)
        ctx.save_for_backward(xq, xc, q, kv, obar, attn, abar, m, hid, s, keep, qi, ci, w_o, w1, w2)
        ctx.dims = (N, nodes_q.shape[0], nodes_c.shape[0])
        return s.view(-1, 1)

    @staticmethod
    def backward(ctx, ds):
        xq, xc, q, kv, obar, attn, abar, m, hid, s, keep, qi, ci, w_o, w1, w2 = ctx.saved_tensors
        N, Sq, Sc = ctx.dims
        C = w_o.shape[0]
        P = s.shape[0]
        wide = N > ops.CLF_MAX_N
        attn_bwd, seg_reduce = (ops.clf_attn_bwd_n, ops.clf_seg_reduce_n) if wide else (ops.clf_attn_bwd, ops.clf_seg_reduce)
        ds = ds.reshape(-1).float().contiguous()
        with _Fp32Gemm():
            dh, _, dw2, db2 = ops.clf_head_bwd(ds, s, hid, keep, w2.reshape(-1))
            dw1, db1 = _wgrad(dh, m, ops.CLF_HID)
            dm = ops.linear_bwd_data(dh, w1, P, ops.CLF_HID, C)
            dwo, dbo = _wgrad(dm, obar, C)
            dobar = ops.linear_bwd_data(dm, w_o, P, C, C)
            dq, dk = attn_bwd(dobar, attn, q, kv, N, qi, ci)
            dq_seg, dkv_seg = seg_reduce(dq, dk, abar, dobar, qi, ci, N, Sq, Sc)
            dwq, dbq = _wgrad(dq_seg, xq, C)
            dwkv, dbkv = _wgrad(dkv_seg, xc, 2 * C)
        return (None, None, None, None, None, None, torch.cat([dwq, dwkv], 0), torch.cat([dbq, dbkv], 0), dwo, dbo, dw1, db1,
                dw2.view(1, -1), db2)


def _host_index(a, name, fn="clf_train_scores"):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{fn}: {name} must hold integers, got {a.dtype}")
    return a.astype(np.int64).reshape(-1)


def clf_train_scores(classifier: CrossAttentionClassifier, nodes_q, nodes_c, q_idx, c_idx, keep) -> torch.Tensor:
    """(P, 1) training-mode scores of the pairs (nodes_q[q_idx[p]], nodes_c[c_idx[p]]), differentiable in the classifier's eight
    parameters (attn.in_proj_*, attn.out_proj.*, fc.0.*, fc.3.*). nodes_q (Sq, C, N), nodes_c (Sc, C, N), C = the classifier's in_dim
    (512, 640, 768 or 1024): fp32 contiguous device node matrices that do not require grad (the encoder is frozen). q_idx, c_idx: integer sequences of length P (host or device; they
    are checked on the host). keep (P, 128): the dropout keep mask scaled by 1 / (1 - p) (draw_keep); all ones = no dropout. The
    classifier's own forward (eval-mode re-rank) is not used. N <= 32 (one attention tile per head); clf_train_scores_n is the
    entry for larger graphs."""
    return _train_scores("clf_train_scores", ops.CLF_MAX_N, classifier, nodes_q, nodes_c, q_idx, c_idx, keep)


def clf_train_scores_n(classifier: CrossAttentionClassifier, nodes_q, nodes_c, q_idx, c_idx, keep) -> torch.Tensor:
    """clf_train_scores for 1 <= N <= ops.CLF_MAX_N_EVAL (128) nodes, same contract: N <= 32 runs the one-tile kernels (the same
    launches and bits as clf_train_scores), 33 .. 128 the multi-tile ones (nsid_clf_attn_fwd_n, _bwd_n, nsid_clf_seg_reduce_n), as
    classifier.pair_scores dispatches in evaluation. The saved attention is 16 (32 ceil(N / 32))^2 bytes per pair (256 KB at
    N = 128) and the per-pair dQ, dK 8 N C bytes, held until the backward has run."""
    return _train_scores("clf_train_scores_n", ops.CLF_MAX_N_EVAL, classifier, nodes_q, nodes_c, q_idx, c_idx, keep)


def _train_scores(fn, max_n, classifier, nodes_q, nodes_c, q_idx, c_idx, keep):
    """the checks of clf_train_scores / clf_train_scores_n (fn, for the messages; max_n nodes at most) and the autograd op"""
    classifier._check_module()
    if classifier.attn.dropout != 0.0:
        raise NotImplementedError(f"{fn}: attention dropout is not supported (the reference's is 0)")
    N = classifier._check_nodes(nodes_q, f"{fn} nodes_q")
    if N > max_n:
        raise ValueError(f"{fn}: N = {N} nodes: eval-mode scoring covers N <= {ops.CLF_MAX_N_EVAL}, training covers "
                         + (f"N <= {ops.CLF_MAX_N} only here; clf_train_scores_n is the entry for graphs of up to {ops.CLF_MAX_N_EVAL}"
                            if max_n < ops.CLF_MAX_N_EVAL else f"N <= {max_n} only"))
    if classifier._check_nodes(nodes_c, f"{fn} nodes_c") != N:
        raise ValueError(f"{fn}: query and candidate node counts differ ({N} vs {nodes_c.shape[2]})")
    if nodes_q.requires_grad or nodes_c.requires_grad:
        raise ValueError(f"{fn}: node matrices must not require grad (the encoder is frozen; inputs get no gradient)")
    qi, ci = _host_index(q_idx, "q_idx", fn), _host_index(c_idx, "c_idx", fn)
    P = qi.size
    if ci.size != P or P == 0:
        raise ValueError(f"{fn}: q_idx and c_idx must have the same nonzero length, got {qi.size}, {ci.size}")
    Sq, Sc = nodes_q.shape[0], nodes_c.shape[0]
    if qi.min() < 0 or qi.max() >= Sq or ci.min() < 0 or ci.max() >= Sc:
        raise ValueError(f"{fn}: indices must lie in [0, {Sq}) (queries) and [0, {Sc}) (candidates)")
    if P > (1 << 28) or max(Sq, Sc) * N >= (1 << 31):
        raise ValueError(f"{fn}: too many pairs or segments for one call")
    if not isinstance(keep, torch.Tensor) or keep.dtype != torch.float32 or not keep.is_cuda or not keep.is_contiguous():
        raise ValueError(f"{fn}: keep must be a contiguous float32 device tensor")
    if tuple(keep.shape) != (P, ops.CLF_HID):
        raise ValueError(f"{fn}: keep must be ({P}, {ops.CLF_HID}), got {tuple(keep.shape)}")
    dev = nodes_q.device
    qt = torch.from_numpy(qi.astype(np.int32)).to(dev)
    ct = torch.from_numpy(ci.astype(np.int32)).to(dev)
    pos = classifier.positional_embedding[0, :N].detach().float().contiguous() if classifier.pos_embed else None
    a, f = classifier.attn, classifier.fc
    return _TrainScores.apply(nodes_q, nodes_c, qt, ct, keep, pos, a.in_proj_weight, a.in_proj_bias, a.out_proj.weight,
                              a.out_proj.bias, f[0].weight, f[0].bias, f[3].weight, f[3].bias)


# ------------------------------------------------------------------------------------------------ the loop
def train_step(classifier, optimizer, scaler, nodes_i, nodes_j, z_i, z_j, num_negatives=3, keep=None):
    """one step of downstream.py:104-134 from features: zero_grad, mining, pairs, scores, BCE(pos) + BCE(neg), backward and the
    optimiser (GradScaler) step; scaler=None: a plain backward and optimizer.step(). keep: (P, 128) mask, or None to draw one with
    torch's generator (classifier.fc[2].p). Returns a namespace with loss (0-dim tensor), hn, q_idx, c_idx, scores and keep."""
    classifier.train()
    criterion = nn.BCELoss()
    B = nodes_i.shape[0]
    optimizer.zero_grad()
    z_all = torch.cat((z_i, z_j), dim=0)
    hn = mine_hard_negatives(z_i, z_j, z_all, num_negatives=num_negatives)
    q_idx, c_idx = pair_lists(hn.cpu(), B)
    P = q_idx.numel()
    if keep is None:
        keep = draw_keep(P, classifier.fc[2].p, nodes_i.device)
    nodes_all = torch.cat((nodes_i, nodes_j), dim=0)
    scores = clf_train_scores_n(classifier, nodes_i, nodes_all, q_idx, c_idx, keep)
    logits_pos, logits_neg = scores[:B], scores[B:]
    pos_labels = torch.ones(logits_pos.shape[0], 1, device=scores.device)
    neg_labels = torch.zeros(logits_neg.shape[0], 1, device=scores.device)
    loss = criterion(logits_pos, pos_labels) + criterion(logits_neg, neg_labels)
    if scaler is not None:
        scaler.scale(loss).backward()
        scaler.step(optimizer)
        scaler.update()
    else:
        loss.backward()
        optimizer.step()
    return SimpleNamespace(loss=loss.detach(), hn=hn, q_idx=q_idx, c_idx=c_idx, scores=scores.detach(), keep=keep)


def train(cfg, train_loader, model, classifier, optimizer, scaler, augment=None, encode=encode_pairs, num_negatives=3,
          draw_mask=draw_keep, on_step=None):
    """downstream.py:97-140: one epoch; returns the mean loss. augment(x_i, x_j) is applied when given (None: the loader yields
    log-mel batches). Extensions, with defaults that reproduce the reference: encode(model, x_i, x_j) -> (nodes_i, nodes_j, z_i, z_j)
    (tests substitute recorded features), num_negatives, draw_mask(P, p, device) (tests substitute recorded masks), on_step(idx,
    step namespace)."""
    if model is not None:
        model.eval()  # Keep the encoder frozen
    classifier.train()
    dev = classifier.attn.in_proj_weight.device
    loss_epoch = 0.0
    for idx, (x_i, x_j) in enumerate(train_loader):
        x_i, x_j = x_i.to(dev), x_j.to(dev)
        with torch.no_grad():
            if augment is not None:
                x_i, x_j = augment(x_i, x_j)
            nodes_i, nodes_j, z_i, z_j = encode(model, x_i, x_j)
        P = (1 + int(num_negatives)) * nodes_i.shape[0]
        keep = draw_mask(P, classifier.fc[2].p, dev)
        st = train_step(classifier, optimizer, scaler, nodes_i, nodes_j, z_i, z_j, num_negatives=num_negatives, keep=keep)
        if on_step is not None:
            on_step(idx, st)
        loss = st.loss.item()
        if idx % 20 == 0:
            print(f"Step [{idx}/{len(train_loader)}]\t Loss: {loss}")
        loss_epoch += loss
    return loss_epoch / len(train_loader)
