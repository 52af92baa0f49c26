"""Mirror of downstream.py:30-78 CrossAttentionClassifier, scored on the MI355X (csrc/rerank.hip).

Same constructor, module tree and state_dict as the reference (`positional_embedding` buffer, `attn.in_proj_*`, `attn.out_proj.*`,
`fc.0.*`, `fc.3.*`), so a clf_*.pth written by downstream.py loads with strict=True. The forward is the reference's eval-mode forward
on a folded form: nothing between out_proj, the node mean and fc.0 is nonlinear, so with G = W1 Wo the tail is
g + sum_h G_h V_h^T a_h (a_h = the column mean of head h's attention), and the candidate side G_h V_h^T = X_j (G_h Wv_h)^T + G_h bv_h
is one linear per segment. The per-segment projections run on the project's fp32 GEMM (ops.linear_fwd), the per-pair work in
nsid_clf_pair_scores.

    clf = CrossAttentionClassifier(C, num_nodes=32).cuda().eval()      # C = the encoder's last width: 512, 640, 768 or 1024
    clf.load_state_dict(torch.load("clf.pth"))
    with torch.no_grad():
        s = clf.pair_scores(nm_query, nm_cand)        # (Sq, C, N), (Sc, C, N) -> (Sq, Sc)

Supported: in_dim 512, 640, 768 or 1024 (the encoder sizes 't', 's', 'm' and the default; head dim in_dim / 4), 4 heads, hidden_dim
128, N <= 128 (and N <= num_nodes with pos_embed), fp32 contiguous inputs whose channel count is the module's in_dim; anything else
raises before a launch. N <= 32 runs on the single-tile kernel (nsid_clf_pair_scores_c), 33 <= N <= 128 (the 256-mel configuration's
128-node matrices; num_nodes=128, or the reference's default 100 for N <= 100) on the multi-tile one (nsid_clf_pair_scores_n); the
dispatch is by N alone, in ops.clf_node_rows / ops.clf_pair_scores. This module's forward stays the eval-mode re-rank path and refuses training mode and grad. Training
(downstream.py's loop) runs through neuralsampleid_amd.downstream: clf_train_scores_n is the training-mode forward and backward on
csrc/clf_train.hip, and train() / train_step() drive it (N <= 128, the same dispatch by N); the trained state_dict loads here as it is."""
import math

import numpy as np
import torch
import torch.nn as nn

from . import ops


class CrossAttentionClassifier(nn.Module):
    def __init__(self, in_dim, num_heads=4, hidden_dim=128, num_nodes=100, pos_embed=True):
        super().__init__()
        self.pos_embed = pos_embed
        if self.pos_embed:
            self.register_buffer("positional_embedding", torch.randn(1, num_nodes, in_dim))
        self.attn = nn.MultiheadAttention(embed_dim=in_dim, num_heads=num_heads, batch_first=True)
        self.fc = nn.Sequential(nn.Linear(in_dim, hidden_dim), nn.ReLU(), nn.Dropout(p=0.3), nn.Linear(hidden_dim, 1), nn.Sigmoid())
        self._fold = None

    # ---------------------------------------------------------------------------------------------------- checks
    def _check_module(self):
        C, H = self.attn.embed_dim, self.attn.num_heads
        if C not in ops.CLF_WIDTHS or H != 4 or self.fc[0].out_features != 128:
            raise NotImplementedError(f"the re-rank kernel covers in_dim {', '.join(map(str, ops.CLF_WIDTHS))}, 4 heads and hidden_dim "
                                      f"128 (got in_dim {C}, {H} heads, hidden_dim {self.fc[0].out_features})")
        if self.attn.in_proj_weight is None or self.attn.in_proj_bias is None or self.attn.bias_k is not None:
            raise NotImplementedError("the re-rank kernel needs the packed in_proj weight and bias of nn.MultiheadAttention")

    def _check_nodes(self, x, name) -> int:
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"{name}: expected a torch tensor")
        if x.dtype != torch.float32:
            raise ValueError(f"{name}: only float32 node matrices are supported, got {x.dtype}")
        C = self.attn.embed_dim
        if x.dim() != 3 or x.shape[1] != C:
            raise ValueError(f"{name}: expected (S, {C}, N) node matrices for a classifier of in_dim {C}, got {tuple(x.shape)}")
        if not x.is_contiguous():
            raise ValueError(f"{name}: node matrices must be contiguous (S, C, N)")
        if not x.is_cuda:
            raise RuntimeError(f"{name}: the classifier runs on the MI355X (cuda) device; there is no CPU path")
        N = x.shape[2]
        if not 1 <= N <= ops.CLF_MAX_N_EVAL:
            raise ValueError(f"{name}: N = {N} nodes is outside [1, {ops.CLF_MAX_N_EVAL}]")
        if self.pos_embed and N > self.positional_embedding.shape[1]:
            raise ValueError(f"{name}: N = {N} exceeds the positional embedding's {self.positional_embedding.shape[1]} nodes")
        return N

    def _check_mode(self):
        self._check_module()
        if self.training or torch.is_grad_enabled():
            raise NotImplementedError("classifier training is not implemented here: call eval() and score under torch.no_grad()")

    # ---------------------------------------------------------------------------------------------------- folded weights
    def _state_key(self):
        ts = list(self.parameters()) + list(self.buffers())
        return tuple((t.data_ptr(), t._version) for t in ts) + (ops.WEIGHT_EPOCH,)

    def folded(self):
        """(wq, bq, wkp, bkp, tail, pos): Wq / sqrt(dh) and its bias, dh = C / 4; [Wk ; Wp] ((C + 512) x C) and [bk ; bp] with Wp_h = G_h Wv_h,
        bp_h = G_h bv_h, G = W1 Wo; tail = {g = W1 bo + b1, w2, b2}; pos (num_nodes, C) or None. Built once per parameter version
        (fp64 on the device, stored fp32)."""
        self._check_module()
        key = self._state_key()
        if self._fold is not None and self._fold[0] == key:
            return self._fold[1]
        with torch.no_grad():
            C, H = self.attn.embed_dim, self.attn.num_heads
            dh = C // H
            win, bin_ = self.attn.in_proj_weight.double(), self.attn.in_proj_bias.double()
            wq, wk, wv = win[:C], win[C:2 * C], win[2 * C:]
            bq, bk, bv = bin_[:C], bin_[C:2 * C], bin_[2 * C:]
            wo, bo = self.attn.out_proj.weight.double(), self.attn.out_proj.bias.double()
            w1, b1 = self.fc[0].weight.double(), self.fc[0].bias.double()
            w2, b2 = self.fc[3].weight.double().reshape(-1), self.fc[3].bias.double().reshape(-1)
            G = w1 @ wo
            g = w1 @ bo + b1
            wp = torch.cat([G[:, h * dh:(h + 1) * dh] @ wv[h * dh:(h + 1) * dh] for h in range(H)], 0)
            bp = torch.cat([G[:, h * dh:(h + 1) * dh] @ bv[h * dh:(h + 1) * dh] for h in range(H)], 0)
            s = 1.0 / math.sqrt(dh)
            f = lambda t: t.float().contiguous()
            pos = f(self.positional_embedding[0]) if self.pos_embed else None
            fold = (f(wq * s), f(bq * s), f(torch.cat([wk, wp], 0)), f(torch.cat([bk, bp], 0)), f(torch.cat([g, w2, b2])), pos)
        torch.cuda.current_stream().synchronize()
        self._fold = (key, fold)
        return fold

    # ---------------------------------------------------------------------------------------------------- prepare / score
    @staticmethod
    def _linear(rows, w, b):
        M, K = rows.shape
        if M == 0:
            return torch.empty((0, w.shape[0]), device=rows.device, dtype=torch.float32)
        prev = ops.get_gemm_precision()
        if prev != "fp32":
            ops.set_gemm_precision("fp32")
        try:
            out, _ = ops.linear_fwd(rows, w, b, M, w.shape[0], K)
        finally:
            if prev != "fp32":
                ops.set_gemm_precision(prev)
        return out

    def project_queries(self, nm: torch.Tensor) -> torch.Tensor:
        """(S, C, N) query node matrices -> (S N, C) rows of (x + pos) Wq^T / sqrt(dh) + bq / sqrt(dh)"""
        self._check_mode()
        N = self._check_nodes(nm, "project_queries")
        wq, bq, _, _, _, pos = self.folded()
        return self._linear(ops.clf_node_rows(nm, None if pos is None else pos[:N].contiguous()), wq, bq)

    def project_candidates(self, nm: torch.Tensor) -> torch.Tensor:
        """(S, C, N) candidate node matrices -> (S N, C + 512) rows [K | P]"""
        self._check_mode()
        N = self._check_nodes(nm, "project_candidates")
        _, _, wkp, bkp, _, pos = self.folded()
        return self._linear(ops.clf_node_rows(nm, None if pos is None else pos[:N].contiguous()), wkp, bkp)

    def score_blocks(self, q_proj, kp_proj, N: int, q_start, q_count, cand_idx, cand_off, cand_count):
        """scores of blocked pair lists on projected segments (ops.clf_pair_scores); returns (flat scores, per-group offsets)"""
        self._check_mode()
        _, _, _, _, tail, _ = self.folded()
        return ops.clf_pair_scores(q_proj, kp_proj, N, tail, q_start, q_count, cand_idx, cand_off, cand_count)

    def pair_scores(self, nm_query: torch.Tensor, nm_cand: torch.Tensor) -> torch.Tensor:
        """(Sq, C, N) x (Sc, C, N) -> (Sq, Sc): the score of every (query segment, candidate segment) pair"""
        self._check_mode()
        Nq, Nc = self._check_nodes(nm_query, "pair_scores"), self._check_nodes(nm_cand, "pair_scores")
        if Nq != Nc:
            raise ValueError(f"pair_scores: query and candidate node counts differ ({Nq} vs {Nc})")
        Sq, Sc = nm_query.shape[0], nm_cand.shape[0]
        q = self.project_queries(nm_query)
        kp = self.project_candidates(nm_cand)
        out, _ = self.score_blocks(q, kp, Nq, [0], [Sq], np.arange(Sc), [0], [Sc])
        return out.view(Sq, Sc)

    def forward(self, x_i, x_j):
        """(B, C, N) pairs -> (B, 1) scores (eval mode, no grad)"""
        self._check_mode()
        N = self._check_nodes(x_i, "forward x_i")
        if self._check_nodes(x_j, "forward x_j") != N or x_i.shape != x_j.shape:
            raise ValueError(f"forward: x_i and x_j must have the same shape, got {tuple(x_i.shape)}, {tuple(x_j.shape)}")
        B = x_i.shape[0]
        q = self.project_queries(x_i)
        kp = self.project_candidates(x_j)
        ar = np.arange(B)
        ones = np.ones(B, np.int64)
        out, _ = self.score_blocks(q, kp, N, ar, ones, ar, ar, ones)
        return out.view(B, 1)
