#!/usr/bin/env python3
"""SHA-256 of the raw output bytes of the classifier kernels (csrc/rerank.hip, csrc/clf_train.hip) on seeded inputs, one line per
case: a bitwise A/B of two builds of the kernel library. Run once per library, a fresh process each, and compare the listings.

    python tools/clf_digest.py > branch.txt;  NSID_LIB=/path/to/other/libnsid_hip.so python tools/clf_digest.py > other.txt

Cases (the smallest shapes that reach every tile count nT = 1 .. 4, the partial last tile, the half-full DH = 160 block and both
K-staging forms of the N <= 32 evaluation kernel), each at C in CLF_WIDTHS:
  clf_pair_scores, clf_pair_scores_dev           N in 1, 31, 32, 33, 64, 100, 128; two groups: 65 query segments against a list with
                                                 a repeated candidate, and 3 against 2
  clf_attn_fwd, clf_attn_bwd, clf_seg_reduce     N in 1, 31, 32; 5 pairs over 2 query and 3 candidate segments
  clf_attn_fwd_n, clf_attn_bwd_n, clf_seg_reduce_n   N in 1, 31, 32, 33, 64, 97, 128; the same pairs (N <= 32 reaches the multi-tile
                                                 kernels this way)
  clf_head_fwd, clf_head_bwd                     37 pairs"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralsampleid_amd import ops  # noqa: E402

DEV = "cuda"


def randn(seed, *shape, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def digest(*ts) -> str:
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def pair_cases():
    q_start, q_count = [0, 65], [65, 3]
    cand_idx, cand_off, cand_count = [2, 0, 2, 1, 1, 3], [0, 4], [4, 2]
    cidx = torch.tensor(cand_idx, dtype=torch.int32, device=DEV)
    tail = randn(7, 257, scale=0.5)
    for C in ops.CLF_WIDTHS:
        for N in (1, 31, 32, 33, 64, 100, 128):
            q = randn(1000 + C + N, 68 * N, C, scale=0.3)
            kp = randn(2000 + C + N, 4 * N, C + ops.CLF_PW, scale=0.3)
            out, _ = ops.clf_pair_scores(q, kp, N, tail, q_start, q_count, cand_idx, cand_off, cand_count)
            yield f"clf_pair_scores C={C} N={N}", digest(out)
            out, _ = ops.clf_pair_scores_dev(q, kp, N, tail, q_start, q_count, cand_count, cidx)
            yield f"clf_pair_scores_dev C={C} N={N}", digest(out)


def train_cases():
    Sq, Sc = 2, 3
    qi = torch.tensor([0, 1, 0, 1, 1], dtype=torch.int32, device=DEV)
    ci = torch.tensor([0, 1, 2, 2, 0], dtype=torch.int32, device=DEV)
    forms = (("", (1, 31, 32), ops.clf_attn_fwd, ops.clf_attn_bwd, ops.clf_seg_reduce),
             ("_n", (1, 31, 32, 33, 64, 97, 128), ops.clf_attn_fwd_n, ops.clf_attn_bwd_n, ops.clf_seg_reduce_n))
    for sfx, nodes, fwd, bwd, red in forms:
        for C in ops.CLF_WIDTHS:
            for N in nodes:
                q = randn(3000 + C + N, Sq * N, C, scale=0.5)
                kv = randn(4000 + C + N, Sc * N, 2 * C, scale=0.5)
                dob = randn(5000 + C + N, qi.numel(), C)
                obar, attn, abar = fwd(q, kv, N, qi, ci)
                yield f"clf_attn_fwd{sfx} C={C} N={N}", digest(obar, attn, abar)
                dq, dk = bwd(dob, attn, q, kv, N, qi, ci)
                yield f"clf_attn_bwd{sfx} C={C} N={N}", digest(dq, dk)
                dqs, dkvs = red(dq, dk, abar, dob, qi, ci, N, Sq, Sc)
                yield f"clf_seg_reduce{sfx} C={C} N={N}", digest(dqs, dkvs)


def head_cases():
    P = 37
    hid, w2, b2 = randn(11, P, ops.CLF_HID), randn(12, ops.CLF_HID, scale=0.2), randn(13, 1)
    keep = (torch.rand(P, ops.CLF_HID, generator=torch.Generator().manual_seed(14)) < 0.7).float().to(DEV) / 0.7
    s = ops.clf_head_fwd(hid, keep, w2, b2)
    yield "clf_head_fwd", digest(s)
    yield "clf_head_bwd", digest(*ops.clf_head_bwd(randn(15, P), s, hid, keep, w2))


def main():
    n = 0
    for cases in (pair_cases, train_cases, head_cases):
        for name, d in cases():
            print(f"{d}  {name}", flush=True)
            n += 1
    print(f"# {n} cases, library {getattr(ops.lib, '_name', '')}", file=sys.stderr)


if __name__ == "__main__":
    main()
