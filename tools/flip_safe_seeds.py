#!/usr/bin/env python3
"""Find, on the CPU, synthetic inputs on which no ReLU or max-relative decision of the training pass is near (tests/oracle64.py).

A gradient can be compared element by element between fp32 kernels and the fp64 oracle only while every decision falls the same way.
For each shape of tests/test_every_element_gpu.py this tries x = randn(B, N, C) from torch.Generator().manual_seed(1000 + seed),
seed = 0, 1, ..., runs the oracle's training forward in float32 and float64 on the same graph, and prints the seeds whose
decision margin / decision error reaches the asked ratio, and the best seed seen. The constants BLOCK_SEEDS / MRCONV_SEEDS of
tests/oracle64.py come from its output; the tests recompute the ratio of each committed seed and assert it.

    python tools/flip_safe_seeds.py                       # every shape, stop at the first seed with ratio >= 8
    python tools/flip_safe_seeds.py --ratio 10 --tries 20000 --only block:3,512,32,3,1
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import oracle64 as O  # noqa: E402

BLOCK_SHAPES = [(B, C, N, k, d) for (C, N, k, d) in ((512, 32, 3, 1), (256, 64, 18, 3), (128, 128, 5, 1), (64, 256, 4, 2)) for B in (1, 3)]
MRCONV_SHAPES = [(1, 256, 64, 3), (3, 256, 64, 18)]


def search(kind, shape, ratio, tries, start=0):
    if kind == "block":
        B, C, N, k, d = shape
        P = O.synth_P(O.block_shapes(C), "blk.")
        pair_of = lambda s: O.block_case(B, C, N, k, d, s, want_grad=False, want_eval=False, P=P)[-1]
    elif kind == "mrconv":
        B, N, C, k = shape
        P = O.synth_P(O.mrconv_shapes(C, 2 * C), "mr.")
        pair_of = lambda s: O.mrconv_case(B, N, C, k, s, want_grad=False, P=P)[-1]
    else:
        pair_of = lambda s: O.mragg_case(*shape, s, want_grad=False)[-1]
    best = (0.0, None, None, None)
    t0 = time.time()
    for seed in range(start, tries):
        pr = pair_of(seed)
        m, e = pr.margin(), pr.error()
        r = m / e if e > 0 else float("inf")
        if r > best[0]:
            best = (r, seed, m, e)
        if r >= ratio:
            break
    r, seed, m, e = best
    n = (seed + 1 if r >= ratio else tries) - start
    print(f"{kind} {shape}: seed {seed} margin {m:.3e} error {e:.3e} ratio {r:.2f}  ({n} seeds tried, {(time.time() - t0) / n:.3f} s per seed){'' if r >= ratio else '  ** BELOW ' + str(ratio)}",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ratio", type=float, default=O.MIN_RATIO)
    ap.add_argument("--tries", type=int, default=20000)
    ap.add_argument("--only", default=None, help="kind:comma-separated shape, e.g. block:3,512,32,3,1 or mragg:3,256,64,18")
    ap.add_argument("--start", type=int, default=0, help="first seed to try (to continue a search)")
    ap.add_argument("--threads", type=int, default=8)
    a = ap.parse_args()
    torch.set_num_threads(a.threads)
    if a.only:
        kind, shape = a.only.split(":")
        return search(kind, tuple(int(v) for v in shape.split(",")), a.ratio, a.tries, a.start)
    for shape in BLOCK_SHAPES:
        search("block", shape, a.ratio, a.tries, a.start)
    for shape in MRCONV_SHAPES:
        search("mrconv", shape, a.ratio, a.tries, a.start)
        search("mragg", shape, a.ratio, a.tries, a.start)


if __name__ == "__main__":
    main()
