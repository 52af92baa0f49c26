"""Times the classifier re-rank (csrc/rerank.hip) at the evaluations' block shapes, the projection GEMMs, a torch-eager fp32
comparison and the whole eval_map_clf on a synthetic sample100-sized emb_dir.

    python tools/rerank_bench.py [--reps 5] [--quick] [--in-dim 512|640|768|1024] [--nodes N]

Pair kernel: ms (median of --reps after a warm-up), pairs/s and TFLOP/s on 1.2 MFLOP per pair at in_dim 512 (2 N^2 C more per
channel of a wider classifier) for --nodes <= 32 (the default 32), and on ops.clf_pair_scores' model in N above that (the multi-tile
kernel, up to 128 nodes: 2 N^2 C + 48 N^2 + 1024 N + 512, 17.7 MFLOP at N = 128, C = 512), with its fraction of the fp32 matrix peak (155 TF, MI355X_MICROARCH). The eager comparison scores the same pairs with a batched fp32 nn.MultiheadAttention written here
(the reference's forward: one classifier call per candidate, batched over query segments, as eval_map.py does)."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralsampleid_amd import fpdb  # noqa: E402
from neuralsampleid_amd.classifier import CrossAttentionClassifier  # noqa: E402
from neuralsampleid_amd.rerank import eval_map_clf  # noqa: E402

PEAK_TF = 155.0


def flop_per_pair(C, N=32):
    if N <= 32:
        return 1.2e6 + 2.0 * 32 * 32 * (C - 512)
    return 2.0 * N * N * C + 12.0 * 4 * N * N + 2.0 * N * 512 + 512.0


def _median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def _clf(C, N=32):
    torch.manual_seed(0)
    clf = CrossAttentionClassifier(in_dim=C, num_nodes=N).cuda().eval()
    return clf


class EagerClf(nn.Module):
    """the reference's forward in torch-eager fp32 (downstream.py:59-78)"""

    def __init__(self, clf):
        super().__init__()
        self.attn, self.fc, self.pos = clf.attn, clf.fc, clf.positional_embedding

    def forward(self, x_i, x_j):
        x_i, x_j = x_i.permute(0, 2, 1), x_j.permute(0, 2, 1)
        pos = self.pos[:, :x_i.shape[1], :]
        a, _ = self.attn(x_i + pos, x_j + pos, x_j + pos)
        return self.fc(a.mean(dim=1))


def time_block(C, name, sq, sc, groups, reps, eager_groups=1, N=32):
    clf = _clf(C, N)
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn(groups * sq, C, N, device="cuda", generator=g)
    c = torch.randn(sc * 4, C, N, device="cuda", generator=g)
    with torch.no_grad():
        qp, kp = clf.project_queries(q), clf.project_candidates(c)
        rng = np.random.default_rng(0)
        lists = [rng.integers(0, c.shape[0], size=sc) for _ in range(groups)]
        args = (qp, kp, N, np.arange(groups) * sq, [sq] * groups, np.concatenate(lists), np.arange(groups) * sc, [sc] * groups)
        t = _median_ms(lambda: clf.score_blocks(*args), reps)
        tq = _median_ms(lambda: clf.project_queries(q), reps)
        tc = _median_ms(lambda: clf.project_candidates(c), reps)
        pairs = groups * sq * sc
        tf = flop_per_pair(C, N) * pairs / t / 1e9
        print(f"{name}: N {N}: {groups} x ({sq} x {sc}) pairs: kernel {t:9.3f} ms  {pairs / t / 1e3:8.2f} Mpairs/s  {tf:6.1f} TF/s "
              f"({tf / PEAK_TF:5.3f} of 155)", flush=True)
        print(f"{name}: projections: queries {groups * sq} segs {tq:7.3f} ms, candidates {c.shape[0]} segs {tc:7.3f} ms", flush=True)
        # eager comparison: one batched classifier call per candidate (eval_map.py:146-153), over eager_groups groups, scaled
        eager = EagerClf(clf)
        qe = q[:sq]

        def run_eager():
            for gi in range(eager_groups):
                for j in lists[gi].tolist():
                    eager(qe, c[j:j + 1].expand(sq, -1, -1))
        te = _median_ms(run_eager, max(1, reps // 2)) * groups / eager_groups
        print(f"{name}: torch-eager fp32 (batched nn.MultiheadAttention per candidate): {te:10.1f} ms (scaled from {eager_groups} "
              f"group(s)) -> kernel speed-up {te / t:7.1f}x", flush=True)


def time_eval_map(C, n_songs, segs, n_tests, q_segs, n_dummy, k_probe=3, N=32):
    rng = np.random.default_rng(0)
    d = 128

    def unit(n):
        x = rng.standard_normal((n, d)).astype(np.float32)
        return x / np.linalg.norm(x, axis=1, keepdims=True)

    clf = _clf(C, N)
    with tempfile.TemporaryDirectory() as tmp:
        ref = unit(n_songs * segs)
        names = [f"s{i}" for i in range(n_songs)]
        fpdb.write_fp_db(tmp, "ref_db", ref, [n for n in names for _ in range(segs)])
        fpdb.write_fp_db(tmp, "dummy_db", unit(n_dummy), ["dummy"] * n_dummy)
        fpdb.write_node_matrices(os.path.join(tmp, "ref_nmatrix"),
                                 {n: rng.standard_normal((segs, C, N), dtype=np.float32) for n in names})
        qrows = unit(n_tests * q_segs)
        fpdb.write_fp_db(tmp, "query_full_db", qrows, [f"q{i // q_segs}" for i in range(n_tests * q_segs)])
        np.save(os.path.join(tmp, "query_full_nmatrix.npy"),
                {f"q{i}": rng.standard_normal((q_segs, C, N), dtype=np.float32) for i in range(n_tests)})
        gt = {n: [f"q{i}"] for i, n in enumerate(names)}
        with torch.no_grad():
            eval_map_clf(tmp, clf, gt, k_probe=k_probe, save=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m, _ = eval_map_clf(tmp, clf, gt, k_probe=k_probe, save=False)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
    print(f"eval_map_clf: {n_tests} tests x {q_segs} query segments, {n_songs} x {segs} ref + {n_dummy} dummy rows, k_probe "
          f"{k_probe}: {t * 1e3:.1f} ms (MAP {float(m):.3f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="8 MAP-like groups instead of 64, a small evaluation")
    ap.add_argument("--in-dim", type=int, default=512, choices=(512, 640, 768, 1024), help="the classifier's width")
    ap.add_argument("--nodes", type=int, default=32, help="nodes per segment, 1 .. 128 (above 32: the multi-tile kernel)")
    a = ap.parse_args()
    C = a.in_dim           # the classifier's width: the encoder sizes 't', 's', 'm' and the default end in 512 .. 1024
    N = a.nodes
    if not 1 <= N <= 128:
        ap.error("--nodes must lie in [1, 128]")
    print(f"in_dim {C}, nodes {N}", flush=True)
    time_block(C, "map block", 350, 1024, 8 if a.quick else 64, a.reps, N=N)
    time_block(C, "hit-rate block", 19, 95, 64, a.reps, eager_groups=8, N=N)
    # node-matrix files grow with N: above 32 nodes the synthetic emb_dir has fewer, shorter songs
    if a.quick:
        time_eval_map(C, *((20, 350, 10, 350) if N <= 32 else (10, 100, 10, 100)), 20_000, N=N)
    else:
        time_eval_map(C, *((75, 350, 100, 350) if N <= 32 else (75, 100, 100, 100)), 100_000, N=N)


if __name__ == "__main__":
    main()
