"""Times the baseline's training objective (simclr.triplet.baseline_objective: csrc/baseline_loss.hip, forward plus backward) on one GPU
next to a torch-eager restatement of baseline/train.py:66-77 plus loss.backward(), in the same process on the same inputs.

    python tools/baseline_loss_bench.py [--shapes 512x2048,256x2048] [--reps 20] [--inner 10]
    python tools/baseline_loss_bench.py --rows 2048,0,256 [--rows 1024,0,1024] [--rows-d 2048]

--rows Bg,p0,n times the objective of one data-parallel rank instead (ops.baseline_objective_rows_fwd_bwd on caller-owned buffers: the
forward over the Bg gathered pairs, the backward for pairs [p0, p0 + n)), forward plus backward and forward alone, at --rows-d
features; where the unsharded op takes the shape (Bg <= 1024) its time on the same inputs stands next to it.

Inputs are clustered unit-norm pairs (centres, per-clip noise scales), so that a real share of the anchors is valid. Both paths are
warmed up, then timed alternately: each sample is a device-event window around --inner forward-plus-backward calls, the median over
--reps samples is reported per call. Launch counts come from one profiled call of each path (torch.profiler, a run of its own after
the timing); the fused count is also what the code enqueues: 6 launches forward plus backward, and 2 to scale by the upstream
gradient. One JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from neuralsampleid_amd.simclr.triplet import baseline_objective  # noqa: E402

MARGIN, BETA, GAMMA = 0.2, 1.0, 1.0


def inputs(B, D, G, seed=0):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(G, D, generator=g)
    sc, sv = 0.2 + 0.7 * torch.rand(B, 1, generator=g), 0.2 + 0.8 * torch.rand(B, 1, generator=g)
    base = c[torch.arange(B) % G] + sc * torch.randn(B, D, generator=g)
    views = [F.normalize(base + sv * torch.randn(B, D, generator=g), dim=1) for _ in range(2)]
    return [v.cuda().requires_grad_(True) for v in views]


def eager_objective(z_i, z_j):
    """the step objective in stock torch ops: pair cross-entropy on cat(z_i, z_j), semi-hard triplet loss on its normalisation"""
    B = z_i.shape[0]
    z = torch.cat([z_i, z_j], dim=0)
    M = z.shape[0]
    eye = torch.eye(M, dtype=torch.bool, device=z.device)
    logits = (z @ z.T).masked_fill(eye, float("-inf"))
    cls = F.cross_entropy(logits, (torch.arange(M, device=z.device) + B) % M)
    e = F.normalize(z, dim=1, p=2)
    labels = torch.cat([torch.arange(B), torch.arange(B)]).to(z.device)
    sim = e @ e.T
    same = labels[:, None] == labels[None, :]
    pos = sim.masked_fill(~(same & ~eye), float("-inf")).max(dim=1).values
    neg_all = sim.masked_fill(same, float("-inf"))
    semi = neg_all.masked_fill(~(neg_all > (pos[:, None] - MARGIN)), float("inf"))
    neg = semi.min(dim=1).values
    valid = ~torch.isinf(neg)
    hinge = F.relu(pos[valid] - neg[valid] + MARGIN)
    trip = hinge.mean() if hinge.numel() > 0 else torch.zeros((), device=z.device)
    return BETA * cls + GAMMA * trip, cls, trip


def step(fn, z_i, z_j):
    z_i.grad = z_j.grad = None
    out = fn(z_i, z_j)
    out[0].backward()
    return out


def window_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def short(name):
    """a kernel's bare name: no return type, namespaces, template or call arguments; long generated names cut"""
    name = name.replace("void ", "").replace("(anonymous namespace)::", "")
    return name.split("(")[0].split("<")[0].split("::")[-1][:40]


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [ev.name for ev in prof.events() if getattr(ev, "device_type", None) == torch.autograd.DeviceType.CUDA]
        kernels = [n for n in names if not n.lower().startswith(("memcpy", "memset"))]
        return {"kernels": len(kernels), "copies_and_memsets": len(names) - len(kernels), "distinct": sorted({short(n) for n in kernels})}
    except Exception as exc:                 # a profiler that does not start is reported, the timing stands
        return {"kernels": f"not counted ({type(exc).__name__})"}


def rows_bench(args):
    from neuralsampleid_amd import ops
    from neuralsampleid_amd._lib import lib
    recs = []
    for spec in args.rows:
        Bg, p0, n = (int(v) for v in spec.split(","))
        D = args.rows_d
        z_i, z_j = (t.detach() for t in inputs(Bg, D, max(2, Bg // 12)))
        ws = torch.empty(lib.nsid_baseline_loss_rows_ws_floats(2 * Bg, D), device="cuda")
        out, dz = torch.empty(4, device="cuda"), (torch.empty(n, D, device="cuda"), torch.empty(n, D, device="cuda"))
        fns = {"rows_fwd_bwd_ms": lambda: ops.baseline_objective_rows_fwd_bwd(z_i, z_j, p0, n, MARGIN, BETA, GAMMA, ws=ws, out=out, dz=dz),
               "rows_fwd_ms": lambda: ops.baseline_objective_rows_fwd_bwd(z_i, z_j, p0, n, MARGIN, BETA, GAMMA, want_grad=False, ws=ws,
                                                                          out=out)}
        if 2 * Bg <= ops.BL_MAX:
            full = (torch.empty(Bg, D, device="cuda"), torch.empty(Bg, D, device="cuda"))
            fns["unsharded_fwd_bwd_ms"] = lambda: ops.baseline_objective_fwd_bwd(z_i, z_j, MARGIN, BETA, GAMMA, ws=ws, out=out, dz=full)
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():
                ms[k].append(window_ms(fn, args.inner))
        rec = {"Bg": Bg, "rows": 2 * Bg, "D": D, "p0": p0, "npairs": n, "workspace_mb": round(ws.numel() * 4 / 2 ** 20, 1)}
        for k, v in ms.items():
            rec[k] = round(float(np.median(v)), 4)
            rec[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
        fns["rows_fwd_bwd_ms"]()
        rec["out"] = [float(v) for v in out.cpu()]
        recs.append(rec)
    print(json.dumps({"bench": "baseline_objective_rows fwd+bwd", "reps": args.reps, "inner": args.inner, "shapes": recs}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x2048,256x2048")
    ap.add_argument("--rows", action="append", default=[], metavar="Bg,p0,n",
                    help="time the rows form (one data-parallel rank's objective) at this cut instead; may be repeated")
    ap.add_argument("--rows-d", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "baseline_loss_bench needs an MI355X"
    if args.rows:
        return rows_bench(args)
    fused_fn = lambda a, b: baseline_objective(a, b, MARGIN, BETA, GAMMA)      # noqa: E731
    rows = []
    for shape in args.shapes.split(","):
        B, D = (int(v) for v in shape.split("x"))
        z_i, z_j = inputs(B, D, max(2, B // 12))
        f_out = step(fused_fn, z_i, z_j)
        f_grad = torch.cat([z_i.grad, z_j.grad]).clone()
        e_out = step(eager_objective, z_i, z_j)
        e_grad = torch.cat([z_i.grad, z_j.grad]).clone()
        for _ in range(5):
            step(fused_fn, z_i, z_j)
            step(eager_objective, z_i, z_j)
        torch.cuda.synchronize()
        fused, eager = [], []
        for _ in range(args.reps):
            fused.append(window_ms(lambda: step(fused_fn, z_i, z_j), args.inner))
            eager.append(window_ms(lambda: step(eager_objective, z_i, z_j), args.inner))
        n_fused, n_eager = launches(lambda: step(fused_fn, z_i, z_j)), launches(lambda: step(eager_objective, z_i, z_j))
        med = lambda v: float(np.median(v))                                      # noqa: E731
        rows.append({"B": B, "D": D, "fused_ms": round(med(fused), 4), "eager_ms": round(med(eager), 4),
                     "fused_ms_min_max": [round(min(fused), 4), round(max(fused), 4)],
                     "eager_ms_min_max": [round(min(eager), 4), round(max(eager), 4)],
                     "eager_over_fused": round(med(eager) / med(fused), 2), "fused_launches": n_fused, "eager_launches": n_eager,
                     "loss_fused": [float(v.detach()) for v in f_out], "loss_eager": [float(v.detach()) for v in e_out],
                     "max_abs_grad_diff": float((f_grad - e_grad).abs().max()), "max_abs_grad": float(e_grad.abs().max())})
    print(json.dumps({"bench": "baseline_objective fwd+bwd", "reps": args.reps, "inner": args.inner, "shapes": rows}), flush=True)


if __name__ == "__main__":
    main()
