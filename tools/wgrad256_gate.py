#!/usr/bin/env python3
"""Gate of the 256x256 weight-gradient class (csrc/wgrad256.hip): the wide problems of the deferred phase of ONE B = 256 contrastive
step (recorded from the step itself: every item the phase would issue on its main lane, i.e. the 128x128-class problems), timed
alone with the 128x128 class (wgrad256 = 0) and the 256x256 class at each rows-per-item setting. Operands are cold: every repetition
first streams a 1 GB buffer through the caches. Prints one JSON line per setting (median / min ms of the launches on the lane).

    python tools/wgrad256_gate.py [--reps 20] [--rows 4096,8192]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from neuralsampleid_amd import functional as F_  # noqa: E402
from neuralsampleid_amd import ops  # noqa: E402


def record_phase(batch):
    from neuralsampleid_amd.encoder.graph_encoder import GraphEncoder
    from neuralsampleid_amd.optim import FusedClipAdam
    from neuralsampleid_amd.simclr.ntxent import ntxent_loss
    from neuralsampleid_amd.simclr.simclr import SimCLR
    from synth import GRAFP_CFG, synth_clips, synth_state
    x_i, x_j = synth_clips(batch)
    model = SimCLR(GRAFP_CFG, GraphEncoder(GRAFP_CFG, in_channels=GRAFP_CFG["n_filters"], k=3, size="t"), overlap_views=True)
    model.load_state_dict(synth_state(model.state_dict()))
    model.cuda().train()
    opt = FusedClipAdam(model.parameters(), lr=GRAFP_CFG["lr"], max_norm=1.0)
    got = []
    orig = F_.DeferredWgrads._issue

    def issue(self, items):
        got.extend(items)
        orig(self, items)
    F_.DeferredWgrads._issue = issue
    try:
        opt.zero_grad()
        _, _, z_i, z_j = model(x_i.cuda(), x_j.cuda())
        ntxent_loss(z_i, z_j, GRAFP_CFG).backward()
    finally:
        F_.DeferredWgrads._issue = orig
    torch.cuda.synchronize()
    # the main lane of functional.DeferredWgrads._issue_two_lanes
    heavy = [it for it in got if it[0].dtype == torch.bfloat16 and (len(it) < 11 or it[10] is None) and it[3] % 128 == 0 and
             it[4] % 128 == 0 and it[5] % 128 == 0]
    # private operands (the step's tensors are reused by the allocator) and a private gradient per layer
    out, dws = [], {}
    for it in heavy:
        dw = dws.setdefault(it[2].data_ptr(), torch.zeros_like(it[2]))
        out.append((it[0].clone(), it[1].clone(), dw) + tuple(it[3:10]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rows", default="4096,8192")
    ap.add_argument("--only", default="", help="one setting (w3, w4_rows8192, ...) and one subset (all / only_256_shapes), e.g. for a PMC run")
    args = ap.parse_args()
    ops.set_gemm_precision("bf16")
    F_.set_activation_dtype("bf16")
    items = record_phase(args.batch)
    flops = sum(2.0 * it[3] * it[4] * it[5] * it[6] for it in items)
    w4 = [it for it in items if it[4] % 256 == 0 and it[5] % 256 == 0]
    print(json.dumps({"items": len(items), "gflop": flops / 1e9, "items_256": len(w4),
                      "gflop_256": sum(2.0 * it[3] * it[4] * it[5] * it[6] for it in w4) / 1e9,
                      "shapes": sorted({(it[3], it[4], it[5], it[6], it[7] is not None) for it in items})}), flush=True)
    flush = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    settings = [("w3", 0, 0)] + [(f"w4_rows{r}", 1, int(r)) for r in args.rows.split(",")]
    for subset_name, subset in (("all", items), ("only_256_shapes", w4)):
        for name, on, rows in settings:
            if args.only and args.only not in (name, f"{subset_name}:{name}", subset_name):
                continue
            ops.reset_tuning()
            ops.set_tuning("wgrad256", on)
            if rows:
                ops.set_tuning("wgg_rows256", rows)
            ts = []
            for rep in range(args.reps + 2):
                flush.add_(1.0)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ops.linear_bwd_weight_batch(subset)
                b.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    ts.append(a.elapsed_time(b))
            ts.sort()
            print(json.dumps({"subset": subset_name, "setting": name, "median_ms": ts[len(ts) // 2], "min_ms": ts[0],
                              "tflops_median": sum(2.0 * it[3] * it[4] * it[5] * it[6] for it in subset) / ts[len(ts) // 2] / 1e9}),
                  flush=True)
    ops.reset_tuning()


if __name__ == "__main__":
    main()
