"""Writes tests/golden/baseline_loss_dp.npz from the REFERENCE's own loss functions (generation time only; the tests read the file):
the two pair cases of the sharded objective (nsid_baseline_objective_rows_fwd_bwd) past the row limit of the unsharded one.

    python tests/golden/make_baseline_loss_dp_golden.py /path/to/NeuralSampleID

Same evaluation as make_baseline_loss_golden.py (its ref_pair: triplet_loss, classifier_loss and the step objective of
baseline/train.py:66-77, once in fp32 and once in fp64), on inputs made with baseline_loss_oracle.recipe(**CASES[name]). Per case
<name>/... the keys of baseline_loss.npz: sha256, cls / trip / loss 32 and 64, valid, pidx, nidx, gap, floor_{cls,trip,loss,dz,dcls,
dtrip}, and the fp64 gradients of the two parts dcls64, dtrip64 in the sampled form of baseline_loss_oracle.compact.
NOT stored: dz32 and dz64. Four gradients of 4096 rows do not fit a committed file of 1 MiB even in the sampled form; dz32 only serves
floor_dz, which is stored, and dz64 = dcls64 + dtrip64 at beta = gamma = 1 (the compact form is linear), which is how the tests form
it. A case whose share of anchors with a decision gap below GAP_MIN reaches 2 % is refused: pick another seed."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import baseline_loss_oracle as O  # noqa: E402
from make_baseline_loss_golden import load_reference, put, ref_pair  # noqa: E402

# M = 2064: the first row count past the unsharded limit that is 16 past a multiple of 64; M = 4096: the limit of the sharded form
CASES = {
    "r1032x64": dict(B=1032, D=64, G=48, seed=1),
    "r2048x64": dict(B=2048, D=64, G=48, seed=0),
}
NEAR_TIE_SHARE_MAX = 0.02


def main(root):
    ref = load_reference(root)
    out = {}
    for name, args in CASES.items():
        a, b = O.recipe(**args)
        put(out, name, "sha256", O.input_digest(a, b))
        r32, r64 = ref_pair(ref, a, b, torch.float32), ref_pair(ref, a, b, torch.float64)
        for k in ("cls", "trip", "loss"):
            put(out, name, k + "32", r32[k].numpy())
            put(out, name, k + "64", r64[k].numpy())
            put(out, name, "floor_" + k, abs(float(r32[k]) - float(r64[k])))
        for k in ("dz", "dcls", "dtrip"):
            c64 = O.compact(r64[k], False)
            if k != "dz":
                for kk, v in c64.items():
                    out[f"{name}/{k}64.{kk}"] = v
            put(out, name, "floor_" + k, O.compact_maxerr(r32[k], c64))
        E32 = r32["zn"]
        d = O.mine(E32 @ E32.T, O.pair_labels(a.shape[0]), O.MARGIN)     # the reference's fp32 similarities
        d64 = O.mine(r64["zn"] @ r64["zn"].T, O.pair_labels(a.shape[0]), O.MARGIN)
        put(out, name, "valid", d["valid"].numpy())
        put(out, name, "pidx", d["pidx"].numpy().astype(np.int32))
        put(out, name, "nidx", d["nidx"].numpy().astype(np.int32))
        put(out, name, "gap", d["gap"].double().numpy())
        near = int((d["gap"] < O.GAP_MIN).sum())
        differ = int(((d["valid"] != d64["valid"]) | (d["pidx"] != d64["pidx"]) | (d["nidx"] != d64["nidx"])).sum())
        print(f"{name:10s} M={E32.shape[0]:4d} D={E32.shape[1]:5d} valid(fp32)={int(d['valid'].sum()):4d} valid(fp64)={int(d64['valid'].sum()):4d} "
              f"active={int(d['active'].sum()):4d} fp32-vs-fp64 decision differences={differ} near-ties={near} "
              + " ".join(f"{k[len(name) + 7:]}={float(v):.3g}" for k, v in out.items() if k.startswith(name + "/floor_")))
        assert near < NEAR_TIE_SHARE_MAX * E32.shape[0], f"{name}: {near} near-tie anchors of {E32.shape[0]}: pick another seed"
    path = os.path.join(HERE, "baseline_loss_dp.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1])
