#!/usr/bin/env python3
"""Golden vectors of the reference's ResidualIBN block (encoder/resnet_ibn.py) in TRAINING mode, fp64, CPU: forward, autograd backward
and the running-statistics update of one call.

Run from the repo root, where the reference checkout is available:

    python tests/golden/make_resnet_train_golden.py

Two blocks, ResidualIBN(64, 128, 1) and ResidualIBN(128, 256, 2), in .train() at B = 3 on 6 x 7 maps. Weights by name
(synth.synth_state with the fixture's tag as prefix), input synth_randn(tag, 3, Cin, 6, 7), upstream gradient
synth_randn(tag + "_dout", 3, Cout, Ho, Wo). Writes one resnet_train_<tag>.npz per block with, in the compact form of tests/compare.py
(fp64 samples, at most 1024 per tensor):
  out, dx                      the block's output and the gradient of its input
  grad.<parameter name>        the gradient of every parameter
  state.<buffer name>          running_mean / running_var of the four BatchNorms after the call
and nbt: num_batches_tracked of the four BatchNorms after the call (all 1)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from compare import NPROJ, sign_vectors  # noqa: E402
from synth import synth_randn, synth_state  # noqa: E402

REF = os.environ.get("NSID_REFERENCE") or os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference")
sys.path.insert(0, REF)
from encoder.resnet_ibn import ResidualIBN  # noqa: E402

torch.set_num_threads(8)
BLOCKS = ((64, 128, 1), (128, 256, 2))
B, H, W = 3, 6, 7
MAX_SAMPLE = 1024


def tag(cin, cout, stride):
    return f"c{cin}_{cout}_s{stride}"


def compact(out, name, t):
    a = t.detach().double().numpy()
    stride = max(7, -(-a.size // MAX_SAMPLE) | 1)
    f = a.reshape(-1)
    chk = np.concatenate([[f.sum(), np.abs(f).sum(), np.sqrt((f * f).sum()), np.abs(f).max()], sign_vectors(f.size, name) @ f])
    assert chk.size == 4 + NPROJ
    out[name + "@s"] = np.ascontiguousarray(f[::stride])
    out[name + "@c"] = chk
    out[name + "@m"] = np.array([stride, a.ndim, *a.shape], np.int64)


def gold():
    for cin, cout, stride in BLOCKS:
        t = tag(cin, cout, stride)
        blk = ResidualIBN(cin, cout, stride)
        blk.load_state_dict(synth_state(blk.state_dict(), prefix=t + "."))
        blk = blk.double().train()
        x = synth_randn(t, B, cin, H, W).double().requires_grad_(True)
        y = blk(x)
        dout = synth_randn(t + "_dout", *y.shape).double()
        y.backward(dout)
        out = {}
        compact(out, "out", y)
        compact(out, "dx", x.grad)
        for k, p in blk.named_parameters():
            compact(out, "grad." + k, p.grad)
        nbt = []
        for k, v in blk.state_dict().items():
            if k.endswith(("running_mean", "running_var")):
                compact(out, "state." + k, v)
            elif k.endswith("num_batches_tracked"):
                nbt.append(int(v))
        out["nbt"] = np.array(nbt, np.int64)
        path = os.path.join(HERE, f"resnet_train_{t}.npz")
        np.savez_compressed(path, **out)
        print(f"  {os.path.basename(path)}  {os.path.getsize(path) / 1024:.0f} KB  out {tuple(y.shape)}  nbt {nbt}")
        assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    gold()
