#!/usr/bin/env python3
"""Golden vectors of one TRAINING call of the reference's baseline (simclr/triplet.py BaselineModel over encoder/resnet_ibn.py
ResNetIBN), fp64, CPU: forward, the two losses of baseline/train.py, backward, and the BatchNorm state after the call.

Run from the repo root, where the reference checkout is available:

    python tests/golden/make_stem_train_golden.py

BaselineModel({}, ResNetIBN()).double().train() with synth.synth_state weights on the pair x_i, x_j =
synth_randn("stem_train_golden_i" / "_j", 2, 84, 40).abs() * 2 + 0.5; loss = classifier_loss(z_i, z_j) + triplet_loss(normalize(cat(z_i,
z_j)), cat(arange(2), arange(2)), 0.2). Writes stem_train_golden.npz with, in the compact form of tests/compare.py (fp64 samples, at most
1024 per tensor): h_i, h_j, z_i, z_j, grad.{conv1.weight, bn1.weight, bn1.bias, embedding_head.bias, global_pool.p},
state.bn1.running_mean / running_var; and plain: loss (loss_cls, loss_trip), nbt (every num_batches_tracked after the call: all 2)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_resnet_train_golden import compact  # noqa: E402
from synth import synth_randn, synth_state  # noqa: E402

REF = os.environ.get("NSID_REFERENCE") or os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference")
sys.path.insert(0, REF)
from encoder.resnet_ibn import ResNetIBN  # noqa: E402
from simclr.triplet import BaselineModel, classifier_loss, triplet_loss  # noqa: E402

torch.set_num_threads(8)
B, H, W = 2, 84, 40
GRADS = ("conv1.weight", "bn1.weight", "bn1.bias", "embedding_head.bias", "global_pool.p")


def gold():
    enc = ResNetIBN()
    enc.load_state_dict(synth_state(enc.state_dict()))
    model = BaselineModel({}, enc).double().train()
    x_i = (synth_randn("stem_train_golden_i", B, H, W).abs() * 2 + 0.5).double()
    x_j = (synth_randn("stem_train_golden_j", B, H, W).abs() * 2 + 0.5).double()
    h_i, h_j, z_i, z_j = model(x_i, x_j)
    z = torch.nn.functional.normalize(torch.cat([z_i, z_j], dim=0), dim=1, p=2)
    labels = torch.cat([torch.arange(B), torch.arange(B)], dim=0)
    loss_cls = classifier_loss(z_i, z_j)
    loss_trip = triplet_loss(z, labels, margin=0.2)
    (loss_cls + loss_trip).backward()
    out = {}
    for name, t in (("h_i", h_i), ("h_j", h_j), ("z_i", z_i), ("z_j", z_j)):
        compact(out, name, t)
    params = dict(enc.named_parameters())
    for k in GRADS:
        compact(out, "grad." + k, params[k].grad)
    sd = enc.state_dict()
    compact(out, "state.bn1.running_mean", sd["bn1.running_mean"])
    compact(out, "state.bn1.running_var", sd["bn1.running_var"])
    out["loss"] = np.array([float(loss_cls.detach()), float(loss_trip.detach())])
    out["nbt"] = np.array([int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")], np.int64)
    path = os.path.join(HERE, "stem_train_golden.npz")
    np.savez_compressed(path, **out)
    print(f"  {os.path.basename(path)}  {os.path.getsize(path) / 1024:.0f} KB  losses {out['loss']}  nbt {set(out['nbt'].tolist())} x {out['nbt'].size}")
    assert os.path.getsize(path) < 128 * 1024


if __name__ == "__main__":
    gold()
