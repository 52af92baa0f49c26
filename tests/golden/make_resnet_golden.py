#!/usr/bin/env python3
"""Golden vectors of the reference's ResNet-IBN baseline (simclr/triplet.py::BaselineModel over encoder/resnet_ibn.py::ResNetIBN),
eval mode, CPU.

Run from the repo root, in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_resnet_golden.py

Weights are synthesized by name (synth.synth_state) with ONE override, encoder.global_pool.p = 2.5 (the by-name rule would draw
p ~ 0.1 randn, for which pow(1/p) is meaningless; 2.5 and not the default 3 so that a hard-wired cube fails). Inputs by rule:
synth_randn(tag, B, 84, T).abs() * 2 (non-negative, like a CQT magnitude). Nothing but outputs, checksums and noise floors is stored.

Writes one resnet_ibn_b{B}_t{T}.npz per input with
  h, z                     (B, 2048) fp32 outputs of the fp32 reference
  stem, layer1..layer4     the stage outputs (B, C, H, W) in the compact form of tests/compare.py
  noise.fp32_rel_h / noise.fp32_max_dz / noise.fp32_rel.<stage>
                           the fp32 reference against the same model in fp64: the floor the fp32-storage tolerances are built from
  emul.bf16_min_cos / emul.bf16_rel_h / emul.bf16_max_dz
                           the fp64 model with every 4-D conv weight rounded to bf16 and the output of every Conv2d / BatchNorm2d /
                           InstanceNorm2d / MaxPool2d rounded to bf16, against plain fp64: the floor of the bf16-storage tolerances
  input_sha, stage_hw
and resnet_ibn_keys.json: the state_dict names and shapes, and per key (sum, l2 norm) of the default initialisation under
torch.manual_seed(42)."""
import copy
import hashlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from compare import NPROJ, sign_vectors  # noqa: E402
from synth import synth_randn, synth_state  # noqa: E402

# the reference checkout: $NSID_REFERENCE, or the directory `reference` next to this repository
REF = os.environ.get("NSID_REFERENCE") or os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference")
sys.path.insert(0, REF)
from encoder.resnet_ibn import ResNetIBN  # noqa: E402
from simclr.triplet import BaselineModel  # noqa: E402

torch.set_num_threads(8)
INPUTS = ((4, 216), (3, 100), (1, 216), (2, 431))
STAGES = ("stem", "layer1", "layer2", "layer3", "layer4")
GEM_P = 2.5
MAX_SAMPLE = 4096


def input_tag(B, T):
    return f"resnet_ibn_b{B}_t{T}"


def synth_input(B, T):
    return synth_randn(input_tag(B, T), B, 84, T).abs() * 2


def compact(out, name, arr):
    a = np.asarray(arr, np.float32)
    stride = max(7, -(-a.size // MAX_SAMPLE) | 1)
    f = a.reshape(-1).astype(np.float64)
    chk = np.concatenate([[f.sum(), np.abs(f).sum(), np.sqrt((f * f).sum()), np.abs(f).max()], sign_vectors(f.size, name) @ f])
    assert chk.size == 4 + NPROJ
    out[name + "@s"] = np.ascontiguousarray(a.reshape(-1)[::stride])
    out[name + "@c"] = chk
    out[name + "@m"] = np.array([stride, a.ndim, *a.shape], np.int64)


def build():
    model = BaselineModel({}, ResNetIBN())
    sd = synth_state(model.state_dict())
    sd["encoder.global_pool.p"] = torch.full((1,), GEM_P)
    model.load_state_dict(sd)
    return model.eval()


def run(model, x):
    """(h, z, {stage: tensor})"""
    got, hooks = {}, []
    enc = model.encoder
    for name, mod in (("stem", enc.maxpool), ("layer1", enc.layer1), ("layer2", enc.layer2), ("layer3", enc.layer3),
                      ("layer4", enc.layer4)):
        hooks.append(mod.register_forward_hook(lambda m, i, o, name=name: got.__setitem__(name, o.detach().clone())))
    with torch.no_grad():
        h, _, z, _ = model(x, x)
    for hk in hooks:
        hk.remove()
    return h, z, got


def bf16_emulation(model64):
    m = copy.deepcopy(model64)
    rnd = lambda t: t.to(torch.bfloat16).to(torch.float64)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 4:
                p.copy_(rnd(p))
    for mod in m.modules():
        if isinstance(mod, (nn.Conv2d, nn.BatchNorm2d, nn.InstanceNorm2d, nn.MaxPool2d)):
            mod.register_forward_hook(lambda m_, i, o: rnd(o))
    return m


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def gold():
    model = build()
    model64 = copy.deepcopy(model).double()
    emul = bf16_emulation(model64)
    for B, T in INPUTS:
        x = synth_input(B, T)
        h, z, st = run(model, x)
        h64, z64, st64 = run(model64, x.double())
        he, ze, _ = run(emul, x.double())
        assert torch.isfinite(h).all() and torch.isfinite(he).all()
        out = {"h": h.numpy(), "z": z.numpy()}
        hw = []
        for name in STAGES:
            compact(out, name, st[name].numpy())
            out[f"noise.fp32_rel.{name}"] = np.array([rel(st[name], st64[name])])
            hw.append(list(st[name].shape[1:]))
        out["stage_chw"] = np.array(hw, np.int64)
        out["noise.fp32_rel_h"] = np.array([rel(h, h64)])
        out["noise.fp32_max_dz"] = np.array([float((z.double() - z64).abs().max())])
        cos = (ze * z64).sum(1) / (ze.norm(dim=1) * z64.norm(dim=1))
        out["emul.bf16_min_cos"] = np.array([float(cos.min())])
        out["emul.bf16_rel_h"] = np.array([rel(he, h64)])
        out["emul.bf16_max_dz"] = np.array([float((ze - z64).abs().max())])
        out["input_sha"] = np.frombuffer(hashlib.sha256(x.numpy().tobytes()).hexdigest()[:16].encode(), np.uint8)
        path = os.path.join(HERE, input_tag(B, T) + ".npz")
        np.savez_compressed(path, **out)
        print(f"  {os.path.basename(path)}  {os.path.getsize(path) / 1024:.0f} KB  maps {hw}  fp32 rel h {out['noise.fp32_rel_h'][0]:.2e} "
              f"max dz {out['noise.fp32_max_dz'][0]:.2e} | stages " + " ".join(f"{out[f'noise.fp32_rel.{n}'][0]:.1e}" for n in STAGES) +
              f" | bf16 emul min cos {out['emul.bf16_min_cos'][0]:.7f} rel h {out['emul.bf16_rel_h'][0]:.2e} "
              f"max dz {out['emul.bf16_max_dz'][0]:.2e}")


def keys():
    torch.manual_seed(42)
    model = BaselineModel({}, ResNetIBN())
    sd = model.state_dict()
    res = {"keys": [[k, list(v.shape)] for k, v in sd.items()],
           "params": int(sum(p.numel() for p in model.parameters())),
           "init_seed": 42,
           "init": {k: [float(v.double().sum()), float(v.double().norm())] for k, v in sd.items()}}
    with open(os.path.join(HERE, "resnet_ibn_keys.json"), "w") as f:
        json.dump(res, f, separators=(",", ":"))
    print(f"  resnet_ibn_keys.json: {len(sd)} keys, {res['params'] / 1e6:.2f} M parameters")


if __name__ == "__main__":
    keys()
    gold()
