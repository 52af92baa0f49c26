"""Writes tests/golden/baseline_loss.npz from the REFERENCE's own loss functions (generation time only; the tests read the file).

    python tests/golden/make_baseline_loss_golden.py /path/to/NeuralSampleID

Imports the reference's simclr/triplet.py (torch alone) and evaluates triplet_loss, classifier_loss and the step objective of
baseline/train.py:66-77 on the inputs of tests/baseline_loss_oracle.py::CASES, once in fp32 (what the reference computes) and once in
fp64 (what it means). Per case <name>/...:
  sha256                 of the fp32 input bytes (the tests regenerate the inputs and check it)
  cls32, trip32, loss32  the reference's fp32 values (pair cases: loss = cls + trip, beta = gamma = 1); cls64, trip64, loss64
  dz32, dz64             autograd gradient of loss wrt cat(z_i, z_j), in the compact form of baseline_loss_oracle.compact
  dcls64, dtrip64        fp64 gradients of the two parts (dtrip through the step's normalisation), always sampled
  de32, de64             triplet cases: gradient wrt the embeddings
  valid, pidx, nidx, gap the mining decisions per anchor on the reference's fp32 similarities, and their decision gap
  floor_*                the reference's own |fp32 - fp64| per quantity (max abs for gradients): the tests allow the kernels 4 x that"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import baseline_loss_oracle as O  # noqa: E402


def load_reference(root):
    spec = importlib.util.spec_from_file_location("ref_triplet", os.path.join(root, "simclr", "triplet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ref_pair(ref, z_i, z_j, dtype):
    zi = z_i.to(dtype).clone().requires_grad_(True)
    zj = z_j.to(dtype).clone().requires_grad_(True)
    B = zi.shape[0]
    z = F.normalize(torch.cat([zi, zj], dim=0), dim=1, p=2)            # train.py:67
    labels = torch.cat([torch.arange(B), torch.arange(B)], dim=0)
    cls = ref.classifier_loss(zi, zj)
    trip = ref.triplet_loss(z, labels, margin=O.MARGIN).to(dtype)
    loss = 1.0 * cls + 1.0 * trip
    dcls = torch.cat(torch.autograd.grad(cls, (zi, zj), retain_graph=True))
    dtrip = torch.cat(torch.autograd.grad(trip, (zi, zj), allow_unused=True)) if trip.requires_grad else torch.zeros_like(dcls)
    return dict(cls=cls.detach(), trip=trip.detach(), loss=loss.detach(), dcls=dcls, dtrip=dtrip, dz=dcls + dtrip, zn=z.detach())


def ref_triplet(ref, e, labels, dtype):
    x = e.to(dtype).clone().requires_grad_(True)
    trip = ref.triplet_loss(x, labels, margin=O.MARGIN).to(dtype)
    de = torch.autograd.grad(trip, (x,))[0] if trip.requires_grad else torch.zeros_like(x)
    return dict(trip=trip.detach(), de=de)


def put(out, name, key, value):
    out[f"{name}/{key}"] = np.asarray(value)


def put_compact(out, name, key, t, whole):
    for k, v in O.compact(t, whole).items():
        out[f"{name}/{key}.{k}"] = v


def main(root):
    ref = load_reference(root)
    out = {}
    for name, (kind, args) in O.CASES.items():
        a, b = O.make_case(name)
        put(out, name, "sha256", O.input_digest(a, b))
        whole = a.shape[1] <= 256
        if kind == "pair":
            r32, r64 = ref_pair(ref, a, b, torch.float32), ref_pair(ref, a, b, torch.float64)
            for k in ("cls", "trip", "loss"):
                put(out, name, k + "32", r32[k].numpy())
                put(out, name, k + "64", r64[k].numpy())
                put(out, name, "floor_" + k, abs(float(r32[k]) - float(r64[k])))
            put_compact(out, name, "dz32", r32["dz"], whole)
            for k in ("dz", "dcls", "dtrip"):
                c64 = O.compact(r64[k], whole and k == "dz")
                for kk, v in c64.items():
                    out[f"{name}/{k}64.{kk}"] = v
                put(out, name, "floor_" + k, O.compact_maxerr(r32[k], c64))
            E32, labels = r32["zn"], O.pair_labels(a.shape[0])
        else:
            r32, r64 = ref_triplet(ref, a, b, torch.float32), ref_triplet(ref, a, b, torch.float64)
            put(out, name, "trip32", r32["trip"].numpy())
            put(out, name, "trip64", r64["trip"].numpy())
            put(out, name, "floor_trip", abs(float(r32["trip"]) - float(r64["trip"])))
            put_compact(out, name, "de32", r32["de"], whole)
            c64 = O.compact(r64["de"], whole)
            for kk, v in c64.items():
                out[f"{name}/de64.{kk}"] = v
            put(out, name, "floor_de", O.compact_maxerr(r32["de"], c64))
            E32, labels = a, b
        d = O.mine(E32 @ E32.T, labels, O.MARGIN)          # the reference's fp32 similarities: the same matmul on the same rows
        put(out, name, "valid", d["valid"].numpy())
        put(out, name, "pidx", d["pidx"].numpy().astype(np.int32))
        put(out, name, "nidx", d["nidx"].numpy().astype(np.int32))
        put(out, name, "gap", d["gap"].double().numpy())
        nv = int(d["valid"].sum())
        act = int(d["active"].sum())
        print(f"{name:10s} M={E32.shape[0]:4d} D={E32.shape[1]:5d} valid={nv:4d} active={act:4d} near-ties={int((d['gap'] < O.GAP_MIN).sum())} "
              + " ".join(f"{k[6:]}={float(v):.3g}" for k, v in out.items() if k.startswith(name + "/floor_")))
    path = os.path.join(HERE, "baseline_loss.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main(sys.argv[1])
