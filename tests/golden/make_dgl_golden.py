#!/usr/bin/env python3
"""Golden vectors of the reference's DGL-variant encoder (encoder/dgl/graph_encoder.py::GraphEncoderDGL), CPU, fp32.

Run from the repo root, in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_dgl_golden.py

`dgl` is not installed here: a small torch stand-in replaces it in sys.modules, so that the unused graph blocks really execute
(brute-force segmented kNN, dgl.graph / edges / local_scope / ndata / apply_edges, update_all with copy_e and a max reducer,
add_self_loop). The blocks' outputs are discarded by the reference (graph_encoder.py:149-160), so the stand-in's edge order and
degree handling cannot reach any recorded value. Weights are synthesized by name (synth.py) and the clips by rule
(synth.synth_clips), so no weights and no inputs are committed.

Writes dgl_passthrough_b8.npz (eval h / z / node matrix, one training step's loss, z, live-parameter gradients and live running
statistics) and dgl_keys.json (state_dict names and shapes for sizes t, s, m and the default)."""
import contextlib
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from compare import NPROJ, sign_vectors  # noqa: E402
from synth import GRAFP_CFG, synth_clips, synth_state  # noqa: E402

REF = os.environ.get("NSID_REFERENCE", "/root/reference")
# the live parameters of SimCLR(GraphEncoderDGL): peak extractor, stem, the three Downsample layers (size 't': backbone 2, 5, 12),
# proj, projector
LIVE_T = ("peak_extractor.", "encoder.stem.", "encoder.backbone.2.", "encoder.backbone.5.", "encoder.backbone.12.", "encoder.proj.",
          "projector.")
MAX_SAMPLE = 8192       # elements kept of one large tensor (compact form: every stride-th element + checksums + projections)


class _Graph:
    def __init__(self, src, dst, num_nodes):
        self.src, self.dst, self.num_nodes = src.long(), dst.long(), int(num_nodes)
        self.ndata, self.edata = {}, {}

    def edges(self):
        return self.src, self.dst

    def to(self, device):
        return self

    @contextlib.contextmanager
    def local_scope(self):
        nd, ed = dict(self.ndata), dict(self.edata)
        try:
            yield
        finally:
            self.ndata, self.edata = nd, ed

    def apply_edges(self, fn):
        e = types.SimpleNamespace(src={k: v[self.src] for k, v in self.ndata.items()},
                                  dst={k: v[self.dst] for k, v in self.ndata.items()})
        self.edata.update(fn(e))

    def update_all(self, message, reduce):
        kind, field, name = message
        assert kind == "copy_e"
        m = self.edata[field]
        order = torch.argsort(self.dst, stable=True)
        deg = torch.bincount(self.dst, minlength=self.num_nodes)
        start = torch.cumsum(deg, 0) - deg
        out = None
        for d in sorted(set(deg.tolist()) - {0}):                # DGL's degree buckets; a node without messages gets zeros
            nodes = torch.nonzero(deg == d).flatten()
            eidx = order[(start[nodes][:, None] + torch.arange(d)[None, :]).reshape(-1)]
            res = reduce(types.SimpleNamespace(mailbox={name: m[eidx].reshape(len(nodes), d, -1)}))
            for k, v in res.items():
                if out is None:
                    out = {k: torch.zeros((self.num_nodes,) + tuple(v.shape[1:]), dtype=v.dtype)}
                out[k][nodes] = v
        self.ndata.update(out or {})


def _segmented_knn_graph(x, k, segs, algorithm=None):
    """DGL's segmented_knn_graph, brute force: k nearest points of each point within its segment (the point itself included),
    edges neighbour -> point"""
    src, dst, off = [], [], 0
    for n in segs:
        xs = x[off:off + n]
        d = torch.cdist(xs, xs)
        nn_ = torch.topk(d, min(k, n), dim=1, largest=False).indices
        dst.append(torch.arange(n).repeat_interleave(nn_.shape[1]) + off)
        src.append(nn_.reshape(-1) + off)
        off += n
    return _Graph(torch.cat(src), torch.cat(dst), off)


def _install_stubs():
    dgl = types.ModuleType("dgl")
    dgl.segmented_knn_graph = _segmented_knn_graph
    dgl.graph = lambda e, num_nodes: _Graph(e[0], e[1], num_nodes)
    dgl.add_self_loop = lambda g: _Graph(torch.cat([g.src, torch.arange(g.num_nodes)]),
                                         torch.cat([g.dst, torch.arange(g.num_nodes)]), g.num_nodes)
    fn = types.ModuleType("dgl.function")
    fn.copy_e = lambda field, out: ("copy_e", field, out)
    dgl.function = fn
    dnn = types.ModuleType("dgl.nn")
    for cls in ("GraphConv", "EdgeConv", "SAGEConv", "GINConv"):      # imported by name, never built with conv='mr'
        setattr(dnn, cls, type(cls, (nn.Module,), {}))
    dgl.nn = dnn
    sys.modules.update({"dgl": dgl, "dgl.function": fn, "dgl.nn": dnn})


_install_stubs()
sys.path.insert(0, REF)
from encoder.dgl.graph_encoder import GraphEncoderDGL  # noqa: E402
from simclr.ntxent import ntxent_loss  # noqa: E402
from simclr.simclr import SimCLR  # noqa: E402

torch.set_num_threads(8)
CFG = dict(GRAFP_CFG)


def compact(out, name, arr):
    """tests/compare.py's compact form with a stride that keeps at most MAX_SAMPLE elements (odd: co-prime with the extents)"""
    a = np.asarray(arr, np.float32)
    if a.size <= MAX_SAMPLE:
        out[name] = a
        return
    stride = -(-a.size // MAX_SAMPLE) | 1
    f = a.reshape(-1).astype(np.float64)
    chk = np.concatenate([[f.sum(), np.abs(f).sum(), np.sqrt((f * f).sum()), np.abs(f).max()], sign_vectors(f.size, name) @ f])
    assert chk.size == 4 + NPROJ
    out[name + "@s"] = np.ascontiguousarray(a.reshape(-1)[::stride])
    out[name + "@c"] = chk
    out[name + "@m"] = np.array([stride, a.ndim, *a.shape], np.int64)


def keys():
    res = {}
    for size in ("t", "s", "m", "b"):
        enc = GraphEncoderDGL(cfg=CFG, in_channels=CFG["n_filters"], k=3, size=size)
        sd = enc.state_dict()
        res[size] = {"keys": [[k, list(v.shape)] for k, v in sd.items()],
                     "params": int(sum(p.numel() for p in enc.parameters()))}
        print(f"  size {size}: {len(sd)} keys, {res[size]['params'] / 1e6:.2f} M parameters")
    with open(os.path.join(HERE, "dgl_keys.json"), "w") as f:
        json.dump(res, f, separators=(",", ":"))


def gold():
    B = 8
    x_i, x_j = synth_clips(B)
    torch.manual_seed(1234)
    model = SimCLR(CFG, GraphEncoderDGL(cfg=CFG, in_channels=CFG["n_filters"], k=3, size="t"))
    model.load_state_dict(synth_state(model.state_dict()))
    live = [n for n, _ in model.named_parameters() if n.startswith(LIVE_T)]
    out = {}
    model.eval()
    with torch.no_grad():
        h_i, h_j, z_i, z_j = model(x_i, x_j)
        nodes, emb = model.encoder(model.peak_extractor(x_i), return_pre_proj=True)
    assert torch.equal(emb, h_i)
    out.update(h_i_eval=h_i.numpy(), z_i_eval=z_i.numpy(), z_j_eval=z_j.numpy())
    compact(out, "nodes_i_eval", nodes.numpy())
    model.train()
    model.zero_grad()
    h_i, h_j, z_i, z_j = model(x_i, x_j)
    loss = ntxent_loss(z_i, z_j, CFG)
    loss.backward()
    out.update(loss_train=np.array([float(loss.detach())], np.float64), z_i_train=z_i.detach().numpy(), z_j_train=z_j.detach().numpy())
    for n, p in model.named_parameters():
        if n in live:
            compact(out, "grad." + n, p.grad.numpy())
    for n, t in model.state_dict().items():
        if n.startswith(LIVE_T) and ("running" in n or "num_batches" in n):
            out["bn." + n] = t.numpy()
    dead = [n for n, p in model.named_parameters() if n not in live]
    assert dead and all(model.get_parameter(n).grad is None for n in dead)     # the blocks ran, their outputs were discarded
    import hashlib
    out["clips_sha"] = np.frombuffer(hashlib.sha256(x_i.numpy().tobytes() + x_j.numpy().tobytes()).hexdigest()[:16].encode(), np.uint8)
    out["live_names"] = np.frombuffer(json.dumps(live).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "dgl_passthrough_b8.npz")
    np.savez_compressed(path, **out)
    print(f"  dgl_passthrough_b8.npz  {os.path.getsize(path) / 1024:.0f} KB, loss {float(loss):.6f}, {len(live)} live parameters")


if __name__ == "__main__":
    keys()
    gold()
