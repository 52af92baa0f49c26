"""The reference's DGL-variant encoder as it computes: encoder/dgl/graph_encoder.py::GraphEncoderDGL (reference :67-160).

Its `_apply_graph_block` (reference :149-160) builds the kNN graph and runs GrapherDGL and FFN, then returns its input `x`
unchanged, so no graph block reaches the output. The network that does is

    stem (1x1 conv, no bias, BatchNorm2d, LeakyReLU 0.2) -> 3 x Downsample (Conv1d k3 s2 p1 + bias, BatchNorm1d, ReLU)
    -> proj (1x1, bias) -> mean over nodes

and `forward(x, return_pre_proj=True)` returns the last Downsample's output (after its ReLU) as the node matrix.
`PassthroughGraphEncoderDGL` reproduces that function on the gfx950 kernels (functional.dgl_chain_forward, csrc/dsact.hip) and
carries the reference's whole module tree, so a DGL-variant checkpoint (449 state_dict keys at size 't') loads and saves strictly.

The unused blocks' parameters never receive a gradient (`grad is None`, as in the reference). Their BatchNorm running statistics
are left untouched: the reference updates them in training mode, because it computes the blocks before discarding them, but
nothing ever reads those buffers. The DGL edge dropout and `include_self` reach only the unused blocks."""
import torch
import torch.nn as nn

from ... import functional as F_
from ..gcn_lib.torch_vertex import _split

SIZES = {"t": ([2, 2, 6, 2], [64, 128, 256, 512]), "s": ([2, 2, 6, 2], [80, 160, 400, 640]),
         "m": ([2, 2, 16, 2], [96, 192, 384, 768])}
SIZE_DEFAULT = ([2, 2, 18, 2], [128, 256, 512, 1024])
ACTS = ("relu", "leakyrelu", "gelu")


def _norm(norm, nc):
    """encoder/dgl/dgl_util.py::norm_layer (reference :27-34)"""
    if norm == "batch":
        return nn.BatchNorm1d(nc, affine=True)
    if norm == "instance":
        return nn.InstanceNorm1d(nc, affine=False)
    raise NotImplementedError(f"Normalization type {norm} is not implemented.")


class MRConv(nn.Module):
    """module tree of dgl_util.py::MRConv (reference :40-48): Linear(2C, C') + Identity + activation"""

    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__()
        self.nn = nn.Sequential(nn.Linear(in_channels * 2, out_channels, bias=bias), nn.Identity(), nn.ReLU())


class GrapherDGL(nn.Module):
    """module tree of dgl_util.py::GrapherDGL with conv='mr' (reference :127-175). Never computed (see the module docstring)."""

    def __init__(self, in_channels, norm=None):
        super().__init__()
        self.norm = _norm(norm, in_channels) if norm else None
        self.conv = MRConv(in_channels, in_channels * 2)
        self.fc1 = nn.Sequential(nn.Conv1d(in_channels, in_channels, kernel_size=1), nn.BatchNorm1d(in_channels))
        self.fc2 = nn.Sequential(nn.Conv1d(in_channels * 2, in_channels, kernel_size=1), nn.BatchNorm1d(in_channels))


class FFN(nn.Module):
    """module tree of encoder/dgl/graph_encoder.py::FFN (reference :34-64). Never computed."""

    def __init__(self, in_features, hidden_features):
        super().__init__()
        self.fc1 = nn.Conv1d(in_features, hidden_features, 1)
        self.bn1 = nn.BatchNorm1d(hidden_features)
        self.fc2 = nn.Conv1d(hidden_features, in_features, 1)
        self.bn2 = nn.BatchNorm1d(in_features)


class Downsample(nn.Module):
    """encoder/dgl/graph_encoder.py::Downsample (reference :8-31): Conv1d(k=3, stride 2, pad 1) + BatchNorm1d + ReLU"""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv1d(in_dim, out_dim, kernel_size=3, stride=2, padding=1), nn.BatchNorm1d(out_dim),
                                  nn.ReLU())


class PassthroughGraphEncoderDGL(nn.Module):
    """PassthroughGraphEncoderDGL(cfg, k=3, ..., size='t'): forward(x (B, in_channels, N)) -> (B, emb_dims); with
    return_pre_proj=True -> (x_nodes (B, C_last, N_last), x_emb). The reference's constructor signature (reference :67-69);
    conv='mr' only (the other convolutions are DGL library modules)."""

    def __init__(self, cfg=None, k=3, conv="mr", act="relu", norm="batch", bias=True, dropout=0.0, dilation=True, epsilon=0.2,
                 drop_path=0.1, size="t", emb_dims=1024, in_channels=3, include_self=False):
        if conv != "mr":
            raise NotImplementedError(f"PassthroughGraphEncoderDGL implements conv='mr' (the published model), not {conv!r}")
        if str(act).lower() not in ACTS:
            raise NotImplementedError(f"Activation function {act} is not implemented.")
        if norm and norm not in ("batch", "instance"):
            raise NotImplementedError(f"Normalization type {norm} is not implemented.")
        super().__init__()
        self.blocks, self.channels = (list(v) for v in SIZES.get(size, SIZE_DEFAULT))
        self.k, self.emb_dims, self.cfg = k, emb_dims, cfg
        self.act, self.norm, self.bias, self.dropout, self.dilation = act, norm, bias, dropout, dilation
        self.epsilon, self.drop_path, self.include_self = epsilon, drop_path, include_self
        self.stem = nn.Sequential(nn.Conv2d(in_channels, self.channels[0], kernel_size=1, bias=False),
                                  nn.BatchNorm2d(self.channels[0]), nn.LeakyReLU(negative_slope=0.2))
        self.backbone = nn.ModuleList([])
        for i in range(len(self.blocks)):
            if i > 0:
                self.backbone.append(Downsample(self.channels[i - 1], self.channels[i]))
            for _ in range(self.blocks[i]):
                self.backbone.append(nn.Sequential(GrapherDGL(self.channels[i], norm=norm),
                                                   FFN(self.channels[i], self.channels[i] * 4)))
        self.proj = nn.Conv2d(self.channels[-1], self.emb_dims, 1, bias=True)

    def downsamples(self):
        return [m for m in self.backbone if isinstance(m, Downsample)]

    def live_modules(self):
        """(prefix, module) of the layers that reach the output, under the names functional.dgl_chain_forward reads"""
        return [("stem.", self.stem)] + [(f"ds{i}.", m) for i, m in enumerate(self.downsamples())] + [("proj.", self.proj)]

    def forward_rows(self, nodes, B, N, return_nodes=False):
        """nodes (B*N, in_channels) node-major -> (B, emb_dims); with return_nodes also the node matrix as
        (rows (B*N_last, C_last), N_last, emb) — GraphEncoder.forward_rows's contract"""
        params, buffers = {}, {}
        for pre, m in self.live_modules()[:-1]:
            p, b = _split(m)
            params.update({pre + k: v for k, v in p.items()})
            buffers.update({pre + k: v for k, v in b.items()})
        x = F_.run_block(F_.dgl_chain_forward, F_.dgl_chain_backward, params, buffers, nodes, B, N, self.training)
        for _ in range(F_.DGL_DOWNSAMPLES):
            N = (N - 1) // 2 + 1
        params, buffers = _split(self.proj)
        emb = F_.run_block(F_.proj_mean_forward, F_.proj_mean_backward, params, buffers, x, B, N)
        return (x, N, emb) if return_nodes else emb

    def forward(self, x, return_pre_proj=False):
        B, C, N = x.shape
        out = self.forward_rows(F_.to_rows(x), B, N, return_nodes=return_pre_proj)
        if not return_pre_proj:
            return out
        rows, n_last, emb = out
        return F_.from_rows(rows, B, n_last), emb
