"""Mirror of simclr/triplet.py::BaselineModel (reference :65-83): forward(x_i, x_j) -> (h_i, h_j, z_i, z_j) with
z = F.normalize(h, p=2, eps=1e-10) and an identity projector. The triplet / classifier losses of that file are training code and
are not part of this project (the baseline is evaluated here, not trained)."""
import torch.nn as nn

from .. import ops

NORM_EPS = 1e-10


class BaselineModel(nn.Module):
    def __init__(self, cfg, encoder):
        super().__init__()
        self.encoder = encoder
        self.cfg = cfg
        self.projector = nn.Identity()

    def _embed(self, x):
        h = self.encoder(x)
        z, _ = ops.l2norm_fwd(self.projector(h), NORM_EPS)
        return h, z

    def forward(self, x_i, x_j):
        h_i, z_i = self._embed(x_i)
        h_j, z_j = self._embed(x_j)
        return h_i, h_j, z_i, z_j
