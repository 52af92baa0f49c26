"""Mirror of simclr/triplet.py (reference :6-83): BaselineModel.forward(x_i, x_j) -> (h_i, h_j, z_i, z_j) with
z = F.normalize(h, p=2, eps=1e-10) and an identity projector, and the two losses of the baseline's training step with the reference's
signatures, each one fused call of csrc/baseline_loss.hip, forward and backward. baseline_objective is the whole objective of
baseline/train.py:66-77 in one call. BaselineModel.train()(x_i, x_j) is the differentiable training forward (tools/
baseline_train_synthetic.py runs the reference's whole step with it). There is no host path: CPU tensors raise."""
import torch
import torch.nn as nn

from .. import ops

NORM_EPS = 1e-10


def _device_f32(name, *ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError(f"{name}: tensors must be on the GPU; there is no CPU path")
    return [t.contiguous().float() for t in ts]


class _TripletFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, embeddings, labels, margin, grad_on):
        need = grad_on and ctx.needs_input_grad[0]
        out, de = ops.triplet_fwd_bwd(embeddings, labels, margin, want_grad=need)
        if need:
            ctx.save_for_backward(de)
        return out[0].reshape(())

    @staticmethod
    def backward(ctx, g):
        (de,) = ctx.saved_tensors
        return ops.scale_f32(de, g.contiguous().float()), None, None, None


class _PairCeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z_i, z_j, grad_on):
        need = grad_on and any(ctx.needs_input_grad)
        out, dzi, dzj = ops.pair_ce_fwd_bwd(z_i, z_j, want_grad=need)
        if need:
            ctx.save_for_backward(dzi, dzj)
        return out[0].reshape(())

    @staticmethod
    def backward(ctx, g):
        dzi, dzj = ctx.saved_tensors
        g = g.contiguous().float()
        return ops.scale_f32(dzi, g), ops.scale_f32(dzj, g), None


class _ObjectiveFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z_i, z_j, margin, beta, gamma, grad_on):
        need = grad_on and any(ctx.needs_input_grad)
        out, dzi, dzj = ops.baseline_objective_fwd_bwd(z_i, z_j, margin, beta, gamma, want_grad=need)
        if need:
            ctx.save_for_backward(dzi, dzj)
        loss, cls, trip = out[0].reshape(()), out[1].reshape(()), out[2].reshape(())
        ctx.mark_non_differentiable(cls, trip)        # the parts are for logging: the gradient is that of the sum
        return loss, cls, trip

    @staticmethod
    def backward(ctx, g, _g_cls, _g_trip):
        dzi, dzj = ctx.saved_tensors
        g = g.contiguous().float()
        return ops.scale_f32(dzi, g), ops.scale_f32(dzj, g), None, None, None, None


def triplet_loss(embeddings, labels, margin=0.2):
    """semi-hard triplet loss (reference :6-40): embeddings (M, D), labels (M,) int64 -> 0-dim tensor"""
    (e,) = _device_f32("triplet_loss", embeddings)
    if not labels.is_cuda:
        raise RuntimeError("triplet_loss: tensors must be on the GPU; there is no CPU path")
    return _TripletFn.apply(e, labels.contiguous().long(), float(margin), torch.is_grad_enabled())


def classifier_loss(z_i, z_j):
    """pair cross-entropy (reference :44-61): row i of cat(z_i, z_j) against row i +- B -> 0-dim tensor"""
    zi, zj = _device_f32("classifier_loss", z_i, z_j)
    return _PairCeFn.apply(zi, zj, torch.is_grad_enabled())


def baseline_objective(z_i, z_j, margin=0.2, beta=1.0, gamma=1.0):
    """beta * classifier_loss(z_i, z_j) + gamma * triplet_loss(normalize(cat(z_i, z_j)), cat(arange(B), arange(B)), margin), the step
    objective of baseline/train.py:66-77 -> (loss, loss_cls, loss_trip), 0-dim tensors; the gradient flows through loss"""
    zi, zj = _device_f32("baseline_objective", z_i, z_j)
    return _ObjectiveFn.apply(zi, zj, float(margin), float(beta), float(gamma), torch.is_grad_enabled())


class _L2NormFn(torch.autograd.Function):
    """z = h / max(|h|, eps) per row (nsid_l2norm_fwd / nsid_l2norm_bwd)"""

    @staticmethod
    def forward(ctx, h, eps):
        z, norm = ops.l2norm_fwd(h, eps)
        ctx.save_for_backward(z, norm)
        ctx.eps = eps
        return z

    @staticmethod
    def backward(ctx, dz):
        z, norm = ctx.saved_tensors
        return ops.l2norm_bwd(dz.contiguous().float(), z, norm, ctx.eps), None


class BaselineModel(nn.Module):
    """forward(x_i, x_j) -> (h_i, h_j, z_i, z_j). In training mode (ResNetIBN encoder) the call is differentiable; as in the reference
    each view is an encoder pass of its own: batch statistics per view, and every BatchNorm's running statistics and counter move
    twice per call."""

    def __init__(self, cfg, encoder):
        super().__init__()
        self.encoder = encoder
        self.cfg = cfg
        self.projector = nn.Identity()

    def _embed(self, x):
        h = self.encoder(x)
        if self.training:
            return h, _L2NormFn.apply(self.projector(h).contiguous(), NORM_EPS)
        z, _ = ops.l2norm_fwd(self.projector(h), NORM_EPS)
        return h, z

    def forward(self, x_i, x_j):
        h_i, z_i = self._embed(x_i)
        h_j, z_j = self._embed(x_j)
        return h_i, h_j, z_i, z_j
