"""The pooling head of the ResNet-IBN baseline (encoder/resnet_ibn.py of the reference: GeMPooling, then nn.Linear) restated in plain
torch for any dtype, its closed-form backward, and the inputs of its tests. Not a test module.

With xh = max(x, eps), m = mean_hw xh^p, y = m^(1/p):
  dx = dy y^(1-p) xh^(p-1) / HW where x > eps, else 0
  dp = sum_{b,c} dy y ( sum_hw xh^p ln xh / (p HW m) - ln m / p^2 )"""
import torch

EPS = 1e-6


def gem(x, p, eps=EPS):
    """x (B, HW, C) -> (B, C): the reference's x.clamp(min=eps).pow(p), mean over the positions, .pow(1 / p)"""
    return x.clamp(min=eps).pow(p).mean(dim=1).pow(1.0 / p)


def gem_backward_closed_form(x, p, dy, eps=EPS):
    HW = x.shape[1]
    xh = x.clamp(min=eps)
    xp = xh.pow(p)
    m = xp.mean(dim=1)
    y = m.pow(1.0 / p)
    dx = (dy * y.pow(1.0 - p) / HW)[:, None, :] * xh.pow(p - 1.0) * (x > eps)
    dp = (dy * y * ((xp * xh.log()).sum(dim=1) / (p * HW * m) - m.log() / (p * p))).sum()
    return dx, dp


def make_rows(B, HW, C, seed, bf16):
    """activations with negative values and values below eps (both get exactly zero gradient), as (B, HW, C) fp32; with bf16 the
    values are bf16-representable"""
    g = torch.Generator().manual_seed(seed)
    x = 0.5 * torch.randn(B, HW, C, generator=g) + 0.3
    x[:, ::3, ::5] = 3e-7                      # below eps, positive
    return x.bfloat16().float() if bf16 else x


def autograd_reference(x, p, dy, dtype, weight=None, bias=None, dh=None):
    """gradients of the reference's formula by autograd in dtype: dict of y, dx, dp and, with a head, h, dw, db"""
    xs = x.to(dtype).clone().requires_grad_(True)
    ps = torch.tensor([p], dtype=dtype, requires_grad=True)
    y = gem(xs, ps)
    if weight is None:
        dx, dp = torch.autograd.grad(y, (xs, ps), dy.to(dtype))
        return dict(y=y.detach(), dx=dx, dp=dp)
    w = weight.to(dtype).clone().requires_grad_(True)
    b = bias.to(dtype).clone().requires_grad_(True)
    h = torch.nn.functional.linear(y, w, b)
    dx, dp, dw, db = torch.autograd.grad(h, (xs, ps, w, b), dh.to(dtype))
    return dict(h=h.detach(), dx=dx, dp=dp, dw=dw, db=db)
