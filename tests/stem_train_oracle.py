"""The training-mode stem of the ResNet-IBN baseline (conv1 7x7 stride 2 pad 3 -> bn1 with batch statistics -> ReLU -> max-pool 3x3
stride 2 pad 1) restated in plain torch for any dtype, gradients by autograd; the closed form of its backward; the band of pooled
entries whose outcome rounding may decide; and the whole encoder (this stem + resnet_train_oracle.trunk_reference's forward). Not a
test module.

Closed form, with g the upstream gradient scattered to the conv pixel that wins each pooled window (first maximum in scan order) where
the winning value is > 0, xh = (r - mean) * invstd, N the number of conv pixels and patch_t the input under tap t (zero in the padding):
    dbeta = a = sum g,  dgamma = b = sum g xh,  dW[c, t] = gamma invstd (sum g patch_t - (a / N) sum patch_t - (b / N) sum xh patch_t)"""
import torch

import resnet_train_oracle as O

F = torch.nn.functional
SHAPES = ((3, 37, 70), (2, 21, 130), (1, 84, 65), (3, 1, 1))      # (B, H, W); (2, 84, 216) runs once on top
BAND_THR = 1e-4
BAND_CAP = 1e-3


def stem_state():
    """conv1.weight, bn1.* by the naming rule of tests/golden/synth.py: what synth_state gives the whole model"""
    from synth import synth_tensor
    like = {"conv1.weight": torch.empty(64, 1, 7, 7), "bn1.weight": torch.empty(64), "bn1.bias": torch.empty(64),
            "bn1.running_mean": torch.empty(64), "bn1.running_var": torch.empty(64)}
    return {k: synth_tensor(k, v) for k, v in like.items()}


def stem_input(B, H, W, tag=None):
    """CQT-magnitude-like: positive, a mean well away from zero"""
    from synth import synth_randn
    return synth_randn(tag or f"stem_train_{B}x{H}x{W}", B, H, W).abs() * 2 + 0.5


def stem_forward(x, sd, bf16=False):
    """x (B, H, W), sd: conv1.weight, bn1.{weight, bias, running_mean, running_var} in one dtype ->
    dict(y (B, 64, Hp, Wp), idx, pre, r, mean, invstd, running). bf16: the stored output is rounded to bf16 (the conv and the BatchNorm
    run in fp32 registers in the kernels: nothing else is stored)"""
    r = F.conv2d(x.unsqueeze(1), sd["conv1.weight"], stride=2, padding=3)
    pre, rm, rv = O.batch_norm_train(r, sd["bn1.weight"], sd["bn1.bias"], sd["bn1.running_mean"], sd["bn1.running_var"])
    y, idx = F.max_pool2d(torch.relu(pre), 3, 2, 1, return_indices=True)
    if bf16:
        y = O._Store.apply(y)
    mean = r.mean(dim=(0, 2, 3))
    invstd = (((r - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3)) + O.BN_EPS).rsqrt()
    return dict(y=y, idx=idx, pre=pre, r=r, mean=mean.detach(), invstd=invstd.detach(),
                running={"bn1.running_mean": rm, "bn1.running_var": rv})


def stem_reference(x, sd, dy, dtype, bf16=False):
    """forward and autograd backward in dtype -> dict(y, pre, idx, grads: {conv1.weight, bn1.weight, bn1.bias}, running)"""
    s = {k: v.to(dtype).clone() for k, v in sd.items()}
    names = ("conv1.weight", "bn1.weight", "bn1.bias")
    for k in names:
        s[k].requires_grad_(True)
    res = stem_forward(x.to(dtype), s, bf16=bf16)
    grads = torch.autograd.grad(res["y"], [s[k] for k in names], dy.to(dtype))
    return dict(y=res["y"].detach(), pre=res["pre"].detach(), idx=res["idx"], r=res["r"].detach(), mean=res["mean"],
                invstd=res["invstd"], grads=dict(zip(names, grads)), running=res["running"])


def stem_closed_form(x, sd, dy):
    """(dW (64, 1, 7, 7), dgamma, dbeta) by the closed form of the module docstring, in x's dtype"""
    with torch.no_grad():
        res = stem_forward(x, sd)
        r, y, idx = res["r"], res["y"], res["idx"]
        N = r.numel() // 64
        g = torch.zeros_like(r).flatten(2)
        g.scatter_add_(2, idx.flatten(2), (dy * (y > 0)).flatten(2))
        patches = F.unfold(x.unsqueeze(1), 7, padding=3, stride=2)               # (B, 49, Hc*Wc)
        xh = ((r - res["mean"].view(1, -1, 1, 1)) * res["invstd"].view(1, -1, 1, 1)).flatten(2)
        a, b = g.sum((0, 2)), (g * xh).sum((0, 2))
        A = torch.einsum("bcl,btl->ct", g, patches)
        S = patches.sum((0, 2))
        X = torch.einsum("bcl,btl->ct", xh, patches)
        dW = (sd["bn1.weight"] * res["invstd"]).view(-1, 1) * (A - a.view(-1, 1) / N * S.view(1, -1) - b.view(-1, 1) / N * X)
    return dW.view(64, 1, 7, 7), b, a


def stem_band(pre, thr):
    """the pooled entries (b, c, hp, wp), as a bool tensor, whose outcome is not decided clear of rounding: with t1, t2 the two largest
    BatchNorm outputs in the 3x3 window and rms over the whole BatchNorm output, |t1| <= thr rms (the ReLU mask), or t1 > 0 and
    t1 - max(t2, 0) <= thr rms (the window's winner)"""
    rms = pre.pow(2).mean().sqrt()
    pp = F.pad(pre, (1, 1, 1, 1), value=float("-inf"))
    u = pp.unfold(2, 3, 2).unfold(3, 3, 2)
    win = u.reshape(*u.shape[:4], 9)
    top = win.topk(2, dim=-1).values
    t1, t2 = top[..., 0], top[..., 1]
    return (t1.abs() <= thr * rms) | ((t1 > 0) & ((t1 - t2.clamp(min=0)) <= thr * rms))


def encoder_forward(x, s, bf16=False):
    """the whole encoder in training mode on x (B, 84, T), free masks; s: the model's floating-point state in the dtype to compute in
    (entries may require gradients) -> dict(h, running: every BatchNorm's running statistics after this call)"""
    st = stem_forward(x, s, bf16=bf16)
    t, running = st["y"], dict(st["running"])
    for prefix, stride in O.LAYERS:
        res = O.block_forward(t, O.sub_state(s, prefix), stride, bf16=bf16)
        t = res["out"]
        running.update({prefix + k: v for k, v in res["running"].items()})
    p = s["global_pool.p"]
    pooled = t.clamp(min=1e-6).pow(p).mean(dim=(2, 3)).pow(1.0 / p)
    h = F.linear(pooled, s["embedding_head.weight"], s["embedding_head.bias"])
    return dict(h=h, running=running)


def baseline_forward(x_i, x_j, sd, dtype, bf16=False, grad=False):
    """BaselineModel.train()(x_i, x_j): two encoder passes, the second on the running statistics the first left ->
    dict(h_i, h_j, z_i, z_j, params: {name: the tensors the passes read}, state: running statistics and counters after the call).
    grad: keep the autograd graph (params then require gradients)"""
    s = {k: v.to(dtype).clone() for k, v in sd.items() if v.is_floating_point()}
    params = {k: v for k, v in s.items() if not k.endswith(("running_mean", "running_var"))}
    if grad:
        for v in params.values():
            v.requires_grad_(True)
    hs = []
    with torch.enable_grad() if grad else torch.no_grad():
        for x in (x_i, x_j):
            res = encoder_forward(x.to(dtype), s, bf16=bf16)
            hs.append(res["h"])
            s.update(res["running"])
        zs = [F.normalize(h, p=2, dim=1, eps=1e-10) for h in hs]
    state = {k: v.detach() for k, v in s.items() if k.endswith(("running_mean", "running_var"))}
    state.update({k: v + 2 for k, v in sd.items() if k.endswith("num_batches_tracked")})
    return dict(h_i=hs[0], h_j=hs[1], z_i=zs[0], z_j=zs[1], params=params, state=state)

