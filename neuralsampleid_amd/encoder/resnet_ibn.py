"""Module shells of the ResNet-IBN baseline (reference: encoder/resnet_ibn.py): the reference's constructor signatures, construction
order (a seeded default initialisation draws the reference's values) and state_dict (193 keys), with the EVAL-MODE forward on the
HIP kernels of csrc/resnet.hip.

Activations are channels-last rows (B*H*W, C) from the stem to the pooling, fp32 or bf16 storage (functional.ACT_DTYPE). Per
ResidualIBN block:
    identity = downsample conv 1x1 (stride s) with its BatchNorm folded     nsid_linear_fwd (s = 1) / nsid_conv2d_fwd (s = 2)
    conv1 1x1 (raw)                                                         nsid_linear_fwd
    IBN + ReLU                                                              nsid_ibn_relu_fwd (in place)
    conv2 3x3 stride s, bn2 folded (no activation)                          nsid_conv2d_fwd
    relu(conv3 1x1 with bn3 folded + identity)                              nsid_conv2d_fwd (1x1 form: addend + ReLU epilogue)
Packed / folded weights and their bf16 shadows are cached by ops.folded_conv_bn (parameter versions and state epochs in the key), so
a load_state_dict is seen by the next forward. The module forward raises on CPU tensors; in training mode ResNetIBN.forward is the
training path below (the block and pooling modules on their own still refuse it).

Training exists from the stem's output rows on: ResidualIBN.train_rows (one autograd.Function per block: batch statistics in all
four BatchNorms, running statistics updated as nn.BatchNorm2d does, nothing folded) and ResNetIBN.trunk_train (the eight blocks and
head_train). Per block, forward / backward:
    conv1 1x1 (raw r1)                     nsid_linear_fwd                      / nsid_linear_bwd_weight, nsid_linear_bwd_data
    BN-half statistics of r1               nsid_col_stat, nsid_bn_finalize
    IBN + ReLU -> y1                       nsid_ibn_relu_fwd                    / nsid_ibn_relu_bwd (y1 is recomputed from r1)
    conv2 3x3 stride s (raw r2)            nsid_conv2d_fwd                      / nsid_conv2d_bwd_weight, nsid_conv2d_bwd_data
    bn2 statistics                         nsid_col_stat, nsid_bn_finalize      / nsid_bn_bwd_*
    conv3 1x1 on bn2(r2) (applied on load) nsid_linear_fwd (statistics epilogue), nsid_bn_finalize / the row-GEMM backward kernels
    downsample 1x1 stride s (raw rd)       nsid_linear_fwd (s = 1) / nsid_conv2d_fwd + nsid_col_stat (s = 2), nsid_bn_finalize
    relu(bn3(r3) + bn_d(rd) or x)          nsid_bn_add_relu_fwd                 / nsid_relu_bwd, nsid_bn_bwd_*
Saved for backward per block: the input rows x (the previous block's output), the raw conv outputs r1, r2, r3, rd, the output rows
(the next block's x) and the per-channel affines.

The stem trains too (ResNetIBN.stem_train, _StemTrainFn): nsid_stem7_stat -> nsid_bn_finalize (bn1's running statistics move) ->
nsid_stem7_pool_train_fwd (the batch affine folded into conv1's weight on the device) / nsid_stem7_bwd, which recomputes the conv
from the input: saved are only the input and the affine. ResNetIBN.forward in training mode is stem_train + trunk_train, so
model.train()(x) is differentiable in every parameter; IBN.forward, ResidualBlock and GeMPooling.forward keep their refusals."""
import torch
import torch.nn as nn

from .. import functional as F_
from .. import ops

N_BINS = 84          # CQT bins of the baseline's input (config/resnet_ibn.yaml: (84, 216) segments)


def _bn_args(bn):
    return bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps


def _require_eval_gpu(module, x, what):
    if module.training:
        raise NotImplementedError(f"{what}: only the eval-mode forward is implemented on the MI355X path (no backward of the 2-D "
                                  "convolution, instance norm and GeM kernels exists): call eval() and run under torch.no_grad()")
    if not x.is_cuda:
        raise NotImplementedError(f"{what}: there is no CPU path; move the model and its input to the GPU")


class IBN(nn.Module):
    """first half of the channels through InstanceNorm2d(affine), second half through BatchNorm2d"""

    def __init__(self, channels):
        super().__init__()
        half1 = int(channels * 0.5)
        self.IN = nn.InstanceNorm2d(half1, affine=True)
        self.BN = nn.BatchNorm2d(channels - half1)

    def relu_rows(self, r, B, HW):
        """relu(IBN(r)) on rows (B*HW, C), in place"""
        C = r.shape[1]
        if self.IN.num_features != C // 2 or self.IN.track_running_stats:
            raise NotImplementedError("IBN on the MI355X path: InstanceNorm2d over the first C/2 channels, without running statistics")
        aff = ops.bn_eval_affine(*_bn_args(self.BN))
        return ops.ibn_relu_fwd(r, B, HW, C, self.IN.weight, self.IN.bias, aff, self.IN.eps, out=r)

    def forward(self, x):
        raise NotImplementedError("IBN without the ReLU behind it is not a kernel of this library (nsid_ibn_relu_fwd fuses the two): "
                                  "run it through ResidualIBN / ResNetIBN")


class _Bottleneck(nn.Module):
    """conv1 1x1 -> norm -> ReLU -> conv2 3x3 (stride) -> bn2 -> conv3 1x1 -> bn3 -> + identity -> ReLU"""

    def _build(self, in_channels, out_channels, stride, norm1):
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, bias=False)
        self.bn1 = norm1(out_channels)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_channels)
        self.conv3 = nn.Conv2d(out_channels, out_channels, kernel_size=1, stride=1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if stride != 1 or in_channels != out_channels:
            self.downsample = nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=stride, bias=False),
                                            nn.BatchNorm2d(out_channels))

    def forward_rows(self, x, B, H, W):
        """x (B*H*W, Cin) rows -> (rows (B*Ho*Wo, Cout), Ho, Wo)"""
        Cin, Cout, s = self.conv1.in_channels, self.conv1.out_channels, self.conv2.stride[0]
        M = B * H * W
        identity = x
        if self.downsample is not None:
            dconv, dbn = self.downsample[0], self.downsample[1]
            if s == 1:      # a row GEMM
                wf, bf = ops.folded_conv_bn(ops.w2d(dconv.weight), None, *_bn_args(dbn))
                identity, _ = ops.linear_fwd(x, wf, bf, M, Cout, Cin)
            else:
                wf, bf = ops.packed_conv_bn(dconv.weight, *_bn_args(dbn))
                identity = ops.conv2d_fwd(x, B, H, W, Cin, wf, bf, Cout, 1, s)
        if isinstance(self.bn1, IBN):
            r, _ = ops.linear_fwd(x, ops.w2d(self.conv1.weight), None, M, Cout, Cin)
            y = self.bn1.relu_rows(r, B, H * W)
        else:
            w1, b1 = ops.folded_conv_bn(ops.w2d(self.conv1.weight), None, *_bn_args(self.bn1))
            y, _ = ops.linear_fwd(x, w1, b1, M, Cout, Cin, act_out=ops.ACT_RELU)
        w2, b2 = ops.packed_conv_bn(self.conv2.weight, *_bn_args(self.bn2))
        y = ops.conv2d_fwd(y, B, H, W, Cout, w2, b2, Cout, 3, s)
        Ho, Wo = ops.conv_out_size(H, 3, s), ops.conv_out_size(W, 3, s)
        w3, b3 = ops.packed_conv_bn(self.conv3.weight, *_bn_args(self.bn3))
        return ops.conv2d_fwd(y, B, Ho, Wo, Cout, w3, b3, Cout, 1, 1, addend=identity, relu=True), Ho, Wo

    def forward(self, x):
        _require_eval_gpu(self, x, type(self).__name__)
        B, C, H, W = x.shape
        rows = x.permute(0, 2, 3, 1).reshape(B * H * W, C).to(F_.ACT_DTYPE).contiguous()
        out, Ho, Wo = self.forward_rows(rows, B, H, W)
        return rows_to_bchw(out, B, Ho, Wo)


class ResidualIBN(_Bottleneck):
    def __init__(self, in_channels, out_channels, stride=1):
        super().__init__()
        self._build(in_channels, out_channels, stride, IBN)

    def _train_params(self):
        ps = [self.conv1.weight, self.bn1.IN.weight, self.bn1.IN.bias, self.bn1.BN.weight, self.bn1.BN.bias, self.conv2.weight,
              self.bn2.weight, self.bn2.bias, self.conv3.weight, self.bn3.weight, self.bn3.bias]
        if self.downsample is not None:
            ps += [self.downsample[0].weight, self.downsample[1].weight, self.downsample[1].bias]
        return ps

    def train_rows(self, x, B, H, W):
        """training-mode forward on rows x (B*H*W, Cin), fp32 or bf16 -> (rows (B*Ho*Wo, Cout), Ho, Wo), differentiable: batch
        statistics in the four BatchNorms (the running statistics and num_batches_tracked move as in nn.BatchNorm2d), backward fills
        the gradients of x and of every parameter of the block"""
        if not x.is_cuda:
            raise NotImplementedError("ResidualIBN.train_rows: there is no CPU path; move the model and its input to the GPU")
        Cin, s = self.conv1.in_channels, self.conv2.stride[0]
        if x.dim() != 2 or tuple(x.shape) != (B * H * W, Cin):
            raise ValueError(f"train_rows: expected rows ({B * H * W}, {Cin}), got {tuple(x.shape)}")
        if self.bn1.IN.num_features != self.conv1.out_channels // 2 or self.bn1.IN.track_running_stats:
            raise NotImplementedError("IBN on the MI355X path: InstanceNorm2d over the first C/2 channels, without running statistics")
        out = _BlockTrainFn.apply(x, self, B, H, W, *self._train_params())
        return out, ops.conv_out_size(H, 3, s), ops.conv_out_size(W, 3, s)


class ResidualBlock(_Bottleneck):
    def __init__(self, in_channels, out_channels, stride=1):
        super().__init__()
        self._build(in_channels, out_channels, stride, nn.BatchNorm2d)


class GeMPooling(nn.Module):
    def __init__(self, p=3, eps=1e-6):
        super().__init__()
        self.p = nn.Parameter(torch.ones(1) * p)
        self.eps = eps

    def pool_rows(self, rows, B, HW):
        """rows (B*HW, C) -> (B, C) fp32; p is read by the kernel from device memory (no host read: capturable)"""
        return ops.gem_pool_fwd(rows, B, HW, rows.shape[1], self.p, self.eps)

    def forward(self, x):
        _require_eval_gpu(self, x, "GeMPooling")
        B, C, H, W = x.shape
        rows = x.permute(0, 2, 3, 1).reshape(B * H * W, C).to(F_.ACT_DTYPE).contiguous()
        return self.pool_rows(rows, B, H * W).view(B, C, 1, 1)


class _HeadTrainFn(torch.autograd.Function):
    """GeM pooling -> embedding head on rows (B*HW, 1024), with its backward (nsid_gem_pool_bwd and the row-GEMM backward kernels)"""

    @staticmethod
    def forward(ctx, rows, p, weight, bias, B, HW, eps):
        C, E = weight.shape[1], weight.shape[0]
        pooled = ops.gem_pool_fwd(rows, B, HW, C, p, eps)
        # B rows against a 1024-deep reduction: split it, as the projection head of the GNN path does in training
        # (functional.proj_mean_forward): 4 x the workgroups and 4 x shorter fp32 summation chains; the partial sums meet in atomics
        h, _ = ops.linear_fwd(pooled, weight, bias, B, E, C, ksplit=4 if (C >= 512 and B <= 512) else 1)
        ctx.save_for_backward(rows, p, weight, pooled)
        ctx.dims = (B, HW, C, E, eps)
        return h

    @staticmethod
    def backward(ctx, dh):
        rows, p, weight, pooled = ctx.saved_tensors
        B, HW, C, E, eps = ctx.dims
        dh = dh.contiguous()
        dw = ops.zeros((E, C), dh.device)
        db = ops.zeros((E,), dh.device)
        ops.linear_bwd_weight(dh, pooled, dw, B, E, C)
        ops.colsum_acc(dh, db)
        dpooled = ops.linear_bwd_data(dh, weight, B, E, C)
        drows, dp = ops.gem_pool_bwd(rows, dpooled, B, HW, C, p, eps)
        return drows, dp, dw, db, None, None, None


def _bn_train(stat, M, bn):
    """batch statistics -> BNAffine; running_mean / running_var / num_batches_tracked move as in nn.BatchNorm2d.train()"""
    if bn.momentum is None or not bn.track_running_stats or not bn.affine:
        raise NotImplementedError("training-mode BatchNorm on the MI355X path: affine, running statistics, a fixed momentum")
    return ops.bn_finalize(stat, M, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps)


class _BlockTrainFn(torch.autograd.Function):
    """one ResidualIBN block in training mode on rows; parameters in the order of _Bottleneck._train_params"""

    @staticmethod
    def forward(ctx, x, blk, B, H, W, *params):
        Cin, Cout, s = blk.conv1.in_channels, blk.conv1.out_channels, blk.conv2.stride[0]
        M = B * H * W
        Ho, Wo = ops.conv_out_size(H, 3, s), ops.conv_out_size(W, 3, s)
        Mo = B * Ho * Wo
        ibn = blk.bn1
        half = Cout // 2
        x = x.contiguous()
        # main branch
        r1, _ = ops.linear_fwd(x, ops.w2d(blk.conv1.weight), None, M, Cout, Cin)
        aff1 = _bn_train(ops.col_stat(r1[:, half:], M, Cout - half), M, ibn.BN)
        y1 = ops.ibn_relu_fwd(r1, B, H * W, Cout, ibn.IN.weight, ibn.IN.bias, aff1, ibn.IN.eps)
        r2 = ops.conv2d_fwd(y1, B, H, W, Cout, ops.packed_conv(blk.conv2.weight), None, Cout, 3, s)
        del y1                                # recomputed from r1 in backward
        aff2 = _bn_train(ops.col_stat(r2, Mo, Cout), Mo, blk.bn2)
        r3, stat3 = ops.linear_fwd(r2, ops.w2d(blk.conv3.weight), None, Mo, Cout, Cout, want_stat=True, in_aff=aff2)
        aff3 = _bn_train(stat3, Mo, blk.bn3)
        # shortcut
        rd, affd = None, None
        if blk.downsample is not None:
            dconv, dbn = blk.downsample[0], blk.downsample[1]
            if s == 1:
                rd, statd = ops.linear_fwd(x, ops.w2d(dconv.weight), None, M, Cout, Cin, want_stat=True)
            else:
                rd = ops.conv2d_fwd(x, B, H, W, Cin, ops.packed_conv(dconv.weight), None, Cout, 1, s)
                statd = ops.col_stat(rd, Mo, Cout)
            affd = _bn_train(statd, Mo, dbn)
        out = ops.bn_add_relu_fwd(r3, aff3, x if rd is None else rd, affd)
        ctx.save_for_backward(x, r1, r2, r3, rd, out)
        ctx.blk, ctx.dims, ctx.affs = blk, (B, H, W, Ho, Wo), (aff1, aff2, aff3, affd)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, r1, r2, r3, rd, out = ctx.saved_tensors
        blk = ctx.blk
        B, H, W, Ho, Wo = ctx.dims
        aff1, aff2, aff3, affd = ctx.affs
        Cin, Cout, s = blk.conv1.in_channels, blk.conv1.out_channels, blk.conv2.stride[0]
        M, Mo, half = B * H * W, B * Ho * Wo, Cout // 2
        ibn = blk.bn1
        dev = x.device
        z = lambda *shape: ops.zeros(shape, dev)
        g = ops.relu_bwd(dout.to(out.dtype).contiguous(), out)
        # conv3 + bn3
        dg3, db3 = z(Cout), z(Cout)
        d3 = ops.bn_backward(g, r3, aff3, ops.ACT_NONE, dg3, db3)
        dw3 = z(Cout, Cout)
        ops.linear_bwd_weight(d3, r2, dw3, Mo, Cout, Cout, in_scale=aff2.scale, in_shift=aff2.shift)
        dz2 = ops.linear_bwd_data(d3, ops.w2d(blk.conv3.weight), Mo, Cout, Cout)
        # conv2 + bn2
        dg2, db2 = z(Cout), z(Cout)
        d2 = ops.bn_backward(dz2, r2, aff2, ops.ACT_NONE, dg2, db2, inplace=True)
        y1 = ops.ibn_relu_fwd(r1, B, H * W, Cout, ibn.IN.weight, ibn.IN.bias, aff1, ibn.IN.eps)
        dw2p = z(Cout, 9 * Cout)
        ops.conv2d_bwd_weight(d2, y1, dw2p, B, H, W, Cout, Cout, 3, s)
        dy1 = ops.conv2d_bwd_data(d2, B, H, W, Cout, ops.packed_conv_bwd(blk.conv2.weight), Cout, 3, s)
        del y1
        # IBN + conv1
        dgi, dbi, dgb, dbb = z(half), z(half), z(Cout - half), z(Cout - half)
        dr1 = ops.ibn_relu_bwd(dy1, r1, B, H * W, Cout, ibn.IN.weight, ibn.IN.bias, aff1, dgi, dbi, dgb, dbb, ibn.IN.eps, out=dy1)
        dw1 = z(Cout, Cin)
        ops.linear_bwd_weight(dr1, x, dw1, M, Cout, Cin)
        w1 = ops.w2d(blk.conv1.weight)
        grads = [dw1.view_as(blk.conv1.weight), dgi, dbi, dgb, dbb, ops.unpack_conv_wgrad(dw2p, Cout, 3), dg2, db2,
                 dw3.view_as(blk.conv3.weight), dg3, db3]
        # shortcut: the block's input receives both gradients in one pass (the addend of the last backward-data launch)
        if rd is None:
            dx = ops.linear_bwd_data(dr1, w1, M, Cout, Cin, addend=g)
        else:
            dconv = blk.downsample[0]
            dgd, dbd = z(Cout), z(Cout)
            dd = ops.bn_backward(g, rd, affd, ops.ACT_NONE, dgd, dbd, inplace=True)
            if s == 1:
                dwd = z(Cout, Cin)
                ops.linear_bwd_weight(dd, x, dwd, M, Cout, Cin)
                dxs = ops.linear_bwd_data(dd, ops.w2d(dconv.weight), M, Cout, Cin)
                dx = ops.linear_bwd_data(dr1, w1, M, Cout, Cin, addend=dxs)
            else:
                dwd = z(Cout, Cin)
                ops.conv2d_bwd_weight(dd, x, dwd, B, H, W, Cin, Cout, 1, s)
                dxm = ops.linear_bwd_data(dr1, w1, M, Cout, Cin)
                dx = ops.conv2d_bwd_data(dd, B, H, W, Cin, ops.packed_conv_bwd(dconv.weight), Cout, 1, s, addend=dxm)
            grads += [dwd.view_as(dconv.weight), dgd, dbd]
        return (dx, None, None, None, None) + tuple(grads)


class _StemTrainFn(torch.autograd.Function):
    """conv1 7x7 s2 -> bn1 (batch statistics) -> ReLU -> max-pool 3x3 s2 on x (B, H, W) -> rows (B*Hp*Wp, 64). Saved: x and the
    affine; the input is data and gets no gradient"""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, bn, dtype):
        w49 = ops.w2d(w)
        stat, tiles, N = ops.stem7_stat(x, w49)
        aff = ops.bn_finalize(stat, N, gamma, beta, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, bn.eps,
                              tiles=tiles)
        rows, _, _ = ops.stem7_pool_train_fwd(x, w49, aff, dtype)
        ctx.save_for_backward(x, w, gamma)
        ctx.aff = aff
        return rows

    @staticmethod
    def backward(ctx, drows):
        x, w, gamma = ctx.saved_tensors
        dw, dg, db = ops.stem7_bwd(drows.contiguous(), x, ops.w2d(w), ctx.aff, gamma)
        return None, dw.view_as(w), dg, db, None, None


def rows_to_bchw(rows, B, H, W):
    """channels-last rows (B*H*W, C) -> the reference's (B, C, H, W) fp32 tensor (module boundary / tests: off the hot path)"""
    return rows.float().view(B, H, W, rows.shape[1]).permute(0, 3, 1, 2).contiguous()


class ResNetIBN(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(ResidualIBN, 64, 128, 2, stride=1)
        self.layer2 = self._make_layer(ResidualIBN, 128, 256, 2, stride=1)
        self.layer3 = self._make_layer(ResidualIBN, 256, 512, 2, stride=2)
        self.layer4 = self._make_layer(ResidualIBN, 512, 1024, 2, stride=2)
        self.global_pool = GeMPooling()
        self.embedding_head = nn.Linear(1024, 2048)

    def _make_layer(self, block, in_channels, out_channels, blocks, stride):
        layers = [block(in_channels, out_channels, stride)]
        layers += [block(out_channels, out_channels) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def forward_rows(self, x, stages=None):
        """x (B, 84, T) fp32 on the GPU -> h (B, 2048) fp32. stages: a dict that receives the stem / layer1..4 outputs as
        (rows, H, W) (tests)"""
        _require_eval_gpu(self, x, "ResNetIBN")
        if x.dim() != 3:
            raise ValueError(f"ResNetIBN takes (B, bins, frames) segments, got {tuple(x.shape)}")
        B = x.shape[0]
        w49, b49 = ops.packed_conv_bn(self.conv1.weight, *_bn_args(self.bn1))
        rows, H, W = ops.stem7_pool_fwd(x.float().contiguous(), w49, b49, F_.ACT_DTYPE)
        if stages is not None:
            stages["stem"] = (rows, H, W)
        for name in ("layer1", "layer2", "layer3", "layer4"):
            for blk in getattr(self, name):
                rows, H, W = blk.forward_rows(rows, B, H, W)
            if stages is not None:
                stages[name] = (rows, H, W)
        pooled = self.global_pool.pool_rows(rows, B, H * W)
        head = self.embedding_head
        h, _ = ops.linear_fwd(pooled, head.weight, head.bias, B, head.out_features, head.in_features)
        return h

    def head_train(self, rows, B, HW):
        """layer-4 rows (B*HW, 1024), fp32 or bf16 -> h (B, 2048), differentiable: backward fills the gradients of rows (fp32),
        global_pool.p, embedding_head.weight and embedding_head.bias (autograd rounds the gradient of bf16 rows to bf16; ops.gem_pool_bwd
        returns it in fp32). trunk_train puts the eight residual blocks in front of it."""
        if not rows.is_cuda:
            raise NotImplementedError("ResNetIBN.head_train: there is no CPU path; move the model and its input to the GPU")
        head = self.embedding_head
        if rows.dim() != 2 or tuple(rows.shape) != (B * HW, head.in_features):
            raise ValueError(f"head_train: expected rows ({B * HW}, {head.in_features}), got {tuple(rows.shape)}")
        return _HeadTrainFn.apply(rows, self.global_pool.p, head.weight, head.bias, B, HW, self.global_pool.eps)

    def trunk_train(self, rows, B, H, W):
        """the stem's output rows (B*H*W, 64), fp32 or bf16 -> h (B, 2048), differentiable, in training mode: the eight residual
        blocks (ResidualIBN.train_rows) and head_train. Backward fills the gradient of every parameter behind the stem and of rows."""
        for name in ("layer1", "layer2", "layer3", "layer4"):
            for blk in getattr(self, name):
                rows, H, W = blk.train_rows(rows, B, H, W)
        return self.head_train(rows, B, H * W)

    def stem_train(self, x):
        """x (B, 84, T) fp32 on the GPU -> (rows (B*Hp*Wp, 64) in ACT_DTYPE, Hp, Wp), differentiable, in training mode: bn1 normalises
        with the statistics of this batch and its running statistics and num_batches_tracked move as in nn.BatchNorm2d. Backward
        fills the gradients of conv1.weight, bn1.weight and bn1.bias."""
        if not x.is_cuda:
            raise NotImplementedError("ResNetIBN.stem_train: like the eval-mode forward, the training-mode forward has no CPU path; "
                                      "move the model and its input to the GPU")
        if x.dim() != 3:
            raise ValueError(f"ResNetIBN takes (B, bins, frames) segments, got {tuple(x.shape)}")
        bn = self.bn1
        if bn.momentum is None or not bn.track_running_stats or not bn.affine:
            raise NotImplementedError("training-mode BatchNorm on the MI355X path: affine, running statistics, a fixed momentum")
        H, W = x.shape[1], x.shape[2]
        rows = _StemTrainFn.apply(x.float().contiguous(), self.conv1.weight, bn.weight, bn.bias, bn, F_.ACT_DTYPE)
        return rows, ops.conv_out_size(ops.conv_out_size(H, 7, 2), 3, 2), ops.conv_out_size(ops.conv_out_size(W, 7, 2), 3, 2)

    def forward(self, x):
        if self.training:
            rows, H, W = self.stem_train(x)
            return self.trunk_train(rows, x.shape[0], H, W)
        return self.forward_rows(x)
