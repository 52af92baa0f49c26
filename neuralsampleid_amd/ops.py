"""Tensor-level wrappers over the C ABI (include/nsid.h): torch supplies device memory and the stream, nothing else.

Every function enqueues HIP kernels from libnsid_hip.so on torch's current stream; none falls back to ATen."""
import math
import os
from typing import Optional, Tuple

import numpy as np
import torch

from ._lib import DEFINES as _H        # the integer #defines of include/nsid.h: every kernel constant below is read from it
from ._lib import _ERR, call, get_tuning, launch_counters, lib, reset_tuning, set_tuning  # noqa: F401  (tuning, counters: re-exported)

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_ELU = _H["NSID_ACT_NONE"], _H["NSID_ACT_RELU"], _H["NSID_ACT_LEAKY"], _H["NSID_ACT_ELU"]
ROW_TILE = _H["NSID_ROW_TILE"]
BN_MOMENTUM = 0.1
BN_EPS = 1e-5


class KernelProfile:
    """Opt-in per-launch timing of the GEMM family with HIP events recorded on the launch stream (bench.py roofline).
    Keys follow the kernel template instantiation that the C side dispatches to: where an entry chooses between kernels the library
    itself names the one it took (include/nsid.h nsid_debug_last_kernel), nothing here restates a launch heuristic."""

    def __init__(self):
        self.records = []          # (kernel, flops, algorithmic bytes, start event, end event, shape)
        self.bracket_ms = self._empty_bracket_ms()

    @staticmethod
    def plug(ms: float = 120.0) -> None:
        """Keep the GPU busy for ~`ms` so that the host runs AHEAD of it: an eager step is host-bound (~7 us of Python / ctypes
        per launch), and an event pair around a launch on an idle GPU also measures the wait for the launch packet
        (a tiny kernel reads 12.4 us, a 19.4 us GEMM 27 us). Behind a plug the queue is full, kernels run back to back and an
        event pair brackets the kernel alone (the same GEMM reads 21.2 us: rocprofv3 says 20.6 us). Measurement aid only:
        never inside a timed region."""
        torch.cuda._sleep(int(ms * 1e-3 * 2.0e9))

    @staticmethod
    def _empty_bracket_ms(n: int = 64) -> float:
        """median elapsed time of an EMPTY event bracket on the current stream: two timed events cost a marker each, and
        that cost sits inside every per-launch measurement of an eager step; it is subtracted in summary()/by_shape()"""
        torch.cuda.synchronize()
        KernelProfile.plug(2.0)
        evs = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        ts = sorted(a.elapsed_time(b) for a, b in evs)
        return ts[len(ts) // 2]

    def _ms(self, e0, e1) -> float:
        return max(e0.elapsed_time(e1) - self.bracket_ms, 1e-4)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, flops, nbytes, e0, e1, shape in self.records:
            d = out.setdefault(name, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += self._ms(e0, e1)
            d["flops"] += flops
            d["bytes"] += nbytes
        return out

    def by_shape(self):
        """per (kernel, M, Nout, K, groups): launches, average us, TFLOP/s, algorithmic GB/s"""
        torch.cuda.synchronize()
        out = {}
        for name, flops, nbytes, e0, e1, shape in self.records:
            shape = tuple(shape)[:4] + (0,) * (4 - min(4, len(shape)))       # records without a GEMM shape: zeros
            d = out.setdefault((name,) + shape, [0, 0.0, flops, nbytes])
            d[0] += 1
            d[1] += self._ms(e0, e1)
        rows = []
        for key, (n, ms, flops, nbytes) in out.items():
            us = 1e3 * ms / n
            rows.append({"kernel": key[0], "M": key[1], "Nout": key[2], "K": key[3], "groups": key[4], "launches": n,
                         "avg_us": round(us, 1), "tflops": round(flops / us / 1e6, 1),
                         "alg_GBps": round(nbytes / us / 1e3, 0), "total_ms": round(ms, 3)})
        return sorted(rows, key=lambda r: -r["total_ms"])


PROFILE: Optional[KernelProfile] = None


def _timed(name, flops, nbytes, fn, shape=()):
    """name None: the entry picks its kernel in C, and the library says AFTER the launch which one it took (profiling only: an
    unprofiled step makes no extra call). fn returning False launched nothing: no record is kept (_try_fused)."""
    if PROFILE is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ran = fn()
    e1.record()
    if ran is not False:
        PROFILE.records.append((lib.nsid_debug_last_kernel().decode() if name is None else name, flops, nbytes, e0, e1, shape))
    return ran


def _try_fused(name, flops, nbytes, entry, args, shape=()) -> bool:
    """Time a library entry that may decline (include/nsid.h NSID_DECLINED). True: its fused form ran and is in the profile. False: it
    launched and wrote nothing, the profile has no record of it, and the caller runs the unfused sequence. Any other code raises, as
    call() does."""
    def launch():
        rc = getattr(lib, entry)(*args)
        if rc not in (_H["NSID_OK"], _H["NSID_DECLINED"]):
            raise RuntimeError(f"{entry} failed: {_ERR.get(rc, rc)}")
        return rc == _H["NSID_OK"]
    return _timed(name, flops, nbytes, launch, shape)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(*ts):
    """parameters / statistics / head tensors: contiguous fp32 on the GPU"""
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("neuralsampleid_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"expected contiguous float32, got {t.dtype} contiguous={t.is_contiguous()}")


F32, BF16 = _H["NSID_F32"], _H["NSID_BF16"]


def _tk(name, nbytes, fn, shape=()):
    """time a launch that moves bytes and does no matrix work (BatchNorm family, streaming passes, optimiser): bench.py's kernel table"""
    return _timed(name, 0.0, float(nbytes), fn, shape)


def _act(*ts) -> int:
    """activation tensors (features, raw conv outputs, their gradients): contiguous fp32 or bf16, all the same type;
    returns the C ABI dtype code"""
    code = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("neuralsampleid_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
        if t.dtype not in (torch.float32, torch.bfloat16) or not t.is_contiguous():
            raise RuntimeError(f"expected contiguous float32/bfloat16, got {t.dtype} contiguous={t.is_contiguous()}")
        c = BF16 if t.dtype == torch.bfloat16 else F32
        if code is not None and c != code:
            raise RuntimeError("activation tensors of one call must share a storage type")
        code = c
    return code


GEMM_FP32, GEMM_BF16 = _H["NSID_GEMM_FP32"], _H["NSID_GEMM_BF16"]


def set_gemm_precision(mode: str) -> None:
    """'fp32' (default; exact fp32 MFMA, the strict-parity path) or 'bf16' (operands rounded to bf16 as they are
    staged into LDS; fp32 storage in HBM, fp32 accumulation; 16x the matrix rate — BASELINE config 2's arithmetic)."""
    call("nsid_set_gemm_precision", {"fp32": GEMM_FP32, "bf16": GEMM_BF16}[mode])


def get_gemm_precision() -> str:
    return "bf16" if lib.nsid_get_gemm_precision() == GEMM_BF16 else "fp32"


def row_tiles(M: int) -> int:
    return (M + ROW_TILE - 1) // ROW_TILE


def w2d(w: torch.Tensor) -> torch.Tensor:
    """conv weight (Cout, Cin/g, 1, 1) or linear weight (Cout, Cin) viewed as a matrix (no copy)"""
    return w.reshape(w.shape[0], -1)


# ------------------------------------------------------------------------------------------------ state epoch
# Our kernels write parameters (nsid_adam_step) and BatchNorm running statistics (nsid_bn_finalize, nsid_bn_running_update)
# through raw pointers, and a hipGraph replay runs no Python at all: torch's `_version` counters do not see those writes.
# Every host-side entry that enqueues such a write bumps an epoch counter: WEIGHT_EPOCH for parameters
# (FusedClipAdam.step, GraphedTrainStep.__call__), STATS_EPOCH for running statistics (bn_finalize, bn_running_update,
# GraphedTrainStep.__call__). The caches below carry them in their keys — bf16 weight shadows: WEIGHT_EPOCH; eval-mode
# BatchNorm affines and folded conv+BN weights: both — so an eval after training steps never reuses constants of older
# weights or statistics.
WEIGHT_EPOCH = 0
STATS_EPOCH = 0


def bump_state_epoch(weights: bool = True, stats: bool = True) -> None:
    global WEIGHT_EPOCH, STATS_EPOCH
    if weights:
        WEIGHT_EPOCH += 1
    if stats:
        STATS_EPOCH += 1


# ------------------------------------------------------------------------------------------------ bf16 weight shadows
class WeightShadows:
    """bf16 copies of weight matrices for the bf16-storage GEMMs (forward / backward-data right operand): half the
    L2->LDS operand bytes and no convert pass in the kernel. Values are the RNE rounding the kernel applies to fp32
    weights anyway, so results are identical.

    Entries are keyed by the fp32 tensor's data pointer: [shadow, (version, WEIGHT_EPOCH)]. `FusedClipAdam` registers views
    of ONE flat shadow buffer, refreshes all of it at the start of every step and marks its entries fresh (`mark_fresh`);
    its update kernel bumps WEIGHT_EPOCH instead of torch's version counters, so a forward that runs after the last
    `step()` (eval, fingerprint extraction) re-converts the weights it reads. Torch-side in-place changes
    (load_state_dict, torch.optim) are caught by the version half of the key. Weights that are not registered are
    converted on the fly (one small launch per GEMM)."""

    def __init__(self):
        self.entries = {}

    def register(self, w: torch.Tensor, shadow: torch.Tensor, owner: torch.Tensor, fresh: bool = False) -> None:
        """`owner` keeps the fp32 memory alive (the optimiser's flat buffer): while it lives the address cannot be
        reused by another tensor; once it is gone the entry is dropped on its next lookup. fresh: `shadow` already holds
        the conversion of the current contents of w"""
        import weakref
        self.entries[w.data_ptr()] = [shadow, (w._version, WEIGHT_EPOCH) if fresh else None, w.numel(), weakref.ref(owner)]

    def mark_fresh(self, w: torch.Tensor) -> None:
        """the registered shadow of `w` has just been refreshed by its owner (FusedClipAdam.sync_shadow)"""
        e = self.entries.get(w.data_ptr())
        if e is not None:
            e[1] = (w._version, WEIGHT_EPOCH)

    def clear(self) -> None:
        self.entries.clear()

    def purge(self) -> int:
        """drop the entries whose fp32 memory is gone (their shadows would otherwise stay alive with the registry)"""
        dead = [k for k, e in self.entries.items() if e[3]() is None]
        for k in dead:
            del self.entries[k]
        return len(dead)

    def operand(self, w: torch.Tensor) -> torch.Tensor:
        e = self.entries.get(w.data_ptr())
        if e is not None and e[3]() is None:
            del self.entries[w.data_ptr()]
            e = None
        if e is None or e[2] != w.numel():
            return f32_to_bf16(w)
        key = (w._version, WEIGHT_EPOCH)
        if e[1] != key:
            f32_to_bf16(w, e[0])
            e[1] = key
        return e[0]


SHADOWS = WeightShadows()


def register_weight_shadows(module) -> int:
    """Give every not-yet-registered GEMM weight of `module` a persistent bf16 shadow (inference: no optimiser keeps one).
    Shadows follow torch-side weight changes through the version check. Returns the number of new shadows."""
    n = 0
    for p in module.parameters():
        if p.is_cuda and p.dim() >= 2 and p.numel() % 8 == 0 and p.data_ptr() not in SHADOWS.entries:
            SHADOWS.register(p.data, torch.empty(p.numel(), device=p.device, dtype=torch.bfloat16), owner=p)
            n += 1
    return n


def f32_to_bf16(src: torch.Tensor, dst: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(src)
    n = src.numel()
    if dst is None:
        dst = torch.empty(((n + 7) // 8 * 8,), device=src.device, dtype=torch.bfloat16)
    if n % 8:            # tiny odd-sized matrices: let torch round (same RNE)
        dst[:n].copy_(src.reshape(-1))
        return dst
    _tk("f32_to_bf16_kernel", 6.0 * n, lambda: call("nsid_f32_to_bf16", _p(src), _p(dst), n, _stream()), (n, 1, 0, 1))
    return dst


def _weight(w: torch.Tensor, dt: int, K: int):
    """(pointer-holder tensor, C ABI dtype code) of a GEMM's weight operand"""
    if dt == BF16 and K % 8 == 0 and w.numel() % 8 == 0:
        return SHADOWS.operand(w), BF16
    return w, F32


# ------------------------------------------------------------------------------------------------ linear
def linear_fwd(x, w, bias, M, Nout, K, groups=1, in_scale=None, in_shift=None, act_in=ACT_NONE, act_out=ACT_NONE,
               want_stat=False, ksplit=1, out=None, addend=None, in_aff=None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """out = f(x) w^T + bias (+ addend, same layout and storage as out: the residual stream, nsid_linear_fwd_res).
    in_aff: the producer's BNAffine instead of (in_scale, in_shift)."""
    if in_aff is not None:
        in_scale, in_shift = in_aff.scale, in_aff.shift
    _chk(w, bias, in_scale, in_shift)
    dt = _act(x, out, addend)
    if addend is not None and (want_stat or ksplit != 1 or act_out != ACT_NONE):
        raise ValueError("the residual addend rides with a plain epilogue (no statistics, no split-K, no output activation)")
    ldx = x.shape[-1]
    if out is None:
        out = torch.empty((M, groups * Nout), device=x.device, dtype=x.dtype)
        if ksplit > 1:
            fill_zero(out)
    stat = torch.empty((2, row_tiles(M), groups * Nout), device=x.device, dtype=torch.float32) if want_stat else None
    esz = x.element_size()
    wop, wdt = _weight(w, dt, K)
    if in_scale is None and act_in != ACT_NONE:
        # activation on load without an affine: only ReLU on bf16 operands, bf16 weights and whole tiles (csrc/gemm.hip ARELU). The tile
        # width is the library's choice: this check covers the narrowest tile, and the library answers NSID_EINVAL for a wider one
        # that the shape does not fill.
        if not (act_in == ACT_RELU and dt == BF16 and wdt == BF16 and M % 128 == 0 and Nout % 64 == 0 and K % 64 == 0
                and ksplit == 1):
            raise ValueError("activation-on-load without an affine needs ReLU, bf16 storage, bf16 weights and whole tiles")
    if addend is not None:
        _timed(None, 2.0 * M * Nout * K * groups,
               groups * (esz * M * K + float(wop.element_size()) * Nout * K + 2 * esz * M * Nout), lambda: call(
            "nsid_linear_fwd_res", _p(x), ldx, _p(wop), wdt, _p(bias), _p(addend), addend.shape[-1], _p(out),
            out.shape[-1], M, Nout, K, groups, _p(in_scale), _p(in_shift), act_in, dt, _stream()), (M, Nout, K, groups))
        return out, None
    _timed(None, 2.0 * M * Nout * K * groups,
           groups * (esz * M * K + float(wop.element_size()) * Nout * K + esz * M * Nout), lambda: call(
        "nsid_linear_fwd", _p(x), ldx, _p(wop), wdt, _p(bias), _p(out), out.shape[-1], M, Nout, K, groups, _p(in_scale),
        _p(in_shift), act_in, act_out, _p(stat), ksplit, dt, _stream()), (M, Nout, K, groups))
    return out, stat


FUSE_EVAL_FFN = True          # eval-mode FFN (BatchNorms folded) as one launch for the C = 64 / 128 stages (csrc/ffn_fused.hip)


def ffn_fused_fwd(x, w1f, b1f, w2f, b2f, M, C, H):
    """out = x + w2f relu(w1f x + b1f) + b2f in one launch (folded eval-mode FFN); None when the shape is outside the fused form"""
    _chk(w1f, b1f, w2f, b2f)
    if _act(x) != BF16 or x.shape != (M, C) or not FUSE_EVAL_FFN:
        return None
    w1, d1 = _weight(w1f, BF16, C)
    w2, d2 = _weight(w2f, BF16, H)
    if d1 != BF16 or d2 != BF16:
        return None
    out = torch.empty_like(x)
    ran = _try_fused("ffn_fused_kernel", 4.0 * M * C * H, 2.0 * x.element_size() * M * C + 4.0 * C * H, "nsid_ffn_fused_fwd",
                     (_p(x), _p(w1), _p(b1f), _p(w2), _p(b2f), _p(out), M, C, H, _stream()), (M, C, H, 1))
    return out if ran else None


FUSE_EVAL_MRCONV = True       # eval-mode max-relative aggregation + grouped conv as one launch (csrc/mrconv_fused.hip)


def mrconv_fused_fwd(y, idx, B, N, C, wf, bf):
    """relu(grouped conv([y, max-relative(y)]) + b) with the BatchNorm folded into (wf, bf), one workgroup per clip; the interleaved
    (B*N, 2C) tensor is never formed. None when the shape is outside the fused form."""
    _chk(wf, bf)
    if not FUSE_EVAL_MRCONV or _act(y) != BF16 or y.shape != (B * N, C) or idx.dtype != torch.int32 or not idx.is_contiguous():
        return None
    w, dw = _weight(wf, BF16, C // 2)
    if dw != BF16:
        return None
    k = idx.shape[-1]
    out = torch.empty((B * N, 2 * C), device=y.device, dtype=y.dtype)
    ran = _try_fused("mrconv_fused_kernel", 2.0 * B * N * (C // 2) * (C // 2) * 4, float(B) * N * (3 * C * y.element_size() + k * 4),
                     "nsid_mrconv_fused_fwd", (_p(y), _p(idx), B, N, C, k, _p(w), _p(bf), _p(out), _stream()),
                     (B * N, C // 2, C // 2, 4))
    return out if ran else None


FUSE_BN_BWD_REDUCE = True     # backward-data GEMMs emit the next BatchNorm-backward's column sums (bf16 storage only)


def linear_bwd_data(dout, w, M, Nout, K, groups=1, addend=None, out=None, bn=None):
    """din = addend + dout @ w.  bn = (r, BNAffine, act): din is dL/dy of the layer y = act(BN(r)); then the call returns
    (din, partial) with partial[2][tiles][groups*K] = that layer's backward column sums (see bn_backward(partial=...))."""
    _chk(w)
    dt = _act(dout, addend, out)
    if out is None:
        out = torch.empty((M, groups * K), device=dout.device, dtype=dout.dtype)
    esz = dout.element_size()
    wop, wdt = _weight(w, dt, K)
    want_pair = bn is not None            # bn=False: "return a pair, nothing to fuse"
    bn = bn or None
    fuse = bn is not None and FUSE_BN_BWD_REDUCE and dt == BF16 and out.shape[-1] == groups * K and (groups * K) % 8 == 0
    if fuse and tuple(bn[0].shape) != (M, groups * K):
        fuse = False
    nbytes = groups * (esz * M * Nout + float(wop.element_size()) * Nout * K
                       + esz * M * K * ((2 if addend is not None else 1) + (1 if fuse else 0)))
    if fuse:
        r, aff, act = bn
        _act(r, out)
        partial = torch.empty((2, row_tiles(M), groups * K), device=dout.device, dtype=torch.float32)
        _timed(None, 2.0 * M * Nout * K * groups, nbytes, lambda: call(
            "nsid_linear_bwd_data_bn", _p(dout), dout.shape[-1], _p(wop), wdt, _p(addend),
            0 if addend is None else addend.shape[-1], _p(out), out.shape[-1], M, Nout, K, groups, dt, _p(r),
            _p(aff.scale), _p(aff.shift), _p(aff.mean), _p(aff.invstd), act, _p(partial), _stream()),
            (M, Nout, K, groups))
        return out, partial
    _timed(None, 2.0 * M * Nout * K * groups, nbytes, lambda: call(
        "nsid_linear_bwd_data", _p(dout), dout.shape[-1], _p(wop), wdt, _p(addend),
        0 if addend is None else addend.shape[-1], _p(out), out.shape[-1], M, Nout, K, groups, dt, _stream()),
        (M, Nout, K, groups))
    return (out, None) if want_pair else out


# BatchNorm-backward apply evaluated on the operand load of the backward-data GEMM (bf16 storage): bit mask over the call sites
# (1: FFN hidden layer, 2: grouped conv, 4: Grapher fc1); True = all, False / 0 = none
FUSE_BN_BWD_APPLY = 4        # measured in the two-stream step (round 3, one-box A/B x2): none 8.09 / 8.06 ms, FFN 8.35 / 8.35, grouped 8.14 / 8.13, fc1 8.08 / 8.09, all 8.33 / 8.32
SITE_FFN, SITE_GCONV, SITE_FC1, SITE_FC2, SITE_FFN2 = 1, 2, 4, 8, 16
# On the layers of csrc/wsgemm.hip (nsid_ws_layer) the fused operand load costs one evaluation per ROW (a workgroup owns all output
# columns), not one per column tile, so every call site takes it (tuning key ws_gemm bit 2); elsewhere FUSE_BN_BWD_APPLY decides


def bn_backward_linear_bwd_data(dy, r, aff: "BNAffine", act, dgamma, dbeta, partial, w, M, Nout, K, groups=1, addend=None,
                                bn=None, site=SITE_FFN, inplace=True):
    """BatchNorm(+act) backward of a conv+BN layer FOLLOWED by that conv's backward-data GEMM, the two fused where the shape allows:
        dr  = BN-backward(dy, r)        (dy = dL/d act(BN(r)); dgamma / dbeta accumulated)
        din = addend + dr @ w           (+ the column sums for the next BatchNorm backward when bn=(r', aff', act'))
    Returns (dr, din, partial_out). Fused form (csrc/gemm.hip ABN): the GEMM evaluates dr on its operand load from dy and r and
    writes it once for the weight gradient — no bn_bwd_apply pass. `partial` = this layer's column sums (from the GEMM that wrote dy,
    or None: a reduce launch). Falls back to bn_backward + linear_bwd_data (same results up to one fp32 rounding before the bf16
    store) for fp32 storage and shapes outside the fused form. inplace: the unfused fallback may overwrite dy with dr (False where the
    caller still needs dy: the residual-stream gradients dx1 / dx2 are also the addends of a later GEMM)."""
    dt = _act(dy, r, addend)
    C = r.shape[1]
    tiles = row_tiles(M)
    s = _stream()
    wop, wdt = _weight(w, dt, K)
    enabled = FUSE_BN_BWD_APPLY is True or (FUSE_BN_BWD_APPLY and (int(FUSE_BN_BWD_APPLY) & site))
    ws_form = (dt == BF16 and wdt == BF16 and M % 128 == 0 and lib.nsid_ws_layer(K, Nout, groups) == 1 and (get_tuning("ws_gemm") & 4) != 0)
    enabled = enabled or ws_form
    fusable = (enabled and dt == BF16 and wdt == BF16 and tuple(r.shape) == (M, groups * Nout) and
               tuple(dy.shape) == (M, groups * Nout) and M % 128 == 0 and
               (ws_form or (Nout % 64 == 0 and K % 64 == 0 and (K <= 64 or K % 128 == 0))))
    if not fusable:
        dr = bn_backward(dy, r, aff, act, dgamma, dbeta, inplace=inplace, partial=partial)
        return (dr,) + linear_bwd_data(dr, w, M, Nout, K, groups, addend=addend, bn=bn if bn is not None else False)
    if partial is None:
        partial = torch.empty((2, tiles, C), device=r.device, dtype=torch.float32)
        part_ = partial
        _tk("col_reduce_kernel", 2.0 * r.element_size() * M * C, lambda: call(
            "nsid_bn_bwd_reduce", _p(dy), _p(r), M, C, _p(aff.scale), _p(aff.shift), _p(aff.mean), _p(aff.invstd), act, _p(part_),
            dt, s), (M, C, 0, 1))
    ptiles = partial.shape[1]                  # rows of THIS layer's partial sums (row tiles, or one per clip from mr_aggregate_bwd)
    coef = torch.empty((6, C), device=r.device, dtype=torch.float32)        # [0:2] = (c0, c1) for the unfused apply, [2:6] = coef4
    if not (DIAG_SKIP_FINALIZE & 2):
        _tk("bn_bwd_finalize_kernel", 8.0 * ptiles * C + 40.0 * C, lambda: call(
            "nsid_bn_bwd_finalize_fused", _p(partial), ptiles, C, M, _p(dgamma), _p(dbeta), _p(coef), _p(aff.scale), _p(aff.shift),
            _p(aff.mean), _p(aff.invstd), _p(coef[2]), s), (M, C, 0, 1))
    dr = torch.empty_like(dy)
    din = torch.empty((M, groups * K), device=dy.device, dtype=dy.dtype)
    want_pair = bn is not None
    bn = bn or None
    fuse_sums = bn is not None and FUSE_BN_BWD_REDUCE and (groups * K) % 8 == 0 and tuple(bn[0].shape) == (M, groups * K)
    part_out = torch.empty((2, tiles, groups * K), device=dy.device, dtype=torch.float32) if fuse_sums else None
    br, baff, bact = bn if fuse_sums else (None, None, ACT_NONE)
    esz = dy.element_size()
    nbytes = groups * (3 * esz * M * Nout + float(wop.element_size()) * Nout * K
                       + esz * M * K * ((2 if addend is not None else 1) + (1 if fuse_sums else 0)))
    ran = _try_fused(None, 2.0 * M * Nout * K * groups, nbytes, "nsid_linear_bwd_data_bnapply", (
        _p(dy), _p(r), _p(coef[2]), act, _p(dr), _p(wop), wdt, _p(addend), 0 if addend is None else addend.shape[-1], _p(din),
        din.shape[-1], M, Nout, K, groups, dt, _p(br), _p(baff.scale) if baff else None, _p(baff.shift) if baff else None,
        _p(baff.mean) if baff else None, _p(baff.invstd) if baff else None, bact, _p(part_out), s), (M, Nout, K, groups))
    if not ran:                # outside the fused form after all: apply with the coefficients already computed, then the plain GEMM
        call("nsid_bn_bwd_apply", _p(dy), _p(r), M, C, _p(aff.scale), _p(aff.shift), _p(aff.mean), _p(aff.invstd), act, _p(coef),
             _p(dr), dt, s)
        res = linear_bwd_data(dr, w, M, Nout, K, groups, addend=addend, out=din, bn=bn if bn is not None else False)
        return (dr,) + res
    return dr, din, part_out


def linear_bwd_weight(dout, x, dw, M, Nout, K, groups=1, in_scale=None, in_shift=None, act_in=ACT_NONE) -> None:
    """dw += dout^T f(x)"""
    _chk(dw, in_scale, in_shift)
    dt = _act(dout, x)
    esz = x.element_size()
    _timed(None, 2.0 * M * Nout * K * groups, groups * (esz * M * Nout + esz * M * K + 4.0 * Nout * K), lambda: call(
        "nsid_linear_bwd_weight", _p(dout), dout.shape[-1], _p(x), x.shape[-1], _p(dw), M, Nout, K, groups,
        _p(in_scale), _p(in_shift), act_in, dt, _stream()), (M, Nout, K, groups))


WGRAD_GROUPED = 1        # 0: the deferred phase issues one nsid_linear_bwd_weight per recorded problem (the gate of round 6: 8.68 ms)


def wgrad_item(it) -> None:
    """one recorded weight-gradient problem through the per-layer launch (the grouped phase's fallback and its test reference)"""
    extra = it[10] if len(it) > 10 else None
    if extra is None:
        linear_bwd_weight(*it[:10])
    else:                                      # ("ds", B, N, C): the packed gradient of a Downsample (unpacked by the caller)
        _, B, N, C = extra[:4]
        downsample3_bwd_weight(it[0], it[1], it[2], B, N, C, it[4])


def linear_bwd_weight_batch(items, max_workgroups: int = 0) -> None:
    """the deferred weight-gradient phase (functional.DeferredWgrads): items = [(dout, x, dw, M, Nout, K, groups, in_scale, in_shift,
    act_in[, extra])] in backward order, both views of a layer sharing the same dw. dw += dout^T f(x) for every item.
    extra = ("ds", B, N, C, weight_grad): a Downsample — x is its input, dw its packed gradient, unpacked into weight_grad afterwards.
    ONE call of nsid_linear_bwd_weight_grouped per storage type: the items that share dw and shape become the two row segments of one
    problem, the problems of all layers one launch per tile class (csrc/gemm.hip wgrad_grouped_kernel).
    max_workgroups > 0: a launch that runs beside the backward chains (at most that many workgroups, each walking several items)."""
    if not items:
        return
    from ._lib import WgradProblem
    import ctypes
    unpack = {}
    for it in items:
        if len(it) > 10 and it[10] is not None:
            unpack[it[2].data_ptr()] = (it[2], it[10][4])
    if not WGRAD_GROUPED:
        for it in items:
            wgrad_item(it)
    else:
        for dtype, code in ((torch.bfloat16, BF16), (torch.float32, F32)):
            probs, open_ = [], {}           # open_: (dw pointer, shape) -> a problem that still has a free second segment
            flops = nbytes = 0.0
            n_items = 0
            for it in items:
                dout, x, dw, M, Nout, K, groups, in_scale, in_shift, act_in = it[:10]
                if dout.dtype != dtype:
                    continue
                extra = it[10] if len(it) > 10 else None
                _chk(dw, in_scale, in_shift)
                if _act(dout, x) != code:
                    raise RuntimeError("a weight-gradient problem with mixed storage types")
                n_items += 1
                flops += 2.0 * M * Nout * K * groups
                nbytes += groups * float(dout.element_size()) * M * (Nout + K)
                ldx = x.shape[-1]
                key = (dw.data_ptr(), M, Nout, K, groups, dout.shape[-1], ldx, act_in, in_scale is None, extra is None)
                q = open_.pop(key, None)
                if q is None:
                    q = WgradProblem()
                    q.dout[0], q.x[0], q.in_scale[0], q.in_shift[0] = _p(dout), _p(x), _p(in_scale), _p(in_shift)
                    q.dw, q.ldd, q.ldx, q.M, q.Nout, q.K, q.groups, q.act_in = _p(dw), dout.shape[-1], ldx, M, Nout, K, groups, act_in
                    q.ds_out_nodes = 0 if extra is None else extra[2] // 2
                    probs.append(q)
                    open_[key] = q
                    nbytes += 4.0 * groups * Nout * K
                else:
                    q.dout[1], q.x[1], q.in_scale[1], q.in_shift[1] = _p(dout), _p(x), _p(in_scale), _p(in_shift)
            if not probs:
                continue
            arr = (WgradProblem * len(probs))(*probs)
            _timed("wgrad_grouped_kernel", flops, nbytes, lambda: call(
                "nsid_linear_bwd_weight_grouped", ctypes.addressof(arr), len(probs), code, int(max_workgroups), _stream()),
                (n_items, len(probs), 0, 1))
    for dwp, wgrad in unpack.values():
        unpack_ds_wgrad(dwp, wgrad)


def colsum_acc(x, out) -> None:
    _chk(out)
    _tk("colsum_atomic_kernel", float(x.element_size()) * x.numel(), lambda: call(
        "nsid_colsum_acc", _p(x), x.shape[-1], x.shape[0], x.shape[1], _p(out), _act(x), _stream()), (x.shape[0], x.shape[1], 0, 1))


# ------------------------------------------------------------------------------------------------ batch norm
class BNAffine:
    """What a consumer needs to apply a producer's BatchNorm on load, plus what backward needs.
    identity: scale == 1, shift == 0 (an eval-mode BatchNorm folded into its conv): consumers that only normalise skip it,
    consumers that also apply an activation on load use the ones/zeros vectors."""
    __slots__ = ("scale", "shift", "mean", "invstd", "identity")

    def __init__(self, scale, shift, mean=None, invstd=None, identity=False):
        self.scale, self.shift, self.mean, self.invstd, self.identity = scale, shift, mean, invstd, identity


_IDENTITY_AFFINE = {}


def identity_affine(C: int, device) -> BNAffine:
    key = (C, str(device))
    a = _IDENTITY_AFFINE.get(key)
    if a is None:
        a = _IDENTITY_AFFINE[key] = BNAffine(torch.ones(C, device=device), torch.zeros(C, device=device), identity=True)
    return a


# eval-mode BatchNorm folded into the preceding conv: BN(W x + b) = (s W) x + (s b + beta - mean s), s = gamma/sqrt(var+eps).
# Constants of the checkpoint: computed once per layer (torch ops, off the hot path), bf16 shadow included, and kept until a
# version counter of one of the six tensors moves.
_FOLDED = {}      # id(gamma) -> (weakref(gamma), versions, w_fold, b_fold)


def folded_conv_bn(w2d, bias, gamma, beta, running_mean, running_var, eps=BN_EPS, source=None):
    """w2d: (Nout_total, K) weight matrix, or a callable that builds it from `source` (the downsample's packed weight);
    `source` is the tensor whose version counter stands for the weight (default: w2d itself)."""
    import weakref
    src = w2d if source is None else source
    versions = (src.data_ptr(), src._version, None if bias is None else (bias.data_ptr(), bias._version), gamma._version,
                beta._version, running_mean._version, running_var._version, eps, WEIGHT_EPOCH, STATS_EPOCH)
    # under stream capture nothing is INSERTED (the constants would be produced by captured work), but an entry made
    # before the capture is used: the replayed kernels then read the cached constants in place (GraphedFingerprinter)
    cacheable = not torch.cuda.is_current_stream_capturing()
    e = _FOLDED.get(id(gamma))
    if e is not None and e[0]() is gamma and e[1] == versions:
        return e[2], e[3]
    with torch.no_grad():
        if callable(w2d):
            w2d = w2d()
        s = gamma.detach() / torch.sqrt(running_var + eps)
        w_fold = (w2d.detach() * s[:, None]).contiguous()
        b_fold = (beta.detach() - running_mean * s) if bias is None else (bias.detach() * s + beta.detach() - running_mean * s)
        b_fold = b_fold.contiguous()
        if w_fold.numel() % 8 == 0:
            SHADOWS.register(w_fold, f32_to_bf16(w_fold), owner=w_fold, fresh=True)
    if cacheable:
        _cache_constants(_FOLDED, id(gamma), (weakref.ref(gamma), versions, w_fold, b_fold))
    return w_fold, b_fold


def _cache_constants(cache, key, entry) -> None:
    """keep constants derived from a parameter (entry[0]: a weakref to it) in one of the version-keyed caches: synchronise once, so
    that they are valid on every stream, and drop the entries of dead models when the cache has grown"""
    torch.cuda.current_stream().synchronize()
    if len(cache) > 4096:
        for k in [k for k, v in cache.items() if v[0]() is None]:
            del cache[k]
    cache[key] = entry


def bn_finalize(stat, M, gamma, beta, running_mean, running_var, num_batches_tracked,
                momentum=BN_MOMENTUM, eps=BN_EPS, tiles=None) -> BNAffine:
    """tiles: the number of partial sums per channel in stat (2, tiles, C); None: row_tiles(M), the layout of the GEMM epilogues and
    of col_stat (stem7_stat leaves another count)"""
    C = gamma.numel()
    tiles = row_tiles(M) if tiles is None else int(tiles)
    buf = torch.empty((4, C), device=gamma.device, dtype=torch.float32)
    if running_mean is not None:
        bump_state_epoch(weights=False)
    _tk("bn_finalize_kernel", 8.0 * tiles * C + 16.0 * C, lambda: call(
        "nsid_bn_finalize", _p(stat), tiles, C, M, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
        _p(num_batches_tracked), momentum, eps, _p(buf[0]), _p(buf[1]), _p(buf[2]), _p(buf[3]), _stream()), (M, C, 0, 1))
    return BNAffine(buf[0], buf[1], buf[2], buf[3])


# Diagnosis only (results wrong, timing valid): bit 0 skips the forward finalize launches, bit 1 the backward ones — the ceiling of
# what moving the finalize arithmetic into neighbouring kernels can buy (bench.py --flag ops.DIAG_SKIP_FINALIZE=3).
DIAG_SKIP_FINALIZE = 0
_DIAG_CONST = {}


def _diag_const(C, device):
    key = (C, str(device))
    if key not in _DIAG_CONST:
        _DIAG_CONST[key] = (torch.ones(C, device=device), torch.zeros(C, device=device), torch.zeros((2, C), device=device))
    return _DIAG_CONST[key]


def bn_finalize_deferred(stat, M, gamma, beta, eps=BN_EPS):
    """training-mode statistics -> (BNAffine, unbiased variance) WITHOUT updating the running statistics (bn_running_update)"""
    C = gamma.numel()
    if DIAG_SKIP_FINALIZE & 1:
        one, zero, _ = _diag_const(C, gamma.device)
        return BNAffine(one, zero, zero, one), one
    buf = torch.empty((5, C), device=gamma.device, dtype=torch.float32)
    _tk("bn_finalize_kernel", 8.0 * row_tiles(M) * C + 20.0 * C, lambda: call(
        "nsid_bn_finalize_deferred", _p(stat), row_tiles(M), C, M, _p(gamma), _p(beta), eps, _p(buf[0]), _p(buf[1]),
        _p(buf[2]), _p(buf[3]), _p(buf[4]), _stream()), (M, C, 0, 1))
    return BNAffine(buf[0], buf[1], buf[2], buf[3]), buf[4]


def bn_running_update(layers_a, layers_b=None, momentum=BN_MOMENTUM) -> None:
    """Deferred running-statistics updates of many BatchNorm layers in one launch per 16 layers.
    layers_a: [(running_mean, running_var, num_batches_tracked or None, mean, uvar)] of the first view, in layer order;
    layers_b: the same layers for the second view (its mean / uvar are applied after the first view's), or None."""
    import ctypes
    n = len(layers_a)
    if n == 0:
        return
    if layers_b is not None and len(layers_b) != n:
        raise ValueError("both views must have run the same BatchNorm layers")
    bump_state_epoch(weights=False)
    arr = lambda vals: (ctypes.c_void_p * n)(*[None if v is None else v.data_ptr() for v in vals])
    Cs = (ctypes.c_int * n)(*[la[0].numel() for la in layers_a])
    for la in layers_a:
        _chk(la[0], la[1], la[3], la[4])
    if layers_b is not None:
        for la, lb in zip(layers_a, layers_b):
            if la[0].data_ptr() != lb[0].data_ptr():
                raise ValueError("the two views disagree on the layer order")
            _chk(lb[3], lb[4])
    call("nsid_bn_running_update", n, Cs, arr([la[0] for la in layers_a]), arr([la[1] for la in layers_a]),
         arr([la[2] for la in layers_a]), arr([la[3] for la in layers_a]), arr([la[4] for la in layers_a]),
         None if layers_b is None else arr([lb[3] for lb in layers_b]),
         None if layers_b is None else arr([lb[4] for lb in layers_b]), momentum, _stream())


# eval-mode BatchNorm affines are constants of the checkpoint: computed once per layer and kept until one of the four tensors
# changes (torch version counters) — fingerprinting spent 6 % of its GPU time recomputing 64 of them per micro-batch.
_EVAL_AFFINE = {}     # id(gamma) -> (weakref(gamma), versions, eps, BNAffine, stream handle, event)


def bn_eval_affine(gamma, beta, running_mean, running_var, eps=BN_EPS) -> BNAffine:
    import weakref
    versions = (gamma._version, beta._version, running_mean._version, running_var._version,
                beta.data_ptr(), running_mean.data_ptr(), running_var.data_ptr(), WEIGHT_EPOCH, STATS_EPOCH)
    cacheable = not torch.cuda.is_current_stream_capturing()
    e = _EVAL_AFFINE.get(id(gamma))
    if e is not None and e[0]() is gamma and e[1] == versions and e[2] == eps:
        if e[4] != _stream() and cacheable:
            torch.cuda.current_stream().wait_event(e[5])      # produced on another stream (a capture starts after a full
        return e[3]                                           # device synchronisation: nothing to wait for there)
    C = gamma.numel()
    buf = torch.empty((2, C), device=gamma.device, dtype=torch.float32)
    call("nsid_bn_eval_affine", _p(gamma), _p(beta), _p(running_mean), _p(running_var), eps, C, _p(buf[0]),
         _p(buf[1]), _stream())
    aff = BNAffine(buf[0], buf[1])
    if cacheable:
        ev = torch.cuda.Event()
        ev.record()
        if len(_EVAL_AFFINE) > 4096:          # entries of dead models
            for k in [k for k, v in _EVAL_AFFINE.items() if v[0]() is None]:
                del _EVAL_AFFINE[k]
        _EVAL_AFFINE[id(gamma)] = (weakref.ref(gamma), versions, eps, aff, _stream(), ev)
    return aff


def bn_apply(r, aff: BNAffine, act=ACT_NONE, residual=None, out=None) -> torch.Tensor:
    dt = _act(r, residual, out)
    M, C = r.shape
    if out is None:
        out = torch.empty_like(r)
    _tk("bn_apply_kernel", r.element_size() * M * C * (3 if residual is not None else 2), lambda: call(
        "nsid_bn_apply", _p(r), _p(aff.scale), _p(aff.shift), act, _p(residual), _p(out), M, C, dt, _stream()), (M, C, 0, 1))
    return out


def bn_backward(dout, r, aff: BNAffine, act, dgamma, dbeta, inplace=False, partial=None) -> torch.Tensor:
    """Gradient w.r.t. the raw conv output r of y = act(BN(r)), given dL/dy; dgamma/dbeta are accumulated.
    partial: the column sums already produced by the GEMM that wrote dout (linear_bwd_data(bn=...)): skips the reduce."""
    dt = _act(dout, r)
    M, C = r.shape
    tiles = row_tiles(M) if partial is None else partial.shape[1]      # rows of partial sums (one per clip from mr_aggregate_bwd)
    s = _stream()
    coef = torch.empty((2, C), device=r.device, dtype=torch.float32)
    if partial is None:
        partial = torch.empty((2, tiles, C), device=r.device, dtype=torch.float32)
        part_ = partial
        _tk("col_reduce_kernel", 2.0 * r.element_size() * M * C, lambda: call(
            "nsid_bn_bwd_reduce", _p(dout), _p(r), M, C, _p(aff.scale), _p(aff.shift), _p(aff.mean), _p(aff.invstd),
            act, _p(part_), dt, s), (M, C, 0, 1))
    if DIAG_SKIP_FINALIZE & 2:
        coef = _diag_const(C, r.device)[2]
    else:
        _tk("bn_bwd_finalize_kernel", 8.0 * tiles * C + 16.0 * C, lambda: call(
            "nsid_bn_bwd_finalize", _p(partial), tiles, C, M, _p(dgamma), _p(dbeta), _p(coef), s), (M, C, 0, 1))
    dr = dout if inplace else torch.empty_like(dout)
    _tk("bn_bwd_apply_kernel", 3.0 * r.element_size() * M * C, lambda: call(
        "nsid_bn_bwd_apply", _p(dout), _p(r), M, C, _p(aff.scale), _p(aff.shift), _p(aff.mean), _p(aff.invstd),
        act, _p(coef), _p(dr), dt, s), (M, C, 0, 1))
    return dr


# ------------------------------------------------------------------------------------------------ graph ops
def knn_graph(r, B, N, C, k, dilation=1, aff: Optional[BNAffine] = None) -> torch.Tensor:
    """(B*N, C) features (optionally with a pending BatchNorm affine) -> int32 (B, N, k) clip-local neighbour ids"""
    dt = _act(r)
    if aff is not None and aff.identity:
        aff = None
    idx = torch.empty((B, N, k), device=r.device, dtype=torch.int32)
    # read the features once, write int32 ids; 2*N^2*C flop on the fp32 matrix pipe (knn2_raw_kernel: one bf16 MFMA pass,
    # executed flops = algorithmic)
    _timed(None, 2.0 * B * N * N * C, float(B) * (N * C * r.element_size() + N * k * 4), lambda: call(
        "nsid_knn_graph", _p(r), r.shape[-1], _p(aff.scale) if aff else None, _p(aff.shift) if aff else None,
        B, N, C, k, dilation, _p(idx), dt, _stream()), (B * N, N, C, 1))
    return idx


def mr_aggregate_fwd(r, idx, B, N, C, aff: Optional[BNAffine] = None, want_argmax=True):
    dt = _act(r)
    if aff is not None and aff.identity:
        aff = None
    k = idx.shape[-1]
    u = torch.empty((B * N, 2 * C), device=r.device, dtype=r.dtype)
    amax = torch.empty((B * N, C), device=r.device, dtype=torch.uint8) if want_argmax else None
    # read x once, write the interleaved (x, max-relative) pair, read idx (+ the arg-max bytes for backward)
    nbytes = float(B) * N * (3 * C * r.element_size() + k * 4 + (C if want_argmax else 0))
    _timed("mr_fwd_kernel", 0.0, nbytes, lambda: call(
        "nsid_mr_aggregate_fwd", _p(r), r.shape[-1], _p(aff.scale) if aff else None,
        _p(aff.shift) if aff else None, _p(idx), B, N, C, k, _p(u), _p(amax), dt, _stream()), (B * N, 2 * C, C, 1))
    return u, amax


FUSE_MR_BWD_SUMS = True      # the aggregation backward also emits the backward column sums of the BatchNorm in front of it (no reduce launch)


def mr_aggregate_bwd(du, idx, amax, B, N, C, bn=None):
    """dL/dy of the max-relative aggregation. bn = (r, aff, act): y was act(BN(r)) of a conv+BN layer (Grapher fc1); where the
    degree-ranked kernel serves the launch the call returns (dy, partial) with partial[2][B][C] = that BatchNorm's backward column
    sums per clip (bn_backward(partial=...) / bn_backward_linear_bwd_data(partial=...)), else (dy, None)."""
    dt = _act(du)
    k = idx.shape[-1]
    dy = torch.empty((B * N, C), device=du.device, dtype=du.dtype)
    nbytes = float(B) * N * (3 * C * du.element_size() + k * 4 + C)
    if bn is not None and FUSE_MR_BWD_SUMS and dt == BF16:
        # whether the degree-ranked kernel serves the shape is csrc/mr.hip's rule (mrs_launch): a declined call launches nothing, then the
        # plain launch below and a reduce by the caller
        r, aff, act = bn
        _chk(aff.scale, aff.shift, aff.mean, aff.invstd)
        partial = torch.empty((2, B, C), device=du.device, dtype=torch.float32)
        if _try_fused(None, 0.0, nbytes + float(B) * N * C * r.element_size(), "nsid_mr_aggregate_bwd_bn", (
                _p(du), _p(idx), _p(amax), B, N, C, k, _p(dy), _p(r), r.shape[-1], _p(aff.scale), _p(aff.shift), _p(aff.mean),
                _p(aff.invstd), act, _p(partial), dt, _stream()), (B * N, C, 2 * C, 1)):
            return dy, partial
    _timed(None, 0.0, nbytes, lambda: call(
        "nsid_mr_aggregate_bwd", _p(du), _p(idx), _p(amax), B, N, C, k, _p(dy), dt, _stream()),
        (B * N, C, 2 * C, 1))
    return (dy, None) if bn is not None else dy


# ------------------------------------------------------------------------------------------------ downsample
def ds_out_nodes(N: int) -> int:
    return (N - 1) // 2 + 1


def im2col3_fwd(x, B, N, C) -> torch.Tensor:
    dt = _act(x)
    col = torch.empty((B * ds_out_nodes(N), 3 * C), device=x.device, dtype=x.dtype)
    call("nsid_im2col3_fwd", _p(x), B, N, C, _p(col), dt, _stream())
    return col


def im2col3_bwd(dcol, B, N, C) -> torch.Tensor:
    dt = _act(dcol)
    dx = torch.empty((B * N, C), device=dcol.device, dtype=dcol.dtype)
    call("nsid_im2col3_bwd", _p(dcol), B, N, C, _p(dx), dt, _stream())
    return dx


class DsPrep:
    """Step-scoped prepared Downsample weights (csrc/misc.hip ds_prepack_kernel): for every registered conv weight (Cout, Cin, 3, 3) the
    packed forward / backward weights in bf16 and two zeroed packed-gradient buffers (one per view), refreshed by ONE launch at the start
    of a step. A training step spent 36 launches on this (pack, pack_bwd, 2 conversions, zero fill, unpack — per layer and per view);
    7 remain (this one + the unpack of each layer and view, which keeps p.grad complete when backward returns)."""

    def __init__(self):
        self.entries = {}           # weight data_ptr -> dict(w, wp16, wb16, dwp, key)

    MAX_LAYERS = _H["NSID_DS_PREPACK_MAX_LAYERS"]

    def purge(self) -> None:
        """drop the layers whose weight is gone or has moved (re-flattened by a newer optimiser): the entries of OTHER live optimisers
        stay (a second FusedClipAdam used to clear them all and silently demoted the first to the per-call launches: ADVICE r4)"""
        for ptr in [k for k, e in self.entries.items() if e["wref"]() is None or e["wref"]().data_ptr() != k]:
            del self.entries[ptr]

    def register(self, w) -> None:
        import weakref
        self.purge()
        if w.data_ptr() in self.entries:
            return
        if len(self.entries) >= self.MAX_LAYERS:
            import warnings
            warnings.warn(f"DsPrep holds {self.MAX_LAYERS} Downsample layers; a further one keeps the per-call pack / convert / zero "
                          "launches (slower, same results)")
            return
        Cout, Cin = w.shape[0], w.shape[1]
        dev = w.device
        self.entries[w.data_ptr()] = dict(wref=weakref.ref(w), Cout=Cout, Cin=Cin, key=None,
                                          wp16=torch.empty((Cout, 3 * Cin), device=dev, dtype=torch.bfloat16),
                                          wb16=torch.empty((2 * Cout, Cin), device=dev, dtype=torch.bfloat16),
                                          dwp=torch.empty((2, Cout, 3 * Cin), device=dev, dtype=torch.float32), slots=0)

    def clear(self) -> None:
        self.entries.clear()

    def _arrays(self, es, *names):
        import ctypes
        n = len(es)
        out = []
        for name in names:
            if name in ("Cout", "Cin"):
                out.append((ctypes.c_int * n)(*[e[name] for e in es]))
            elif name == "w":
                out.append((ctypes.c_void_p * n)(*[e["wref"]().data_ptr() for e in es]))
            else:
                out.append((ctypes.c_void_p * n)(*[e[name].data_ptr() for e in es]))
        return out

    def refresh(self) -> None:
        """pack every registered weight (current values) and zero the shared packed gradients: one launch on the current stream"""
        self.purge()
        es = [e for e in self.entries.values() if e["wref"]().is_cuda] if DS_PREP_ENABLED else []
        if not es:
            return
        w, wp16, wb16, dwp, Cout, Cin = self._arrays(es, "w", "wp16", "wb16", "dwp", "Cout", "Cin")
        _tk("ds_prepack_kernel", sum(4.0 * e["wref"]().numel() / 3 + 2.0 * 5 * e["Cout"] * e["Cin"] + 12.0 * e["Cout"] * e["Cin"] for e in es),
            lambda: call("nsid_ds_prepack", len(es), w, wp16, wb16, dwp, Cout, Cin, _stream()))
        for e in es:
            e["key"], e["slots"] = (e["wref"]()._version, WEIGHT_EPOCH), 0

    def take_slot(self, e):
        """a zeroed packed-gradient buffer of this step (two per layer: one per view), or None when both are taken"""
        if e["slots"] >= e["dwp"].shape[0]:
            return None
        e["slots"] += 1
        return e["dwp"][e["slots"] - 1]

    def get(self, w):
        """the prepared entry of `w` if it was refreshed for the weight's current contents, else None (callers pack per call)"""
        e = self.entries.get(w.data_ptr())
        if not DS_PREP_ENABLED or e is None or e["key"] != (w._version, WEIGHT_EPOCH):
            return None
        owner = e["wref"]()
        # the entry is keyed by address and holds only a weak reference: a NEW weight at the address of a freed one must not inherit
        # its packed copies. `.data` / detach aliases of the registered parameter share its storage and are accepted.
        if owner is None or (owner is not w and (owner.data_ptr() != w.data_ptr() or owner.shape != w.shape or
                                                 owner.untyped_storage().data_ptr() != w.untyped_storage().data_ptr())):
            return None
        return e


DS_PREP = DsPrep()
DS_PREP_ENABLED = 1        # bench.py --flag ops.DS_PREP_ENABLED=0: the per-call pack / convert / zero launches instead (one-box A/B)


def downsample3_fwd(x, B, N, C, wp, bias, Cout, want_stat=False, w16=None):
    """Conv2d 3x3 s2 p1 on a width-1 map as ONE GEMM over a zero-padded strided view of x (no im2col): (B*N, C) ->
    (B*N/2, Cout) raw conv output (+ BatchNorm partial statistics). wp: packed weight (Cout, 3C) fp32 (pack_ds_weight); w16: the same
    already in bf16 (DsPrep; wp may then be None)."""
    _chk(wp, bias)
    dt = _act(x)
    No = N // 2
    M = B * No
    out = torch.empty((M, Cout), device=x.device, dtype=x.dtype)
    stat = torch.empty((2, row_tiles(M), Cout), device=x.device, dtype=torch.float32) if want_stat else None
    wop, wdt = (w16, BF16) if (w16 is not None and dt == BF16) else _weight(wp, dt, 3 * C)      # w16: prepared bf16 packed weight (DsPrep)
    esz = x.element_size()
    _timed("gemm_kernel<128,%d,true,true>" % (64 if Cout <= 64 else 128), 2.0 * M * Cout * 3 * C,
           esz * B * N * C + float(wop.element_size()) * Cout * 3 * C + esz * M * Cout, lambda: call(
        "nsid_downsample3_fwd", _p(x), B, N, C, _p(wop), wdt, _p(bias), _p(out), Cout, _p(stat), dt, _stream()),
        (M, Cout, 3 * C, 1))
    return out, stat


def downsample3_bwd_weight(dout, x, dwp, B, N, C, Cout) -> None:
    """dwp (Cout, 3C) += dout^T col(x), col read as a view of x"""
    _chk(dwp)
    dt = _act(dout, x)
    M = B * (N // 2)
    esz = x.element_size()
    _timed("gemm_kernel<64,64,false,false>", 2.0 * M * Cout * 3 * C, esz * (M * Cout + B * N * C) + 4.0 * Cout * 3 * C,
           lambda: call("nsid_downsample3_bwd_weight", _p(dout), _p(x), _p(dwp), B, N, C, Cout, dt, _stream()),
           (M, Cout, 3 * C, 1))


def downsample3_bwd_data(dout, wp, w_odd, B, N, C, Cout, w16=None) -> torch.Tensor:
    """dx (B*N, C) from dout (B*N/2, Cout): even rows one GEMM, odd rows one GEMM over overlapping rows of dout (no col2im).
    w16 = (packed forward weight, packed odd-row weight) already in bf16 (DsPrep): wp / w_odd may then be None"""
    dt = _act(dout)
    dx = torch.empty((B * N, C), device=dout.device, dtype=dout.dtype)
    if w16 is not None and dt == BF16:
        wop, oop, wdt, odt = w16[0], w16[1], BF16, BF16
    else:
        _chk(wp, w_odd)
        wop, wdt = _weight(wp, dt, 3 * C)
        oop, odt = _weight(w_odd, dt, C)
    if odt != wdt:                       # both from the same arithmetic mode
        wop, wdt, oop, odt = wp, F32, w_odd, F32
    M = B * (N // 2)
    esz = dout.element_size()
    _timed("gemm_kernel<128,%d,true,false>" % (64 if C <= 64 else 128), 2.0 * M * Cout * 3 * C,
           esz * (M * Cout + B * N * C) + float(wop.element_size()) * Cout * 3 * C, lambda: call(
        "nsid_downsample3_bwd_data", _p(dout), _p(wop), _p(oop), wdt, _p(dx), B, N, C, Cout, dt, _stream()),
        (M, Cout, 3 * C, 1))
    return dx


def pack_ds_weight_bwd(w) -> torch.Tensor:
    """(Cout, Cin, 3, 3) -> (2*Cout, Cin): [W_2 ; W_0] of kernel column 1, the right operand of the odd-row backward GEMM"""
    _chk(w)
    Cout, Cin = w.shape[0], w.shape[1]
    wb = torch.empty((2 * Cout, Cin), device=w.device, dtype=torch.float32)
    call("nsid_pack_ds_weight_bwd", _p(w), Cout, Cin, _p(wb), _stream())
    return wb


def pack_ds_weight(w) -> torch.Tensor:
    _chk(w)
    Cout, Cin = w.shape[0], w.shape[1]
    wp = torch.empty((Cout, 3 * Cin), device=w.device, dtype=torch.float32)
    call("nsid_pack_ds_weight", _p(w), Cout, Cin, _p(wp), _stream())
    return wp


def unpack_ds_wgrad(dwp, dw) -> None:
    _chk(dwp, dw)
    call("nsid_unpack_ds_wgrad", _p(dwp), dw.shape[0], dw.shape[1], _p(dw), _stream())


# ------------------------------------------------------------------------------------------------ DGL-variant Downsample chain
# Conv1d(k = 3, stride 2, pad 1) with the BatchNorm + activation of the layer in front applied on the operand load (csrc/dsact.hip).
# w: the Conv1d weight (Cout, C, 3) as stored, fp32. x / r_prev: that layer's raw conv output rows (B*N, C).
def dsact_fwd(x, B, N, C, w, bias, Cout, in_aff: Optional["BNAffine"] = None, act_in=ACT_NONE, want_stat=False,
              out_aff: Optional["BNAffine"] = None, act_out=ACT_NONE):
    """-> (out (B*No, Cout), stat (2, row_tiles(B*No), Cout) or None). out_aff: the eval-mode BatchNorm of THIS layer, applied with
    act_out in the epilogue (out is then the activated output)"""
    dt = _act(x)
    _chk(w, bias, *((in_aff.scale, in_aff.shift) if in_aff is not None else ()),
         *((out_aff.scale, out_aff.shift) if out_aff is not None else ()))
    No = ds_out_nodes(N)
    M = B * No
    out = torch.empty((M, Cout), device=x.device, dtype=x.dtype)
    stat = torch.empty((2, row_tiles(M), Cout), device=x.device, dtype=torch.float32) if want_stat else None
    _timed("dsact_fwd_kernel", 2.0 * M * Cout * 3 * C, float(x.element_size()) * (B * N * C + M * Cout), lambda: call(
        "nsid_dsact_fwd", _p(x), B, N, C, _p(in_aff.scale) if in_aff else None, _p(in_aff.shift) if in_aff else None, act_in,
        _p(w), _p(bias), _p(out), Cout, _p(stat), _p(out_aff.scale) if out_aff else None, _p(out_aff.shift) if out_aff else None,
        act_out, dt, _stream()), (M, Cout, 3 * C, 1))
    return out, stat


def dsact_bwd_weight(dout, x, dw, B, N, C, Cout, in_aff: Optional["BNAffine"] = None, act_in=ACT_NONE) -> None:
    """dw (Cout, C, 3) += dout^T . col(act_in(in_aff(x)))"""
    dt = _act(dout, x)
    _chk(dw, *((in_aff.scale, in_aff.shift) if in_aff is not None else ()))
    M = dout.shape[0]
    _timed("dsact_wgrad_kernel", 2.0 * M * Cout * 3 * C, float(x.element_size()) * (B * N * C + M * Cout), lambda: call(
        "nsid_dsact_bwd_weight", _p(dout), _p(x), _p(in_aff.scale) if in_aff else None, _p(in_aff.shift) if in_aff else None,
        act_in, _p(dw), B, N, C, Cout, dt, _stream()), (Cout, 3 * C, M, 1))


def dsact_bwd_data(dout, w, B, N, C, Cout, r_prev=None, aff: Optional["BNAffine"] = None, act=ACT_NONE, want_partial=False):
    """-> (g (B*N, C), partial or None): g = (conv-transpose of dout) * act'(aff(r_prev)), i.e. the gradient w.r.t. the pre-activation
    of the layer in front; partial (2, rows, C): that layer's BatchNorm-backward column sums (bn_backward(g, ..., ACT_NONE, partial=))"""
    dt = _act(dout, r_prev)
    _chk(w)
    if r_prev is not None:
        _chk(aff.scale, aff.shift)
    if want_partial:
        _chk(aff.mean, aff.invstd)
    dx = torch.empty((B * N, C), device=dout.device, dtype=dout.dtype)
    partial = torch.empty((2, int(lib.nsid_dsact_part_rows(B, N)), C), device=dout.device, dtype=torch.float32) \
        if want_partial else None
    M = dout.shape[0]
    _timed("dsact_dgrad_kernel", 2.0 * M * Cout * 3 * C, float(dout.element_size()) * (M * Cout + 2 * B * N * C), lambda: call(
        "nsid_dsact_bwd_data", _p(dout), _p(w), _p(dx), B, N, C, Cout, _p(r_prev), _p(aff.scale) if aff else None,
        _p(aff.shift) if aff else None, _p(aff.mean) if want_partial else None, _p(aff.invstd) if want_partial else None, act,
        _p(partial), dt, _stream()), (B * N, C, 3 * Cout, 1))
    return dx, partial


# ------------------------------------------------------------------------------------------------ peak extractor
def peak_patchify_fwd(spec, w, bias, pb, pf, out_dtype=torch.float32):
    _chk(spec, w, bias)
    B, H, W = spec.shape
    F = w.shape[0]
    n = (H // pb) * (W // pf)
    out = torch.empty((B * n, F), device=spec.device, dtype=out_dtype)
    minmax = torch.empty((B, 2), device=spec.device, dtype=torch.float32)
    _tk("patchify_fwd_kernel", 4.0 * B * H * W + float(out.element_size()) * B * n * F, lambda: call(
        "nsid_peak_patchify_fwd", _p(spec), _p(w), _p(bias), B, H, W, pb, pf, F, _p(out), F, _p(minmax), _act(out),
        _stream()), (B * n, F, pb * pf * 3, 1))
    return out, minmax


PATCHIFY_BWD_WS = True      # GraFP's patch: per-clip partial sums + one reduce launch (csrc/misc.hip patchify_bwd2_kernel)


def peak_patchify_bwd(spec, minmax, out, dout, pb, pf, dw, dbias) -> None:
    _chk(spec, minmax, dw, dbias)
    B, H, W = spec.shape
    F = out.shape[-1]
    nbytes = 4.0 * B * H * W + 2.0 * out.element_size() * out.numel()
    if PATCHIFY_BWD_WS and (H, W, pb, pf, F) == (64, 128, 4, 8, 8) and out.is_contiguous() and dout.is_contiguous():
        ws = torch.empty((B, 776), device=spec.device, dtype=torch.float32)
        _tk("patchify_bwd2_kernel", nbytes + 8.0 * ws.numel(), lambda: call(
            "nsid_peak_patchify_bwd_ws", _p(spec), _p(minmax), _p(out), _p(dout), F, B, H, W, pb, pf, F, _p(dw), _p(dbias), _p(ws),
            _act(out, dout), _stream()), (out.shape[0], out.shape[1], pb * pf * 3, 1))
        return
    _tk("patchify_bwd_kernel", nbytes, lambda: call(
        "nsid_peak_patchify_bwd", _p(spec), _p(minmax), _p(out), _p(dout), out.shape[-1], B, H, W, pb, pf,
        out.shape[-1], _p(dw), _p(dbias), _act(out, dout), _stream()), (out.shape[0], out.shape[1], pb * pf * 3, 1))


# ------------------------------------------------------------------------------------------------ head
def node_mean_fwd(x, B, N, C) -> torch.Tensor:
    out = torch.empty((B, C), device=x.device, dtype=torch.float32)
    _tk("node_mean_fwd_kernel", float(x.element_size()) * B * N * C, lambda: call(
        "nsid_node_mean_fwd", _p(x), B, N, C, _p(out), _act(x), _stream()), (B * N, C, 0, 1))
    return out


def node_mean_bwd(dout, B, N, C, dtype=torch.float32) -> torch.Tensor:
    _chk(dout)
    dx = torch.empty((B * N, C), device=dout.device, dtype=dtype)
    _tk("node_mean_bwd_kernel", float(dx.element_size()) * B * N * C, lambda: call(
        "nsid_node_mean_bwd", _p(dout), B, N, C, _p(dx), _act(dx), _stream()), (B * N, C, 0, 1))
    return dx


def elu_bwd(dout, out) -> torch.Tensor:
    _chk(dout, out)
    din = torch.empty_like(dout)
    call("nsid_elu_bwd", _p(dout), _p(out), out.numel(), _p(din), _stream())
    return din


def l2norm_fwd(p, eps):
    _chk(p)
    B, d = p.shape
    z = torch.empty_like(p)
    norm = torch.empty((B,), device=p.device, dtype=torch.float32)
    call("nsid_l2norm_fwd", _p(p), B, d, eps, _p(z), _p(norm), _stream())
    return z, norm


def l2norm_bwd(dz, z, norm, eps) -> torch.Tensor:
    _chk(dz, z, norm)
    B, d = z.shape
    dp = torch.empty_like(z)
    call("nsid_l2norm_bwd", _p(dz), _p(z), _p(norm), B, d, eps, _p(dp), _stream())
    return dp


def ntxent_fwd_bwd(z_i, z_j, tau, p0=0, npairs=None, want_grad=True):
    """z_i, z_j: (Bg, d) global embeddings; this rank owns pairs [p0, p0+npairs).
    Returns (loss contribution of the owned rows / (2*Bg), dz_i, dz_j) — dz_* have npairs rows."""
    _chk(z_i, z_j)
    Bg, d = z_i.shape
    npairs = Bg if npairs is None else npairs
    ws = torch.empty((lib.nsid_ntxent_ws_floats(Bg),), device=z_i.device, dtype=torch.float32)
    loss = torch.empty((1,), device=z_i.device, dtype=torch.float32)
    dzi = torch.empty((npairs, d), device=z_i.device, dtype=torch.float32) if want_grad else None
    dzj = torch.empty((npairs, d), device=z_i.device, dtype=torch.float32) if want_grad else None
    # 2 (2B)^2 d flop per pass (similarities; the backward pass recomputes them), bytes = z in + dz out
    _timed("ntxent_kernels", 2.0 * (2 * Bg) * (2 * npairs) * d * (2 if want_grad else 1), 4.0 * d * (2 * Bg + 2 * npairs), lambda: call(
        "nsid_ntxent_fwd_bwd", _p(z_i), _p(z_j), Bg, d, float(tau), p0, npairs, _p(ws), _p(loss), _p(dzi), _p(dzj),
        _stream()), (2 * npairs, 2 * Bg, d, 1))
    return loss, dzi, dzj


# ------------------------------------------------------------------------------------------------ baseline objective (csrc/baseline_loss.hip)
BL_MAX = _H["NSID_BL_MAX"]        # rows (M, or 2 B) and features of the baseline's losses


def _bl_check(name, M, d):
    if d % 16 != 0 or not 16 <= d <= BL_MAX or not 1 <= M <= BL_MAX:
        raise ValueError(f"{name}: D % 16 == 0, 16 <= D <= {BL_MAX} and at most {BL_MAX} rows are supported, got {M} rows of {d}")


def _bl_ws(M, d, device):
    return torch.empty((lib.nsid_baseline_loss_ws_floats(M, d),), device=device, dtype=torch.float32)


def _bl_mining(ws, M):
    """the per-anchor decisions a call leaves at the head of its workspace (include/nsid.h): p*, n* (int32, -1: none), valid, active"""
    Mp = (M + 63) // 64 * 64
    ints = ws[Mp:4 * Mp].view(torch.int32)
    flags = ints[2 * Mp:2 * Mp + M]
    return {"pidx": ints[:M], "nidx": ints[Mp:Mp + M], "valid": (flags & 1).bool(), "active": (flags & 2).bool()}


def pair_ce_fwd_bwd(z_i, z_j, want_grad=True):
    """classifier_loss of simclr/triplet.py:44-61 on z = cat(z_i, z_j): (loss (1,), dz_i, dz_j); gradients None when not wanted"""
    _chk(z_i, z_j)
    B, d = z_i.shape
    if z_j.shape != z_i.shape:
        raise ValueError(f"pair_ce_fwd_bwd: z_i {tuple(z_i.shape)} and z_j {tuple(z_j.shape)} differ")
    _bl_check("pair_ce_fwd_bwd", 2 * B, d)
    ws = _bl_ws(2 * B, d, z_i.device)
    out = torch.empty((1,), device=z_i.device, dtype=torch.float32)
    dzi = torch.empty_like(z_i) if want_grad else None
    dzj = torch.empty_like(z_j) if want_grad else None
    M = 2 * B
    _timed("baseline_loss_kernels<ce>", 2.0 * M * M * d * (2 if want_grad else 1), 4.0 * d * M * (2 if want_grad else 1), lambda: call(
        "nsid_pair_ce_fwd_bwd", _p(z_i), _p(z_j), B, d, _p(ws), _p(out), _p(dzi), _p(dzj), _stream()), (M, M, d, 1))
    return out, dzi, dzj


def triplet_fwd_bwd(e, labels, margin=0.2, want_grad=True, mining=False):
    """triplet_loss of simclr/triplet.py:6-40: (out (2,) = [loss, n_valid], de); mining=True appends the per-anchor decisions"""
    _chk(e)
    if not (labels.is_cuda and labels.dtype == torch.int64 and labels.is_contiguous()):
        raise RuntimeError("triplet_fwd_bwd: labels must be a contiguous int64 tensor on the GPU")
    M, d = e.shape
    if labels.numel() != M:
        raise ValueError(f"triplet_fwd_bwd: {M} embeddings and {labels.numel()} labels")
    _bl_check("triplet_fwd_bwd", M, d)
    ws = _bl_ws(M, d, e.device)
    out = torch.empty((2,), device=e.device, dtype=torch.float32)
    de = torch.empty_like(e) if want_grad else None
    _timed("baseline_loss_kernels<triplet>", 2.0 * M * M * d, 4.0 * d * M * (2 if want_grad else 1), lambda: call(
        "nsid_triplet_fwd_bwd", _p(e), _p(labels), M, d, float(margin), _p(ws), _p(out), _p(de), _stream()), (M, M, d, 1))
    return (out, de, _bl_mining(ws, M)) if mining else (out, de)


def baseline_objective_fwd_bwd(z_i, z_j, margin=0.2, beta=1.0, gamma=1.0, want_grad=True, mining=False, ws=None, out=None, dz=None):
    """the step objective of baseline/train.py:66-77: (out (4,) = [loss, cls, trip, n_valid], dz_i, dz_j). ws / out / dz = (dz_i, dz_j):
    caller-owned buffers (a captured step allocates nothing)"""
    _chk(z_i, z_j)
    B, d = z_i.shape
    if z_j.shape != z_i.shape:
        raise ValueError(f"baseline_objective_fwd_bwd: z_i {tuple(z_i.shape)} and z_j {tuple(z_j.shape)} differ")
    M = 2 * B
    _bl_check("baseline_objective_fwd_bwd", M, d)
    if ws is None:
        ws = _bl_ws(M, d, z_i.device)
    if out is None:
        out = torch.empty((4,), device=z_i.device, dtype=torch.float32)
    _chk(ws, out)
    if ws.numel() < lib.nsid_baseline_loss_ws_floats(M, d) or out.numel() < 4:
        raise ValueError("baseline_objective_fwd_bwd: workspace or result buffer too small")
    if dz is not None:
        dzi, dzj = dz
        _chk(dzi, dzj)
        if dzi.shape != z_i.shape or dzj.shape != z_i.shape:
            raise ValueError("baseline_objective_fwd_bwd: gradient buffers do not match the inputs")
    else:
        dzi = torch.empty_like(z_i) if want_grad else None
        dzj = torch.empty_like(z_j) if want_grad else None
    _timed("baseline_loss_kernels<objective>", 2.0 * M * M * d * (3 if dzi is not None else 2), 4.0 * d * M * 4, lambda: call(
        "nsid_baseline_objective_fwd_bwd", _p(z_i), _p(z_j), B, d, float(margin), float(beta), float(gamma), _p(ws), _p(out),
        _p(dzi), _p(dzj), _stream()), (M, M, d, 1))
    return (out, dzi, dzj, _bl_mining(ws, M)) if mining else (out, dzi, dzj)


BL_ROWS_MAX = _H["NSID_BL_ROWS_MAX"]   # rows (2 Bg) of the gathered batch of baseline_objective_rows_fwd_bwd


def baseline_objective_rows_fwd_bwd(z_i_all, z_j_all, p0=0, npairs=None, margin=0.2, beta=1.0, gamma=1.0, want_grad=True, mining=False,
                                    ws=None, out=None, dz=None):
    """the step objective for one data-parallel rank: z_*_all are the gathered (Bg, d) embeddings of the global batch (rank-major, as
    parallel.gather_pair returns them), 2 Bg <= 4096. (out (4,) = [loss, cls, trip, n_valid] of the GLOBAL batch, dz_i, dz_j), the
    gradients (npairs, d) of out[0] with respect to pairs [p0, p0 + npairs); npairs=None: every pair from p0. The forward covers all rows
    on every rank, so out is bitwise equal on all of them, and a gradient row does not depend on the cut. ws / out / dz and mining (the
    decisions of all 2 Bg anchors) as in baseline_objective_fwd_bwd."""
    name = "baseline_objective_rows_fwd_bwd"
    _chk(z_i_all, z_j_all)
    Bg, d = z_i_all.shape
    if z_j_all.shape != z_i_all.shape:
        raise ValueError(f"{name}: z_i_all {tuple(z_i_all.shape)} and z_j_all {tuple(z_j_all.shape)} differ")
    M = 2 * Bg
    if d % 16 != 0 or not 16 <= d <= BL_MAX or not 1 <= Bg or M > BL_ROWS_MAX:
        raise ValueError(f"{name}: D % 16 == 0, 16 <= D <= {BL_MAX} and at most {BL_ROWS_MAX} rows are supported, got {M} rows of {d}")
    if npairs is None:
        npairs = Bg - p0
    if p0 < 0 or npairs < 1 or p0 + npairs > Bg:
        raise ValueError(f"{name}: pairs [{p0}, {p0} + {npairs}) are not a range of the {Bg} gathered pairs")
    if ws is None:
        ws = torch.empty((lib.nsid_baseline_loss_rows_ws_floats(M, d),), device=z_i_all.device, dtype=torch.float32)
    if out is None:
        out = torch.empty((4,), device=z_i_all.device, dtype=torch.float32)
    _chk(ws, out)
    if ws.numel() < lib.nsid_baseline_loss_rows_ws_floats(M, d) or out.numel() < 4:
        raise ValueError(f"{name}: workspace or result buffer too small")
    if dz is not None:
        dzi, dzj = dz
        _chk(dzi, dzj)
        if dzi.shape != (npairs, d) or dzj.shape != (npairs, d):
            raise ValueError(f"{name}: gradient buffers do not match the owned pairs")
    else:
        dzi = torch.empty((npairs, d), device=z_i_all.device, dtype=torch.float32) if want_grad else None
        dzj = torch.empty((npairs, d), device=z_i_all.device, dtype=torch.float32) if want_grad else None
    flops = 2.0 * M * d * (2 * M + (2 * npairs if dzi is not None else 0))
    _timed("baseline_loss_kernels<objective rows>", flops, 4.0 * d * (3 * M + 2 * npairs), lambda: call(
        "nsid_baseline_objective_rows_fwd_bwd", _p(z_i_all), _p(z_j_all), Bg, d, p0, npairs, float(margin), float(beta), float(gamma),
        _p(ws), _p(out), _p(dzi), _p(dzj), _stream()), (2 * npairs, M, d, 1))
    return (out, dzi, dzj, _bl_mining(ws, M)) if mining else (out, dzi, dzj)


# ------------------------------------------------------------------------------------------------ step plumbing
def fill_zero(t: torch.Tensor) -> torch.Tensor:
    """t[...] = 0 with our own streaming kernel (zero_grad: the captured step holds no ATen kernel)"""
    if not (t.is_cuda and t.is_contiguous()):
        raise RuntimeError("fill_zero needs a contiguous device tensor")
    _tk("fill_zero_kernel", float(t.numel() * t.element_size()), lambda: call(
        "nsid_fill_zero", _p(t), t.numel() * t.element_size(), _stream()), (t.numel(), 1, 0, 1))
    return t


def zeros(shape, device, dtype=torch.float32) -> torch.Tensor:
    return fill_zero(torch.empty(shape, device=device, dtype=dtype))


def scale_f32(x: torch.Tensor, scale: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = x * scale[0] (scale: a device scalar such as autograd's grad_output; None: plain copy)"""
    _chk(x, out)
    if scale is not None:
        scale = scale.reshape(-1)
        _chk(scale)
    if out is None:
        out = torch.empty_like(x)
    call("nsid_scale_f32", _p(x), _p(scale), x.numel(), _p(out), _stream())
    return out


def logmel_fft(waves: torch.Tensor, n_fft: int, hop: int, window: torch.Tensor, twiddle: torch.Tensor, fb: torch.Tensor,
               band: torch.Tensor) -> torch.Tensor:
    """waves (B, L) fp32 (last dimension contiguous, any clip stride) -> log-mel dB (B, n_mels, 1 + L // hop) in ONE launch
    (nsid_logmel_fft, csrc/frontend.hip): reflect framing, real FFT, power, mel sums and dB without a temporary in HBM.
    window (n_fft,), twiddle (n_fft, 2) = (cos, sin)(-2 pi j / n_fft) from fp64, fb (n_mels, n_fft/2+1), band (n_mels, 2) int32"""
    _chk(window, twiddle, fb)
    if waves.dim() != 2 or not waves.is_cuda or waves.dtype != torch.float32 or waves.stride(1) != 1:
        raise RuntimeError("logmel_fft takes (B, L) float32 waveforms on the MI355X device with a contiguous last dimension")
    B, L = waves.shape
    if L <= n_fft // 2:
        raise RuntimeError(f"waveforms of {L} samples are too short for reflect padding by n_fft/2 = {n_fft // 2}")
    n_mels, T = fb.shape[0], 1 + L // hop
    out = torch.empty((B, n_mels, T), device=waves.device, dtype=torch.float32)
    call("nsid_logmel_fft", _p(waves), waves.stride(0) if B > 1 else L, B, L, n_fft, hop, _p(window), _p(twiddle), _p(fb),
         _p(band), n_mels, _p(out), n_mels * T, T, _stream())
    return out


def cqt(waves: torch.Tensor, hop: int, width: int, groups, taps: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """waves (B, L) fp32 (last dimension contiguous, any clip stride) -> constant-Q magnitudes (B, n_bins, 1 + L // hop) in ONE
    launch (nsid_cqt, csrc/cqt.hip): reflect framing, banded exact-fp32 MFMA correlation, sqrt(l_k) and the magnitude without a
    temporary in HBM. groups: host int32 array (n_groups, 5) = {first bin, bins, first tap, extent, table offset}; taps: the packed
    table; scale (n_bins,) = sqrt(l_k) — frontend.CQTFrontEnd builds all three."""
    _chk(taps, scale)
    if waves.dim() != 2 or not waves.is_cuda or waves.dtype != torch.float32 or waves.stride(1) != 1:
        raise RuntimeError("cqt takes (B, L) float32 waveforms on the MI355X device with a contiguous last dimension")
    B, L = waves.shape
    if L <= width // 2:
        raise RuntimeError(f"waveforms of {L} samples are too short for reflect padding by width/2 = {width // 2}")
    if groups.dtype != np.int32 or groups.ndim != 2 or groups.shape[1] != 5 or not groups.flags["C_CONTIGUOUS"]:
        raise RuntimeError("groups must be a C-contiguous int32 host array of shape (n_groups, 5)")
    n_bins, T = scale.numel(), 1 + L // hop
    out = torch.empty((B, n_bins, T), device=waves.device, dtype=torch.float32)
    call("nsid_cqt", _p(waves), waves.stride(0) if B > 1 else L, B, L, hop, width, n_bins, groups.ctypes.data, groups.shape[0],
         _p(taps), taps.numel(), _p(scale), _p(out), n_bins * T, T, _stream())
    return out


# ---- packs of songs (packs.py): the kernels cannot check their device tables, so the wrappers take them from a packs.WavePack only
# (built from a PackPlan that packs.plan_pack derived and validated on the host), never as loose tensors.
def _pack_of(pack, kind: Optional[str], spec: torch.Tensor):
    from .packs import WavePack
    if not isinstance(pack, WavePack) or (kind is not None and pack.plan.kind != kind):
        raise TypeError(f"expected a packs.WavePack{'' if kind is None else ' of kind ' + kind}")
    plan = pack.plan
    if not spec.is_cuda or spec.dtype != torch.float32 or spec.dim() != 2 or spec.stride(1) != 1 or spec.stride(0) != plan.ld \
            or spec.shape[0] != plan.n_rows or spec.shape[1] < plan.total_cols:
        raise RuntimeError(f"the packed spectrogram must be ({plan.n_rows}, >= {plan.total_cols}) float32 on the MI355X device "
                           f"with a row stride of {plan.ld}")
    return plan


def logmel_fft_ragged(pack, n_fft: int, window: torch.Tensor, twiddle: torch.Tensor, fb: torch.Tensor, band: torch.Tensor,
                      spec: torch.Tensor) -> torch.Tensor:
    """the songs of a packs.WavePack -> log-mel dB in ONE launch (nsid_logmel_fft_ragged, csrc/frontend.hip): song i's frames
    are the columns [cols[i], cols[i] + frames[i]) of spec (n_mels, ld), bit-equal to logmel_fft on that song alone"""
    _chk(window, twiddle, fb)
    plan = _pack_of(pack, "logmel", spec)
    if fb.shape[0] != plan.n_rows:
        raise RuntimeError("the filterbank does not match the plan's rows")
    call("nsid_logmel_fft_ragged", _p(pack.wave), _p(pack._songs), plan.n_songs, plan.max_len, plan.total_items, plan.total_cols,
         n_fft, plan.hop, _p(window), _p(twiddle), _p(fb), _p(band), plan.n_rows, _p(spec), plan.ld, _stream())
    return spec


def cqt_ragged(pack, width: int, groups, taps: torch.Tensor, scale: torch.Tensor, spec: torch.Tensor) -> torch.Tensor:
    """the songs of a packs.WavePack -> constant-Q magnitudes in ONE launch (nsid_cqt_ragged, csrc/cqt.hip), in the same packed
    columns, bit-equal to cqt on each song alone"""
    _chk(taps, scale)
    plan = _pack_of(pack, "cqt", spec)
    if groups.dtype != np.int32 or groups.ndim != 2 or groups.shape[1] != 5 or not groups.flags["C_CONTIGUOUS"]:
        raise RuntimeError("groups must be a C-contiguous int32 host array of shape (n_groups, 5)")
    if scale.numel() != plan.n_rows:
        raise RuntimeError("the bin scales do not match the plan's rows")
    call("nsid_cqt_ragged", _p(pack.wave), _p(pack._songs), plan.n_songs, plan.max_len, plan.total_items, plan.total_cols, plan.hop,
         width, plan.n_rows, groups.ctypes.data, groups.shape[0], _p(taps), taps.numel(), _p(scale), _p(spec), plan.ld, _stream())
    return spec


def unfold_segments_ragged(pack, s0: int, nseg: int, out: torch.Tensor) -> torch.Tensor:
    """segments s0 .. s0 + nseg - 1 of the pack's segment list -> out[:nseg] (nsid_unfold_segments_ragged, csrc/misc.hip); out:
    (>= nseg, n_rows, n_frames) contiguous fp32, the rows from nseg on are not touched"""
    plan = _pack_of(pack, None, pack.spec)
    if s0 < 0 or nseg < 1 or s0 + nseg > plan.total_segs:
        raise RuntimeError(f"segments [{s0}, {s0 + nseg}) outside the pack's {plan.total_segs}")
    _chk(out)
    if out.dim() != 3 or out.shape[0] < nseg or tuple(out.shape[1:]) != (plan.n_rows, plan.n_frames):
        raise RuntimeError(f"the micro-batch buffer must be (>= {nseg}, {plan.n_rows}, {plan.n_frames})")
    call("nsid_unfold_segments_ragged", _p(pack.spec), plan.ld, plan.n_rows, plan.n_frames, _p(pack._seg_col), s0, nseg, _p(out),
         _stream())
    return out[:nseg]


# ---- waveform augmentations (csrc/augment.hip, include/nsid.h nsid_aug_*): one wrapper per stage; modules/transformations.
# GPUWaveAugment owns the tables and the workspaces and chains the four. The extents follow the host-side rate bounds alone.
AUG_N_FFT, AUG_HOP, AUG_BINS = _H["NSID_AUG_N_FFT"], _H["NSID_AUG_HOP"], _H["NSID_AUG_BINS"]


def aug_frames_in(L: int) -> int:
    return 1 + L // AUG_HOP


def aug_frames_out_max(L: int, rate_lo) -> int:
    """ceil(T_in / rate_lo) in fp64 on float32(rate_lo): the frames a clip can have after the vocoder"""
    return int(math.ceil(aug_frames_in(L) / float(np.float32(rate_lo))))


def aug_stretched_max(L: int, rate_lo) -> int:
    """rint(L / rate_lo), ties to even: the samples a clip can have after the inverse STFT"""
    return int(np.rint(float(L) / float(np.float32(rate_lo))))


def _aug_waves(name, *ws):
    for w in ws:
        if w.dim() != 2 or not w.is_cuda or w.dtype != torch.float32 or w.stride(1) != 1:
            raise RuntimeError(f"{name} takes (B, L) float32 waveforms on the MI355X device with a contiguous last dimension")


def aug_stft(x_i: torch.Tensor, x_j: torch.Tensor, gain: torch.Tensor, window: torch.Tensor, twiddle: torch.Tensor,
             spec: Optional[torch.Tensor] = None) -> torch.Tensor:
    """STFT of gain[b] * x_j[b] + x_i[b] (n_fft 2048, hop 512, center / zero padding) -> (B, 1 + L // 512, 1025, 2) fp32 = complex64
    with the bin index fastest; the mix is applied on the staging load, no mixed copy is written"""
    _aug_waves("aug_stft", x_i, x_j)
    _chk(gain, window, twiddle, spec)
    B, L = x_i.shape
    if x_j.shape != x_i.shape or gain.numel() != B:
        raise RuntimeError("aug_stft: x_i, x_j of one shape (B, L) and gain of B entries")
    T = aug_frames_in(L)
    if spec is None:
        spec = torch.empty((B, T, AUG_BINS, 2), device=x_i.device, dtype=torch.float32)
    elif spec.numel() < B * T * AUG_BINS * 2:
        raise RuntimeError("aug_stft: the spectrum workspace is too small")
    call("nsid_aug_stft", _p(x_i), x_i.stride(0) if B > 1 else L, _p(x_j), x_j.stride(0) if B > 1 else L, B, L, _p(gain),
         _p(window), _p(twiddle), _p(spec), _stream())
    return spec


def aug_vocoder(spec: torch.Tensor, B: int, L: int, rate: torch.Tensor, rate_lo, rate_hi, out: Optional[torch.Tensor] = None):
    """phase vocoder by rate[b] (clamped into [rate_lo, rate_hi]) on (B, T_in, 1025) spectra -> (B, T_out_max, 1025, 2); clip b's
    columns t >= ceil(T_in / rate) are not written"""
    _chk(spec, rate, out)
    T_max = aug_frames_out_max(L, rate_lo)
    if spec.numel() < B * aug_frames_in(L) * AUG_BINS * 2 or rate.numel() != B:
        raise RuntimeError("aug_vocoder: spec must hold (B, 1 + L // 512, 1025) complex values and rate B entries")
    if out is None:
        out = torch.empty((B, T_max, AUG_BINS, 2), device=spec.device, dtype=torch.float32)
    elif out.numel() < B * T_max * AUG_BINS * 2:
        raise RuntimeError("aug_vocoder: the output workspace is too small")
    call("nsid_aug_vocoder", _p(spec), B, L, _p(rate), float(rate_lo), float(rate_hi), _p(out), T_max, _stream())
    return out


def aug_istft(spec: torch.Tensor, B: int, L: int, rate: torch.Tensor, rate_lo, rate_hi, window: torch.Tensor, twiddle: torch.Tensor,
              wave: Optional[torch.Tensor] = None) -> torch.Tensor:
    """inverse STFT of the vocoder's (B, T_out_max, 1025) spectra -> (B, S_max) stretched waveforms, S_max = rint(L / rate_lo); clip
    b holds rint(L / rate) samples, the rest of its row is not written"""
    _chk(spec, rate, window, twiddle, wave)
    T_max, S_max = aug_frames_out_max(L, rate_lo), aug_stretched_max(L, rate_lo)
    if spec.numel() < B * T_max * AUG_BINS * 2 or rate.numel() != B:
        raise RuntimeError("aug_istft: spec must hold (B, T_out_max, 1025) complex values and rate B entries")
    if wave is None:
        wave = torch.empty((B, S_max), device=spec.device, dtype=torch.float32)
    elif wave.numel() < B * S_max:
        raise RuntimeError("aug_istft: the waveform workspace is too small")
    call("nsid_aug_istft", _p(spec), T_max, B, L, _p(rate), float(rate_lo), float(rate_hi), _p(window), _p(twiddle), _p(wave),
         S_max, _stream())
    return wave


def aug_finish(wave: torch.Tensor, B: int, L: int, mode: torch.Tensor, rate: torch.Tensor, rate_lo, rate_hi, table: torch.Tensor,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, S_max) stretched waveforms -> (B, L): mode 1 resamples by rate through the tabulated filter, any other mode copies;
    both cut or zero-fill to L"""
    _chk(wave, rate, table)
    S_max = aug_stretched_max(L, rate_lo)
    if not mode.is_cuda or mode.dtype != torch.int32 or not mode.is_contiguous() or mode.numel() != B or rate.numel() != B:
        raise RuntimeError("aug_finish: mode must be B contiguous int32 entries on the device, rate B entries")
    if wave.numel() < B * S_max:
        raise RuntimeError("aug_finish: wave must hold (B, rint(L / rate_lo)) samples")
    if out is None:
        out = torch.empty((B, L), device=wave.device, dtype=torch.float32)
    else:
        _aug_waves("aug_finish", out)
        if out.shape != (B, L):
            raise RuntimeError("aug_finish: out must be (B, L)")
    call("nsid_aug_finish", _p(wave), S_max, B, L, _p(mode), _p(rate), float(rate_lo), float(rate_hi), _p(table), _p(out),
         out.stride(0) if B > 1 else L, _stream())
    return out


# ---- the baseline's waveform effects (csrc/augment_fx.hip, include/nsid.h nsid_aug_compress / _biquad / _frames); modules/
# transformations.GPUBaselineWaveAugment chains them with the four stages above
AUG_FX_MAX_SECTIONS, AUG_FX_MAX_FRAMES = _H["NSID_AUG_FX_MAX_SECTIONS"], _H["NSID_AUG_FX_MAX_FRAMES"]


def _aug_table(name, t, dtype, shape):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != shape:
        raise RuntimeError(f"{name} must be a contiguous {dtype} tensor of shape {shape} on the MI355X device")


def _aug_out(name, x, out):
    if out is None:
        return torch.empty(x.shape, device=x.device, dtype=torch.float32)
    _aug_waves(name, out)
    if out.shape != x.shape:
        raise RuntimeError(f"{name}: out must have the input's shape (B, L)")
    return out


def aug_compress(x: torch.Tensor, mode1: torch.Tensor, cmp: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the reference's Compressor on the rows with mode1 == 1: cmp (B, 4) fp64 = threshold, ratio, attack, release; the other rows
    of `out` are not written"""
    _aug_waves("aug_compress", x)
    B, L = x.shape
    _aug_table("aug_compress: mode1", mode1, torch.int32, (B,))
    _aug_table("aug_compress: cmp", cmp, torch.float64, (B, 4))
    out = _aug_out("aug_compress", x, out)
    call("nsid_aug_compress", _p(x), x.stride(0) if B > 1 else L, B, L, _p(mode1), _p(cmp), _p(out),
         out.stride(0) if B > 1 else L, _stream())
    return out


def aug_biquad(x: torch.Tensor, mode1: torch.Tensor, sos: torch.Tensor, n_sec: torch.Tensor,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a cascade of n_sec[b] second-order sections on the rows with mode1 == 0: sos (B, S, 6) fp64 = b0, b1, b2, a1, a2 and the
    factor applied to the section's output; the other rows of `out` are not written"""
    _aug_waves("aug_biquad", x)
    B, L = x.shape
    if sos.dim() != 3 or not 1 <= sos.shape[1] <= AUG_FX_MAX_SECTIONS:
        raise RuntimeError(f"aug_biquad: sos must be (B, S, 6) with 1 <= S <= {AUG_FX_MAX_SECTIONS}")
    _aug_table("aug_biquad: mode1", mode1, torch.int32, (B,))
    _aug_table("aug_biquad: sos", sos, torch.float64, (B, sos.shape[1], 6))
    _aug_table("aug_biquad: n_sec", n_sec, torch.int32, (B,))
    out = _aug_out("aug_biquad", x, out)
    call("nsid_aug_biquad", _p(x), x.stride(0) if B > 1 else L, B, L, _p(mode1), _p(sos), sos.shape[1], _p(n_sec), _p(out),
         out.stride(0) if B > 1 else L, _stream())
    return out


def aug_frames(x_i: torch.Tensor, t1: torch.Tensor, gain: torch.Tensor, mode2: torch.Tensor, frame_size: torch.Tensor,
               frame_ops: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frame edits of the mix gain * t1 + x_i on the rows with 2 <= mode2 <= 4: frame_ops (B, F) int32 bit masks (1 duplicate, 2
    remove, 4 silence); the other rows of `out` are not written"""
    _aug_waves("aug_frames", x_i, t1)
    B, L = x_i.shape
    if t1.shape != x_i.shape or frame_ops.dim() != 2 or not 1 <= frame_ops.shape[1] <= AUG_FX_MAX_FRAMES:
        raise RuntimeError(f"aug_frames: x_i, t1 of one shape (B, L) and frame_ops (B, F) with 1 <= F <= {AUG_FX_MAX_FRAMES}")
    _aug_table("aug_frames: gain", gain, torch.float32, (B,))
    _aug_table("aug_frames: mode2", mode2, torch.int32, (B,))
    _aug_table("aug_frames: frame_size", frame_size, torch.int32, (B,))
    _aug_table("aug_frames: frame_ops", frame_ops, torch.int32, (B, frame_ops.shape[1]))
    out = _aug_out("aug_frames", x_i, out)
    call("nsid_aug_frames", _p(x_i), x_i.stride(0) if B > 1 else L, _p(t1), t1.stride(0) if B > 1 else L, _p(gain), B, L,
         _p(mode2), _p(frame_size), _p(frame_ops), frame_ops.shape[1], _p(out), out.stride(0) if B > 1 else L, _stream())
    return out


# ---- stem pairs (csrc/stems.hip, include/nsid.h nsid_resample_sinc / nsid_stem_pairs_*); modules/data.py owns the bank and the draws
RESAMPLE_WIDTH, RESAMPLE_ROLLOFF = 6, 0.99           # torchaudio's lowpass_filter_width and rolloff defaults
RESAMPLE_MAX_C, RESAMPLE_LDS_BYTES = _H["NSID_RESAMPLE_MAX_C"], _H["NSID_RESAMPLE_LDS_BYTES"]
_RESAMPLE_TABLES = {}                                # (orig, new, device) -> the compact table on the device


def _resample_ratio(orig: int, new: int):
    """(orig, new) divided by their gcd, width, base"""
    orig, new = int(orig), int(new)
    if orig < 1 or new < 1:
        raise ValueError("resampling rates must be positive integers")
    g = math.gcd(orig, new)
    orig, new = orig // g, new // g
    base = min(orig, new) * RESAMPLE_ROLLOFF
    return orig, new, int(math.ceil(RESAMPLE_WIDTH * orig / base)), base


def _resample_k(p, j, orig, new, width, base):
    """(t before the clamp, the fp64 filter value) at phases p and taps j (integer arrays that broadcast), in torchaudio's
    operation order"""
    t = ((-p).astype(np.float64) / new + (j - width).astype(np.float64) / orig) * base
    tc = np.clip(t, -RESAMPLE_WIDTH, RESAMPLE_WIDTH)
    window = np.cos(tc * math.pi / RESAMPLE_WIDTH / 2) ** 2
    tp = tc * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(tp == 0, 1.0, np.sin(tp) / tp)
    return t, k * window * (base / orig)


def resample_table(orig: int, new: int) -> np.ndarray:
    """k[p][j], p < new, j < 2 width + orig (rates divided by their gcd): the polyphase filter of torchaudio's Resample(orig, new)
    with its defaults, evaluated in fp64 and rounded to fp32 once. The rounded table is part of the resampler's definition."""
    orig, new, width, base = _resample_ratio(orig, new)
    if new * (2 * width + orig) > 1 << 26:
        raise ValueError(f"the full filter table of {orig} -> {new} has {new} x {2 * width + orig} entries: too large to tabulate")
    _, k = _resample_k(np.arange(new)[:, None], np.arange(2 * width + orig)[None, :], orig, new, width, base)
    return k.astype(np.float32)


def resample_compact(orig: int, new: int, max_bytes: Optional[int] = None):
    """the live taps of resample_table, computed without the full table: (rows (new, ts) fp32, first (new,) int32, live (new,) int32,
    ntap, width, orig, new). A tap is live where the clamp did not fire (|t| < 6); phase p's live taps are
    k[p][first[p] : first[p] + live[p]], its row is zero behind them, ntap = max live, and ts = ntap | 1 is the row stride the kernel
    keeps in LDS. max_bytes: raise before tabulating when new * (ts + 1) * 4 cannot stay below it."""
    o, n, width, base = _resample_ratio(orig, new)
    half = RESAMPLE_WIDTH * o / base                         # |j - width - p o / n| < half
    if max_bytes is not None and n * int(2 * half) * 4 > max_bytes:          # ts + 1 >= int(2 half): cannot fit
        raise RuntimeError(f"resample_sinc: the compact filter table of {orig} -> {new} ({n} phases x about {int(2 * half)} taps) "
                           f"exceeds the {max_bytes} bytes of LDS the kernel keeps it in")
    p = np.arange(n, dtype=np.int64)[:, None]
    lo = np.floor(width + p * o / n - half).astype(np.int64) - 2
    j = lo + np.arange(int(2 * half) + 6, dtype=np.int64)[None, :]
    t, k = _resample_k(p, j, o, n, width, base)
    alive = (np.abs(t) < RESAMPLE_WIDTH) & (j >= 0) & (j < 2 * width + o)
    a0 = alive.argmax(1)
    live = alive.sum(1).astype(np.int32)
    first = j[np.arange(n), a0].astype(np.int32)
    ntap = int(live.max())
    ts = ntap | 1
    assert live.min() >= 1 and not alive[:, 0].any() and not alive[:, -1].any()          # the window held every live tap
    rows = np.zeros((n, ts), dtype=np.float32)
    k32 = k.astype(np.float32)
    for q in range(n):
        assert alive[q, a0[q]:a0[q] + live[q]].all()                                     # one run per phase
        rows[q, :live[q]] = k32[q, a0[q]:a0[q] + live[q]]
    if max_bytes is not None and (rows.size + n) * 4 > max_bytes:
        raise RuntimeError(f"resample_sinc: the compact filter table of {orig} -> {new} ({n} phases x {ntap} taps) exceeds the "
                           f"{max_bytes} bytes of LDS the kernel keeps it in")
    return rows, first, live, ntap, width, o, n


def resample_out_len(T: int, orig: int, new: int) -> int:
    g = math.gcd(int(orig), int(new))
    return -((-(new // g) * T) // (orig // g))


def _resample_tables(orig, new, device):
    key = (int(orig), int(new), torch.device(device))
    e = _RESAMPLE_TABLES.get(key)
    if e is None:
        if orig == new:                              # the downmix alone: one phase, one tap of weight 1
            rows, first, ntap, width, o, n = np.ones((1, 1), np.float32), np.zeros(1, np.int32), 1, 0, 1, 1
        else:
            rows, first, _, ntap, width, o, n = resample_compact(orig, new, RESAMPLE_LDS_BYTES)
        e = (torch.from_numpy(rows).to(device), torch.from_numpy(first).to(device), ntap, rows.shape[1], width, o, n)
        _RESAMPLE_TABLES[key] = e
    return e


def resample_sinc(x: torch.Tensor, orig: int, new: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torchaudio.transforms.Resample(orig, new) (defaults) of the mono downmix of x: (T,) or (C, T) fp32 on the device, C <= 8 ->
    (ceil(new T / orig),). orig == new returns the input ((T,)) or its downmix ((C, T))."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() not in (1, 2) or x.stride(-1) != 1:
        raise RuntimeError("resample_sinc takes (T,) or (C, T) float32 audio on the MI355X device with a contiguous last dimension; "
                           "there is no host path")
    C, T = (1, x.shape[0]) if x.dim() == 1 else x.shape
    if not 1 <= C <= RESAMPLE_MAX_C or not 1 <= T < 2 ** 31:
        raise RuntimeError(f"resample_sinc: 1 <= C <= {RESAMPLE_MAX_C} channels of 1 <= T < 2^31 samples, got C = {C}, T = {T}")
    if orig == new and x.dim() == 1:
        return x
    rows, first, ntap, ts, width, o, n = _resample_tables(orig, new, x.device)
    T_out = resample_out_len(T, orig, new)
    if T_out >= 2 ** 31:
        raise RuntimeError("resample_sinc: the output must have fewer than 2^31 samples")
    if out is None:
        out = torch.empty((T_out,), device=x.device, dtype=torch.float32)
    elif not out.is_cuda or out.dtype != torch.float32 or out.shape != (T_out,) or not out.is_contiguous():
        raise RuntimeError(f"resample_sinc: out must be ({T_out},) contiguous float32 on the device")
    stride = x.stride(0) if x.dim() == 2 and C > 1 else T
    _tk("resample_sinc", 4 * (C * T + T_out), lambda: call(
        "nsid_resample_sinc", _p(x), stride, C, T, o, n, width, _p(rows), _p(first), ntap, ts, _p(out), T_out, _stream()), (C, T))
    return out


def _sp_table(name, t, dtype, shape):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != shape:
        raise RuntimeError(f"stem_pairs: {name} must be a contiguous {dtype} tensor of shape {shape} on the MI355X device")


def stem_pairs(bank: torch.Tensor, base: torch.Tensor, length: torch.Tensor, track: torch.Tensor, start: torch.Tensor,
               key: torch.Tensor, off_i: torch.Tensor, off_j: torch.Tensor, L: int, O: int, silence: float,
               pack: Optional[int] = None):
    """N candidate clips from the bank (flat fp32 buffer; track t = three rows of length[t] from element base[t]): SNR gate, split,
    crops and silence test (include/nsid.h nsid_stem_pairs_gate / _build), two launches, no host synchronisation.
    pack None -> (x_i (N, L), x_j (N, L), status (N,) i32, snr (N, 3) f32), rejected rows zero;
    pack = B  -> (x_i (B, L), x_j (B, L), n_ok () i32, status, snr): the accepted clips in order, zeros from row n_ok on."""
    if not isinstance(bank, torch.Tensor) or not bank.is_cuda or bank.dtype != torch.float32 or bank.dim() != 1 or \
            not bank.is_contiguous() or bank.numel() < 1:
        raise RuntimeError("stem_pairs: the bank is a flat contiguous float32 buffer on the MI355X device; there is no host path")
    n_tracks, N = base.numel(), track.numel()
    L, O = int(L), int(O)
    if n_tracks < 1 or not 1 <= N <= 65535 or L < 1 or O < 1 or L + O >= 2 ** 30:
        raise RuntimeError("stem_pairs: need at least one track, 1 <= N <= 65535 clips, L >= 1, O >= 1 and L + O < 2^30")
    _sp_table("base", base, torch.int64, (n_tracks,))
    _sp_table("length", length, torch.int32, (n_tracks,))
    _sp_table("track", track, torch.int32, (N,))
    _sp_table("start", start, torch.int32, (N,))
    _sp_table("key", key, torch.float32, (N, 3))
    _sp_table("off_i", off_i, torch.int32, (N,))
    _sp_table("off_j", off_j, torch.int32, (N,))
    dev = bank.device
    status = torch.empty((N,), device=dev, dtype=torch.int32)
    plan = torch.empty((N,), device=dev, dtype=torch.int32)
    snr = torch.empty((N, 3), device=dev, dtype=torch.float32)
    W = L + O
    _tk("stem_pairs_gate", 4 * N * (3 * W + 3 * L), lambda: call(
        "nsid_stem_pairs_gate", _p(bank), bank.numel(), _p(base), _p(length), n_tracks, _p(track), _p(start), _p(key), _p(off_i),
        _p(off_j), N, L, O, float(silence), _p(status), _p(snr), _p(plan), _stream()), (N, W))
    if pack is None:
        rows, n_ok = N, None
    else:
        rows = int(pack)
        if not 1 <= rows <= 65535:
            raise RuntimeError("stem_pairs: 1 <= pack <= 65535 output rows")
        n_ok = torch.empty((), device=dev, dtype=torch.int32)
    x_i = torch.empty((rows, L), device=dev, dtype=torch.float32)
    x_j = torch.empty((rows, L), device=dev, dtype=torch.float32)
    _tk("stem_pairs_build", 4 * rows * 5 * L, lambda: call(
        "nsid_stem_pairs_build", _p(bank), bank.numel(), _p(base), _p(length), n_tracks, _p(track), _p(start), _p(off_i), _p(off_j),
        _p(status), _p(plan), N, L, O, 0 if pack is None else 1, rows if pack is not None else 0, _p(x_i), L, _p(x_j), L, _p(n_ok),
        _stream()), (rows, L))
    if pack is None:
        return x_i, x_j, status, snr
    return x_i, x_j, n_ok, status, snr


def batched_index_select_fwd(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """x (B, C, N) fp32, idx (B, Nq, k) int32 -> (B, C, Nq, k) — the reference's batched_index_select (torch_nn.py:79-98)"""
    _chk(x)
    B, C, N = x.shape
    _, Nq, k = idx.shape
    out = torch.empty((B, C, Nq, k), device=x.device, dtype=torch.float32)
    call("nsid_batched_index_select_fwd", _p(x), _p(idx), B, C, N, Nq, k, _p(out), _stream())
    return out


def batched_index_select_bwd(dout: torch.Tensor, idx: torch.Tensor, N: int) -> torch.Tensor:
    _chk(dout)
    B, C, Nq, k = dout.shape
    dx = zeros((B, C, N), dout.device)
    call("nsid_batched_index_select_bwd", _p(dout), _p(idx), B, C, N, Nq, k, _p(dx), _stream())
    return dx


# ------------------------------------------------------------------------------------------------ optimiser
def sumsq_partial(g_flat) -> torch.Tensor:
    _chk(g_flat)
    n = g_flat.numel()
    partial = torch.empty((lib.nsid_sumsq_blocks(n),), device=g_flat.device, dtype=torch.float32)
    _tk("sumsq_kernel", 4.0 * n, lambda: call("nsid_sumsq_partial", _p(g_flat), n, _p(partial), _stream()), (n, 1, 0, 1))
    return partial


def adam_step(p, g, m, v, hyper, step, partial, gnorm_out) -> None:
    _chk(p, g, m, v, hyper, partial, gnorm_out)
    # reads p, g, m, v and writes p, m, v: 28 bytes per parameter
    _tk("adam_kernel", 28.0 * p.numel(), lambda: call(
        "nsid_adam_step", _p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), _p(step), _p(partial), partial.numel(),
        _p(gnorm_out), _stream()), (p.numel(), 1, 0, 1))


# ------------------------------------------------------------------------------------------------ layout
def bcn_to_rows(x, dtype=torch.float32) -> torch.Tensor:
    """(B, C, N[, 1]) fp32 reference layout -> node-major (B*N, C) in the activation storage type"""
    _chk(x)
    B, C, N = x.shape[0], x.shape[1], x.shape[2]
    rows = torch.empty((B * N, C), device=x.device, dtype=dtype)
    call("nsid_bcn_to_rows", _p(x), B, C, N, _p(rows), C, _act(rows), _stream())
    return rows


def rows_to_bcn(rows, B, N) -> torch.Tensor:
    """node-major (B*N, C) of either storage type -> (B, C, N) fp32"""
    C = rows.shape[-1]
    x = torch.empty((B, C, N), device=rows.device, dtype=torch.float32)
    call("nsid_rows_to_bcn", _p(rows), C, B, C, N, _p(x), _act(rows), _stream())
    return x


# ------------------------------------------------------------------------------------------------ exact flat-L2 search (csrc/search.hip)
SEARCH_MAX_K = _H["NSID_SEARCH_MAX_K"]
SEARCH_D_LIMITS = "d % 16 == 0 and 16 <= d <= 256, or d % 64 == 0 and 256 < d <= 2048"


def search_d_ok(d) -> bool:
    """the row widths csrc/search.hip takes (l2_shape_ok): above 256 flat_l2_topk runs its LDS-staged wide kernel"""
    return (d % 16 == 0 and 16 <= d <= 256) or (d % 64 == 0 and 256 < d <= 2048)


def _search_rows(t, name):
    """a (n, d) fp32 matrix on the GPU with unit column stride and 16-byte rows; d % 16 == 0 and 16 <= d <= 256, or d % 64 == 0
    and 256 < d <= 2048 (SEARCH_D_LIMITS)"""
    if not t.is_cuda:
        raise RuntimeError("neuralsampleid_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
    if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) % 4 or t.data_ptr() % 16:
        raise RuntimeError(f"{name}: expected a (rows, d) float32 matrix with unit column stride and 16-byte aligned rows")
    d = t.shape[1]
    if not search_d_ok(d):
        raise ValueError(f"{name}: d = {d} is outside the search kernels' limits ({SEARCH_D_LIMITS})")
    return max(t.stride(0), d)


def row_sqnorm(x) -> torch.Tensor:
    """(n, d) fp32 -> (n,) fp32 squared row norms in one fixed summation order"""
    ldx = _search_rows(x, "row_sqnorm")
    n, d = x.shape
    out = torch.empty((n,), device=x.device, dtype=torch.float32)
    _tk("row_sqnorm_kernel", 4.0 * n * (d + 1), lambda: call("nsid_row_sqnorm", _p(x), ldx, n, d, _p(out), _stream()), (n, d, 0, 1))
    return out


def _flat_l2_topk(name, q, x, x_sqnorm, k, q_sqnorm, ex):
    """the two search entries: ex = None (nsid_flat_l2_topk) or the (ex_lo, ex_hi) device tensors of nsid_flat_l2_topk_excl"""
    k = int(k)
    if not 1 <= k <= SEARCH_MAX_K:
        raise ValueError(f"{name}: k = {k} is outside [1, {SEARCH_MAX_K}]")
    ldq, ldx = _search_rows(q, f"{name} q"), _search_rows(x, f"{name} x")
    if q.shape[1] != x.shape[1]:
        raise ValueError(f"{name}: query d = {q.shape[1]} != database d = {x.shape[1]}")
    _chk(x_sqnorm)
    nq, d = q.shape
    nx = x.shape[0]
    if x_sqnorm.numel() != nx:
        raise ValueError(f"{name}: x_sqnorm must hold one norm per database row")
    for t in ex or ():
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() \
                or t.numel() != nq:
            raise ValueError(f"{name}: ex_lo and ex_hi must be contiguous int32 tensors of {nq} entries on the GPU")
    if q_sqnorm is None:
        q_sqnorm = row_sqnorm(q)
    D = torch.empty((nq, k), device=q.device, dtype=torch.float32)
    I = torch.empty((nq, k), device=q.device, dtype=torch.int64)
    if nq == 0:
        return D, I
    wsb = int(lib.nsid_workspace_bytes(b"flat_l2_topk", nq, nx))
    ws = torch.empty((max(wsb, 16),), device=q.device, dtype=torch.uint8)
    xp, xnp = (_p(x), _p(x_sqnorm)) if nx else (None, None)
    tail = (d, k, _p(D), _p(I), _p(ws), ws.numel(), _stream())
    # phase 1 streams the database once per query block (32 rows; 128 at d > 256) and runs 2 nq nx d flop on the fp32 matrix pipe
    if ex is None:
        fn = lambda: call("nsid_flat_l2_topk", _p(q), ldq, nq, xp, ldx, nx, xnp, _p(q_sqnorm), *tail)
    else:
        fn = lambda: call("nsid_flat_l2_topk_excl", _p(q), ldq, nq, xp, ldx, nx, xnp, _p(q_sqnorm), _p(ex[0]), _p(ex[1]), *tail)
    _timed(name, 2.0 * nq * nx * d, 4.0 * nx * d + 4.0 * nq * d + 12.0 * nq * k, fn, (nq, nx, d, k))
    return D, I


def flat_l2_topk(q, x, x_sqnorm, k, q_sqnorm=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """exhaustive squared-L2 top-k of every row of q (nq, d) over the rows of x (nx, d) with their norms x_sqnorm (row_sqnorm):
    D (nq, k) fp32 ascending, I (nq, k) int64, equal distances smaller id first, k > nx padded with I = -1, D = +inf"""
    return _flat_l2_topk("flat_l2_topk", q, x, x_sqnorm, k, q_sqnorm, None)


def flat_l2_topk_excl(q, x, x_sqnorm, k, ex_lo, ex_hi, q_sqnorm=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """flat_l2_topk in which the database rows ex_lo[i] <= j < ex_hi[i] do not compete for query row i (leave-one-out search; ex_lo[i]
    >= ex_hi[i]: nothing is left out). ex_lo, ex_hi: int32 device tensors of nq entries, any values (they are only compared with row
    ids); nothing here reads them on the host. Row i's result is bitwise flat_l2_topk's over x without those rows, the ids mapped
    back; a row with fewer than k rows left is padded with I = -1, D = +inf."""
    return _flat_l2_topk("flat_l2_topk_excl", q, x, x_sqnorm, k, q_sqnorm, (ex_lo, ex_hi))


def flat_norm_topk(q, x, norm, k, ex=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The exhaustive top-k of every row of q (nq, d) over the rows of x (nx, d) under the cohort-normalised score (include/nsid.h,
    "normalised candidate search"): z[i][j] is the cell ops.pair_sim(norm=) stores for the same two rows, bit for bit, and row i gets
    its k largest z. norm = (q_mu, q_rs, x_mu, x_rs) as pair_sim takes them (cohort_stats of the rows of q and of x). Z (nq, k) fp32
    descending, I (nq, k) int64; equal z smaller id first, a NaN z does not compete, and where fewer than k rows compete the tail is
    I = -1, Z = -inf. ex = (ex_lo, ex_hi): flat_l2_topk_excl's per-row ranges of database rows that do not compete, None for none.
    The kernel taken is the library's to name (nsid_debug_last_kernel); there is no fallback."""
    name = "flat_norm_topk"
    k = int(k)
    if not 1 <= k <= SEARCH_MAX_K:
        raise ValueError(f"{name}: k = {k} is outside [1, {SEARCH_MAX_K}]")
    ldq, ldx = _search_rows(q, f"{name} q"), _search_rows(x, f"{name} x")
    if q.shape[1] != x.shape[1]:
        raise ValueError(f"{name}: query d = {q.shape[1]} != database d = {x.shape[1]}")
    nq, d = q.shape
    nx = x.shape[0]
    norm = _norm_stats(norm, nq, nx, name)
    if ex is not None and (not isinstance(ex, (tuple, list)) or len(ex) != 2):
        raise ValueError(f"{name}: ex must be (ex_lo, ex_hi) or None")
    for t in ex or ():
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() \
                or t.numel() != nq:
            raise ValueError(f"{name}: ex_lo and ex_hi must be contiguous int32 tensors of {nq} entries on the GPU")
    Z = torch.empty((nq, k), device=q.device, dtype=torch.float32)
    I = torch.empty((nq, k), device=q.device, dtype=torch.int64)
    if nq == 0:
        return Z, I
    wsb = int(lib.nsid_workspace_bytes(b"flat_norm_topk", nq, nx))
    ws = torch.empty((max(wsb, 16),), device=q.device, dtype=torch.uint8)
    exp = (None, None) if ex is None else (_p(ex[0]), _p(ex[1]))
    # flat_l2_topk's flop and bytes, and the two statistics of every row
    _timed(None, 2.0 * nq * nx * d, 4.0 * nx * (d + 2) + 4.0 * nq * (d + 2) + 12.0 * nq * k,
           lambda: call("nsid_flat_norm_topk", _p(q), ldq, nq, _p(x) if nx else None, ldx, nx, *(_p(t) for t in norm), *exp, d, k, _p(Z),
                        _p(I), _p(ws), ws.numel(), _stream()), (nq, nx, d, k))
    return Z, I


# ---- the certified bf16 pre-filter (include/nsid.h)
PREFILTER_M = SEARCH_MAX_K          # candidates per query row
PREFILTER_MAX_D = 256               # the coarse kernel's widest row; above it the plain search runs


def prefilter_d_ok(d) -> bool:
    return d % 16 == 0 and 16 <= d <= PREFILTER_MAX_D


def _bf16_rows_t(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.bfloat16 or t.dim() != 2 or t.stride(1) != 1 \
            or t.stride(0) % 8 or t.data_ptr() % 16:
        raise RuntimeError(f"{name}: expected a (rows, d) bfloat16 matrix on the GPU with unit column stride and 16-byte aligned rows")
    return max(t.stride(0), t.shape[1])


def bf16_rows(x) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(n, d) fp32 -> (xb, err, nrm): the round-to-nearest-even bf16 rows, err[i] >= ||x_i - xb_i|| and nrm[i] >= max(||x_i||,
    ||xb_i||) as fp32 rounded upwards (fp64 sums on the device)"""
    ldx = _search_rows(x, "bf16_rows")
    n, d = x.shape
    xb = torch.empty((n, d), device=x.device, dtype=torch.bfloat16)
    err = torch.empty((n,), device=x.device, dtype=torch.float32)
    nrm = torch.empty((n,), device=x.device, dtype=torch.float32)
    _tk("bf16_rows_kernel", 6.0 * n * d + 8.0 * n, lambda: call("nsid_bf16_rows", _p(x), ldx, n, d, _p(xb), d, _p(err), _p(nrm), _stream()),
        (n, d, 0, 1))
    return xb, err, nrm


def _ex_pair(name, ex, nq):
    for t in ex or ():
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() \
                or t.numel() != nq:
            raise ValueError(f"{name}: ex_lo and ex_hi must be contiguous int32 tensors of {nq} entries on the GPU")


def flat_l2_topk_coarse(qb, xb, x_sqnorm, ex=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """the pre-filter's coarse pass: per row of qb (nq, d) bf16 the PREFILTER_M smallest coarse keys x_sqnorm[j] - 2 qb.xb_j (bf16
    MFMA, fp32 accumulate) over the rows of xb, ties smaller id first; ex = (ex_lo, ex_hi) as in flat_l2_topk_excl. Returns ckey
    (nq, M) fp32 and cid (nq, M) int32, pads (+inf, INT_MAX) last."""
    name = "flat_l2_topk_coarse"
    ldq, ldx = _bf16_rows_t(qb, f"{name} qb"), _bf16_rows_t(xb, f"{name} xb")
    nq, d = qb.shape
    nx = xb.shape[0]
    if xb.shape[1] != d:
        raise ValueError(f"{name}: query d = {d} != database d = {xb.shape[1]}")
    if not prefilter_d_ok(d):
        raise ValueError(f"{name}: d = {d} is outside d % 16 == 0 and 16 <= d <= {PREFILTER_MAX_D}")
    _chk(x_sqnorm)
    if x_sqnorm.numel() != nx:
        raise ValueError(f"{name}: x_sqnorm must hold one norm per database row")
    _ex_pair(name, ex, nq)
    M = PREFILTER_M
    ckey = torch.empty((nq, M), device=qb.device, dtype=torch.float32)
    cid = torch.empty((nq, M), device=qb.device, dtype=torch.int32)
    if nq == 0:
        return ckey, cid
    wsb = int(lib.nsid_workspace_bytes(b"flat_l2_topk_coarse", nq, nx))
    ws = torch.empty((max(wsb, 16),), device=qb.device, dtype=torch.uint8)
    xp, xnp = (_p(xb), _p(x_sqnorm)) if nx else (None, None)
    lo, hi = (_p(ex[0]), _p(ex[1])) if ex is not None else (None, None)
    _timed(name, 2.0 * nq * nx * d, 2.0 * nx * d + 2.0 * nq * d + 8.0 * nq * M, lambda: call(
        "nsid_flat_l2_topk_coarse", _p(qb), ldq, nq, xp, ldx, nx, xnp, lo, hi, d, _p(ckey), _p(cid), _p(ws), ws.numel(), _stream()),
        (nq, nx, d, M))
    return ckey, cid


def flat_l2_rescore(q, x, x_sqnorm, q_sqnorm, q_err, q_nrm, xmax, exmax, ckey, cid, k):
    """the pre-filter's exact pass: the candidates cid (nq, M) of every query row re-scored with flat_l2_topk's fp32 chain and sorted by
    (key, id). Returns (D, I, E, cert): (nq, k) results, the per-row error bound and the uint8 certificate; D / I of a row with
    cert = 0 are not the search result. xmax / exmax: device floats (1 element) >= max ||x_j|| / max ||x_j - bf16(x_j)||."""
    name = "flat_l2_rescore"
    k = int(k)
    if not 1 <= k <= SEARCH_MAX_K:
        raise ValueError(f"{name}: k = {k} is outside [1, {SEARCH_MAX_K}]")
    ldq, ldx = _search_rows(q, f"{name} q"), _search_rows(x, f"{name} x")
    nq, d = q.shape
    nx = x.shape[0]
    if x.shape[1] != d or not prefilter_d_ok(d):
        raise ValueError(f"{name}: d = {d} / {x.shape[1]} must agree and lie in d % 16 == 0, 16 <= d <= {PREFILTER_MAX_D}")
    _chk(x_sqnorm, q_sqnorm, q_err, q_nrm, xmax, exmax, ckey)
    if x_sqnorm.numel() != nx or q_sqnorm.numel() != nq or q_err.numel() != nq or q_nrm.numel() != nq or xmax.numel() != 1 \
            or exmax.numel() != 1:
        raise ValueError(f"{name}: one norm per row and one-element xmax / exmax are expected")
    M = PREFILTER_M
    if tuple(ckey.shape) != (nq, M) or tuple(cid.shape) != (nq, M) or cid.dtype != torch.int32 or not cid.is_cuda or not cid.is_contiguous():
        raise ValueError(f"{name}: ckey / cid must be ({nq}, {M}) fp32 / int32 tensors on the GPU")
    D = torch.empty((nq, k), device=q.device, dtype=torch.float32)
    I = torch.empty((nq, k), device=q.device, dtype=torch.int64)
    E = torch.empty((nq,), device=q.device, dtype=torch.float32)
    cert = torch.empty((nq,), device=q.device, dtype=torch.uint8)
    if nq == 0:
        return D, I, E, cert
    xp, xnp = (_p(x), _p(x_sqnorm)) if nx else (None, None)
    _timed(name, 128.0 * nq * M * d, 4.0 * nq * M * d + 4.0 * nq * d + 12.0 * nq * k, lambda: call(
        "nsid_flat_l2_rescore", _p(q), ldq, nq, xp, ldx, nx, xnp, _p(q_sqnorm), _p(q_err), _p(q_nrm), _p(xmax), _p(exmax), _p(ckey),
        _p(cid), d, k, _p(D), _p(I), _p(E), _p(cert), _stream()), (nq, M, d, k))
    return D, I, E, cert


def flat_l2_topk_pre(q, x, xb16, x_sqnorm, xmax, exmax, k, ex=None):
    """flat_l2_topk (ex = None) or flat_l2_topk_excl (ex = (ex_lo, ex_hi)) through the certified bf16 pre-filter: bf16_rows of the
    queries, the coarse pass over xb16 (bf16_rows of x), the exact re-score. Returns (D, I, cert); rows with cert = 1 hold the plain
    entry's result bit for bit, rows with cert = 0 do NOT: there is no fallback here (search.FlatL2Index.search runs it)."""
    qb, q_err, q_nrm = bf16_rows(q)
    ckey, cid = flat_l2_topk_coarse(qb, xb16, x_sqnorm, ex)
    D, I, _, cert = flat_l2_rescore(q, x, x_sqnorm, row_sqnorm(q), q_err, q_nrm, xmax, exmax, ckey, cid, k)
    return D, I, cert


def seq_scores(q, x, I, starts, lens, ldo) -> torch.Tensor:
    """eval.py:325-331 for every (start, length) pair at once: out[p, j] = mean over i < min(L, nx - cid) of q[s+i].x[cid+i] with
    cid = I[s + j // k, j % k] (j < L k), NaN for cid < 0 and for j >= L k. starts / lens: host integer sequences (checked here
    against the rows of q and I, then copied to the GPU)."""
    import numpy as np
    ldq, ldx = _search_rows(q, "seq_scores q"), _search_rows(x, "seq_scores x")
    if q.shape[1] != x.shape[1]:
        raise ValueError("seq_scores: query and database d differ")
    if I.dtype != torch.int64 or I.dim() != 2 or not I.is_contiguous() or not I.is_cuda:
        raise RuntimeError("seq_scores: I must be a contiguous (rows, k) int64 tensor on the GPU")
    k = I.shape[1]
    if not 1 <= k <= SEARCH_MAX_K:
        raise ValueError(f"seq_scores: k = {k} is outside [1, {SEARCH_MAX_K}]")
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    if starts.shape != lens.shape:
        raise ValueError("seq_scores: starts and lens differ in length")
    ldo = int(ldo)
    npairs = starts.size
    if npairs and (starts.min() < 0 or lens.min() < 1 or (starts + lens).max() > min(q.shape[0], I.shape[0])):
        raise ValueError("seq_scores: every pair needs 0 <= start, 1 <= length and start + length <= the rows of q and I")
    if not 0 <= ldo <= 4 * 65535:
        raise ValueError(f"seq_scores: ldo = {ldo} is outside [0, 262140]")
    out = torch.empty((npairs, ldo), device=q.device, dtype=torch.float32)
    if npairs == 0 or ldo == 0:
        return out
    st = torch.from_numpy(starts.astype(np.int32)).to(q.device)
    ln = torch.from_numpy(lens.astype(np.int32)).to(q.device)
    nx, d = x.shape
    _tk("seq_scores_kernel", 8.0 * float(lens.sum()) * k * d, lambda: call(
        "nsid_seq_scores", _p(q), ldq, _p(x), ldx, nx, d, _p(I), k, _p(st), _p(ln), npairs, _p(out), ldo, _stream()),
        (npairs, ldo, d, 1))
    return out


# ------------------------------------------------------------------------------------------------ song-level vote (csrc/vote.hip)
VOTE_MAX_CAND = _H["NSID_VOTE_MAX_CAND"]          # L k of a pair at most
VOTE_MAX_TOP = _H["NSID_VOTE_MAX_TOP"]


def _vote_args(name, I, starts, lens, song_of, n_dummy, exclude, top):
    """the checks the two votes share; returns (k, starts, lens as int64 numpy, exclude as int32 numpy or None, n_ref, n_dummy, top)"""
    if not I.is_cuda or not song_of.is_cuda:
        raise RuntimeError("neuralsampleid_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
    if I.dtype != torch.int64 or I.dim() != 2 or not I.is_contiguous():
        raise RuntimeError(f"{name}: I must be a contiguous (rows, k) int64 tensor on the GPU")
    if song_of.dtype != torch.int32 or song_of.dim() != 1 or not song_of.is_contiguous():
        raise RuntimeError(f"{name}: song_of must be a contiguous 1-D int32 tensor (one song code per ref row; negative = never votes) on the GPU")
    k, top, n_dummy = I.shape[1], int(top), int(n_dummy)
    if not 1 <= k <= SEARCH_MAX_K:
        raise ValueError(f"{name}: k = {k} is outside [1, {SEARCH_MAX_K}]")
    if not 1 <= top <= VOTE_MAX_TOP:
        raise ValueError(f"{name}: top = {top} is outside [1, {VOTE_MAX_TOP}]")
    if n_dummy < 0 or n_dummy + song_of.numel() >= 2 ** 31:
        raise ValueError(f"{name}: n_dummy must be >= 0 and the ids must stay below 2^31")
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    if starts.shape != lens.shape:
        raise ValueError(f"{name}: starts and lens differ in length")
    if starts.size and (starts.min() < 0 or lens.min() < 1 or (starts + lens).max() > I.shape[0]):
        raise ValueError(f"{name}: every pair needs 0 <= start, 1 <= length and start + length <= the rows of I")
    if starts.size and int(lens.max()) * k > VOTE_MAX_CAND:
        raise ValueError(f"{name}: a pair of {int(lens.max())} rows x k = {k} has more than {VOTE_MAX_CAND} candidates")
    if exclude is not None:
        exclude = np.asarray(exclude, dtype=np.int64).reshape(-1)
        if exclude.shape != starts.shape:
            raise ValueError(f"{name}: exclude must hold one song code (-1 = none) per pair")
        exclude = exclude.astype(np.int32)
    return k, starts, lens, exclude, int(song_of.numel()), n_dummy, top


def _vote_out(npairs, top, device):
    return (torch.empty((npairs, top), device=device, dtype=torch.int32), torch.empty((npairs, top), device=device, dtype=torch.float64),
            torch.empty((npairs,), device=device, dtype=torch.int32))


def _vote_table(device, starts, lens, exclude, *more):
    """the per-pair int32 columns of a vote in ONE upload (a one-pair vote is latency: every copy counts); returns the device rows
    (starts, lens, exclude or None, *more)"""
    cols = [starts, lens, lens if exclude is None else exclude, *more]
    t = torch.from_numpy(np.stack(cols).astype(np.int32)).to(device)
    return (t[0], t[1], None if exclude is None else t[2], *(t[3 + i] for i in range(len(more))))


def song_vote(I, scores, starts, lens, song_of, n_dummy, exclude=None, top=10):
    """The song-level vote of eval.py:296-367 for every (start, length) pair at once (search.aggregate_hit_rates's rule).

    I (rows, k) int64 ids over dummy ++ ref; scores (pairs, >= max length * k) fp32: seq_scores' output for the same pairs; song_of
    (n_ref,) int32 device song codes (a negative code never votes); exclude: one song code per pair that never votes (-1 = none), or None. starts / lens / exclude:
    host integer sequences, checked here. Returns (songs (pairs, top) int32, best first, -1 past the last; totals (pairs, top) float64,
    bit for bit the host's sums; n_songs (pairs,) int32 = the distinct songs that voted), all on the device."""
    k, starts, lens, exclude, n_ref, n_dummy, top = _vote_args("song_vote", I, starts, lens, song_of, n_dummy, exclude, top)
    if not scores.is_cuda:
        raise RuntimeError("neuralsampleid_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1 and scores.shape[1] > 1:
        raise RuntimeError("song_vote: scores must be a (pairs, columns) float32 matrix with unit column stride on the GPU")
    npairs = starts.size
    if scores.shape[0] != npairs or (npairs and scores.shape[1] < int(lens.max()) * k):
        raise ValueError(f"song_vote: scores must be ({npairs}, >= {int(lens.max()) * k if npairs else 0}), got {tuple(scores.shape)}")
    songs, totals, n_songs = _vote_out(npairs, top, I.device)
    if npairs == 0:
        return songs, totals, n_songs
    lds = int(scores.stride(0)) if npairs > 1 else int(scores.shape[1])
    if not scores.shape[1] <= lds <= VOTE_MAX_CAND:
        raise ValueError(f"song_vote: the rows of scores must be {VOTE_MAX_CAND} floats apart at most and must not overlap, got {lds}")
    st, ln, ex = _vote_table(I.device, starts, lens, exclude)
    ncand = float((lens * k).sum())
    _tk("song_vote_kernel", 12.0 * ncand + 4.0 * ncand + 16.0 * npairs * top, lambda: call(
        "nsid_song_vote", _p(I), k, _p(scores), lds, _p(st), _p(ln), npairs, _p(song_of), n_ref, n_dummy, _p(ex), top, _p(songs),
        _p(totals), _p(n_songs), _stream()), (npairs, int(lens.max()) * k, top, 1))
    return songs, totals, n_songs


def song_vote_clf(I, S, s_off, s_ld, starts, lens, song_of, n_dummy, exclude=None, threshold=0.5, top=10):
    """The song-level vote of eval_hr.py:85-156 for every (start, length) pair at once (rerank.vote_hit_rates_clf's rule, without
    its node-matrix file skips: every ref row of the index has node matrices).

    S: flat fp32 classifier scores on the device; pair p's block starts at s_off[p], has rows of s_ld[p] floats, and its column j is
    walk position j (clf_pair_scores_dev over vote_candidates' list): the score of position j is the max over the pair's first L rows,
    added to its song when >= threshold. The other arguments and the result are song_vote's."""
    k, starts, lens, exclude, n_ref, n_dummy, top = _vote_args("song_vote_clf", I, starts, lens, song_of, n_dummy, exclude, top)
    _chk(S)
    S = S.reshape(-1)
    s_off = np.asarray(s_off, dtype=np.int64).reshape(-1)
    s_ld = np.asarray(s_ld, dtype=np.int64).reshape(-1)
    npairs = starts.size
    if s_off.shape != starts.shape or s_ld.shape != starts.shape:
        raise ValueError("song_vote_clf: s_off and s_ld must hold one entry per pair")
    if npairs and (s_off.min() < 0 or s_ld.min() < 0 or s_ld.max() >= 2 ** 31
                   or (s_off + (lens - 1) * s_ld + lens * k).max() > S.numel()):
        raise ValueError("song_vote_clf: a pair's score block (length rows of s_ld floats, length * k columns) leaves S")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("song_vote_clf: threshold is NaN")
    songs, totals, n_songs = _vote_out(npairs, top, I.device)
    if npairs == 0:
        return songs, totals, n_songs
    st, ln, ex, sl = _vote_table(I.device, starts, lens, exclude, s_ld)
    so = torch.from_numpy(np.ascontiguousarray(s_off)).to(I.device)
    ncand = float((lens * k).sum())
    _tk("song_vote_kernel<clf>", 12.0 * ncand + 4.0 * float((lens * lens * k).sum()) + 16.0 * npairs * top, lambda: call(
        "nsid_song_vote_clf", _p(I), k, _p(S), _p(so), _p(sl), _p(st), _p(ln), npairs, _p(song_of), n_ref, n_dummy, _p(ex), threshold,
        top, _p(songs), _p(totals), _p(n_songs), _stream()), (npairs, int(lens.max()) * k, top, 1))
    return songs, totals, n_songs


DIAG_MAX_BIN = _H["NSID_DIAG_MAX_BIN"]


def diag_vote(I, starts, lens, song_of, n_dummy, exclude=None, bin_rows=16, top=10):
    """The diagonal-histogram vote (include/nsid.h nsid_diag_vote) for every (start, length) pair at once: a song's score is the
    largest number of its hits (query row i, reference row r) whose diagonal r - i falls into one bin of 2 bin_rows rows (bins
    overlap by half), wherever in the pair's rows the diagonal starts. It needs no scores.

    I, starts, lens, song_of, n_dummy, exclude: song_vote's. Returns (songs (pairs, top) int32, best first, -1 past the last; counts
    (pairs, top) int32; i_lo, i_hi, r_lo, r_hi (pairs, top) int32: the first and last query row (index into I) and reference row of
    the hits in the song's winning bin, -1 past the last; n_songs (pairs,) int32 = the distinct songs that voted), on the device."""
    k, starts, lens, exclude, n_ref, n_dummy, top = _vote_args("diag_vote", I, starts, lens, song_of, n_dummy, exclude, top)
    bin_rows = int(bin_rows)
    if not 1 <= bin_rows <= DIAG_MAX_BIN:
        raise ValueError(f"diag_vote: bin_rows = {bin_rows} is outside [1, {DIAG_MAX_BIN}]")
    if n_ref + VOTE_MAX_CAND >= 2 ** 31:
        raise ValueError(f"diag_vote: {n_ref} reference rows + {VOTE_MAX_CAND} must stay below 2^31")
    npairs = starts.size
    out = tuple(torch.empty((npairs, top), device=I.device, dtype=torch.int32) for _ in range(6))
    n_songs = torch.empty((npairs,), device=I.device, dtype=torch.int32)
    if npairs == 0:
        return (*out, n_songs)
    st, ln, ex = _vote_table(I.device, starts, lens, exclude)
    ncand = float((lens * k).sum())
    _tk("diag_vote_kernel", 2 * 12.0 * ncand + 24.0 * npairs * top, lambda: call(
        "nsid_diag_vote", _p(I), k, _p(st), _p(ln), npairs, _p(song_of), n_ref, n_dummy, _p(ex), bin_rows, top, *(_p(t) for t in out),
        _p(n_songs), _stream()), (npairs, int(lens.max()) * k, top, bin_rows))
    return (*out, n_songs)


def vote_candidates(I, n_dummy, n_ref) -> torch.Tensor:
    """the device candidate list of a search result: I (any shape) int64 ids over dummy ++ ref -> int32 of the same shape, I - n_dummy
    for a ref row and 0 elsewhere (the votes skip those positions from I, so what is scored there is never read)"""
    if not I.is_cuda:
        raise RuntimeError("neuralsampleid_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
    if I.dtype != torch.int64 or not I.is_contiguous():
        raise RuntimeError("vote_candidates: I must be a contiguous int64 tensor on the GPU")
    n_dummy, n_ref = int(n_dummy), int(n_ref)
    if n_dummy < 0 or n_ref < 0 or n_dummy + n_ref >= 2 ** 31:
        raise ValueError("vote_candidates: n_dummy and n_ref must be >= 0 and the ids must stay below 2^31")
    cidx = torch.empty(I.shape, device=I.device, dtype=torch.int32)
    n = I.numel()
    if n:
        _tk("vote_candidates_kernel", 12.0 * n, lambda: call("nsid_vote_candidates", _p(I), n, n_dummy, n_ref, _p(cidx), _stream()),
            (n, 0, 0, 1))
    return cidx


# ------------------------------------------------------------------------------------------------ locating a sample (csrc/align.hip)
ALIGN_MAX_ROWS = _H["NSID_ALIGN_MAX_ROWS"]        # query rows of a pair at most
ALIGN_MAX_COLS = _H["NSID_ALIGN_MAX_COLS"]        # song rows of a pair at most
ALIGN_MAX_TOP = _H["NSID_ALIGN_MAX_TOP"]
ALIGN_MAX_SONG_ROWS = _H["NSID_ALIGN_MAX_SONG_ROWS"]   # song rows of a pair at most where the walk goes in column panels (local_align_panels)
ALIGN_TILE = 32                                   # pair_sim's tiles (one wave each)


def _align_seq(name, what, v, n=None):
    v = np.asarray(v, dtype=np.int64).reshape(-1)
    if n is not None and v.size != n:
        raise ValueError(f"{name}: {what} must hold one entry per pair ({n}), got {v.size}")
    return v


def pair_sim_tiles(q_len, x_len) -> np.ndarray:
    """the work list of pair_sim: (ntiles, 3) int32 rows {pair, i0, j0}, the 32 x 32 tiles of every pair, largest pairs first (equal
    sizes in pair order), a pair's tiles row-major"""
    q_len, x_len = np.asarray(q_len, dtype=np.int64), np.asarray(x_len, dtype=np.int64)
    ti, tj = (q_len + ALIGN_TILE - 1) // ALIGN_TILE, (x_len + ALIGN_TILE - 1) // ALIGN_TILE
    order = np.argsort(-(ti * tj), kind="stable")
    order = order[(ti * tj)[order] > 0]
    if order.size == 0:
        return np.zeros((0, 3), dtype=np.int32)
    cnt = (ti * tj)[order]
    pair = np.repeat(order, cnt)
    local = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    w = tj[pair]
    return np.stack([pair, (local // w) * ALIGN_TILE, (local % w) * ALIGN_TILE], axis=1).astype(np.int32)


COHORT_MIN, COHORT_MAX, COHORT_CHUNK = _H["NSID_COHORT_MIN"], _H["NSID_COHORT_MAX"], _H["NSID_COHORT_CHUNK"]


def cohort_stats(x, cohort) -> Tuple[torch.Tensor, torch.Tensor]:
    """The background statistics of every row of x (n, d) over the cohort (M, d), COHORT_MIN <= M <= COHORT_MAX: (mu, rs), fp32 device
    tensors of n entries, the mean of the row's pair_sim scores against the cohort rows and 1 / their standard deviation, summed in
    fp64 in the fixed order of include/nsid.h ("cohort score normalisation"): a row's bits depend on the row and the cohort alone."""
    ldx, ldc = _search_rows(x, "cohort_stats x"), _search_rows(cohort, "cohort_stats cohort")
    if x.shape[1] != cohort.shape[1]:
        raise ValueError(f"cohort_stats: row d = {x.shape[1]} != cohort d = {cohort.shape[1]}")
    (n, d), M = x.shape, cohort.shape[0]
    if not COHORT_MIN <= M <= COHORT_MAX:
        raise ValueError(f"cohort_stats: a cohort of {M} rows is outside [{COHORT_MIN}, {COHORT_MAX}]")
    if n >= 2 ** 31:
        raise ValueError("cohort_stats: x must have fewer than 2^31 rows")
    mu = torch.empty((n,), device=x.device, dtype=torch.float32)
    rs = torch.empty((n,), device=x.device, dtype=torch.float32)
    if n == 0:
        return mu, rs
    ws = torch.empty((int(lib.nsid_workspace_bytes(b"cohort_stats", n, M)) // 8,), device=x.device, dtype=torch.float64)
    _timed("cohort_partial_kernel", 2.0 * n * M * d, 4.0 * d * (n + M) + 8.0 * n, lambda: call(
        "nsid_cohort_stats", _p(x), ldx, n, _p(cohort), ldc, M, d, _p(mu), _p(rs), _p(ws), _stream()), (n, M, d, 1))
    return mu, rs


def _norm_stats(norm, nq, nx, name="pair_sim"):
    """pair_sim's (and flat_norm_topk's) norm=(q_mu, q_rs, x_mu, x_rs): contiguous fp32 device vectors that cover every row of q / x"""
    if not isinstance(norm, (tuple, list)) or len(norm) != 4:
        raise ValueError(f"{name}: norm must be (q_mu, q_rs, x_mu, x_rs)")
    for t, what, rows in zip(norm, ("q_mu", "q_rs", "x_mu", "x_rs"), (nq, nq, nx, nx)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: norm {what} must be a torch tensor on the GPU")
        _chk(t)
        if t.dim() != 1 or t.numel() < rows:
            raise ValueError(f"{name}: norm {what} must be a vector with one entry per row ({rows}), got {tuple(t.shape)}: the "
                             "statistics are indexed by the absolute row of q / x")
    return tuple(norm)


def pair_sim(q, x, q_start, q_len, x_start, x_len, s_ld=None, out=None, long_songs=False, norm=None):
    """The score matrices of many (query rows, song rows) pairs in one launch: S_p[i, j] = q[q_start[p] + i] . x[x_start[p] + j], the
    dot of flat_l2_topk (one k-ordered fp32 fmaf chain; an element's bits depend on its two rows alone).

    norm=(q_mu, q_rs, x_mu, x_rs) (cohort_stats of ALL rows of q and of x, indexed by absolute row): the cohort-normalised cell
    0.5 ((s - q_mu[i]) q_rs[i] + (s - x_mu[j]) x_rs[j]) is stored instead of the dot s (nsid_pair_sim_norm, the same tiles); None is
    nsid_pair_sim itself.

    q (nq, d), x (nx, d): fp32 rows as the search takes them. q_start / q_len / x_start / x_len: host integer sequences, one entry per
    pair, checked here and then uploaded; lengths may be 0, and are at most ALIGN_MAX_ROWS / ALIGN_MAX_COLS. s_ld: per pair the row
    stride of its block (default x_len). out: a flat fp32 device tensor to write into (default: a new one; what lies between x_len
    and s_ld is not written). long_songs=True: x_len may be up to ALIGN_MAX_SONG_ROWS (the kernel has no width limit; the matrices
    are local_align_panels' input). Returns (S flat fp32, s_off int64 numpy, s_ld int64 numpy): pair p's block starts at S[s_off[p]]."""
    max_cols = ALIGN_MAX_SONG_ROWS if long_songs else ALIGN_MAX_COLS
    q_start = _align_seq("pair_sim", "q_start", q_start)
    npairs = q_start.size
    q_len, x_start, x_len = (_align_seq("pair_sim", w, v, npairs) for w, v in (("q_len", q_len), ("x_start", x_start), ("x_len", x_len)))
    s_ld = x_len.copy() if s_ld is None else _align_seq("pair_sim", "s_ld", s_ld, npairs)
    if npairs and (q_start.min() < 0 or q_len.min() < 0 or x_start.min() < 0 or x_len.min() < 0):
        raise ValueError("pair_sim: every pair needs 0 <= start and 0 <= length")
    if npairs and (q_len.max() > ALIGN_MAX_ROWS or x_len.max() > max_cols):
        raise ValueError(f"pair_sim: a pair of {int(q_len.max())} x {int(x_len.max())} rows is outside the limits "
                         f"({ALIGN_MAX_ROWS} query rows, {max_cols} song rows); longer inputs are refused, not split")
    ldq, ldx = _search_rows(q, "pair_sim q"), _search_rows(x, "pair_sim x")
    if q.shape[1] != x.shape[1]:
        raise ValueError(f"pair_sim: query d = {q.shape[1]} != song d = {x.shape[1]}")
    if npairs and ((q_start + q_len).max() > q.shape[0] or (x_start + x_len).max() > x.shape[0]):
        raise ValueError("pair_sim: every pair needs start + length <= the rows of q / x")
    if npairs and ((s_ld < x_len).any() or s_ld.max() >= 2 ** 31):
        raise ValueError("pair_sim: s_ld must be >= x_len for every pair")
    if q.shape[0] >= 2 ** 31:
        raise ValueError("pair_sim: q must have fewer than 2^31 rows")
    if norm is not None:
        norm = _norm_stats(norm, q.shape[0], x.shape[0])
    size = q_len * s_ld
    s_off = np.cumsum(size) - size
    total = int(size.sum())
    if out is None:
        out = torch.empty((total,), device=q.device, dtype=torch.float32)
    else:
        _chk(out)
        if out.dim() != 1 or out.numel() < total:
            raise ValueError(f"pair_sim: out must be a flat tensor of at least {total} floats")
    tiles = pair_sim_tiles(q_len, x_len)
    if tiles.shape[0] == 0:
        return out, s_off, s_ld
    dev = q.device
    t32 = torch.from_numpy(np.stack([q_start, q_len, x_len, s_ld]).astype(np.int32)).to(dev)
    t64 = torch.from_numpy(np.stack([x_start, s_off])).to(dev)
    tl = torch.from_numpy(np.ascontiguousarray(tiles)).to(dev)
    d = q.shape[1]
    cells = float((q_len * x_len).sum())
    args = (_p(q), ldq, q.shape[0], _p(x), ldx, x.shape[0], d, _p(t32[0]), _p(t32[1]), _p(t64[0]), _p(t32[2]), _p(t64[1]), _p(t32[3]),
            npairs, _p(tl), tiles.shape[0], _p(out), out.numel())
    nbytes = 4.0 * cells + 4.0 * d * 2 * ALIGN_TILE * tiles.shape[0]
    if norm is None:
        _timed("pair_sim_kernel", 2.0 * cells * d, nbytes, lambda: call("nsid_pair_sim", *args, _stream()),
               (npairs, tiles.shape[0], d, 1))
    else:
        _timed("pair_sim_norm_kernel", 2.0 * cells * d, nbytes, lambda: call("nsid_pair_sim_norm", *args, *(_p(t) for t in norm), _stream()),
               (npairs, tiles.shape[0], d, 1))
    return out, s_off, s_ld


def local_align(S, s_off, s_ld, q_len, x_len, theta, min_score=0.0, top=16):
    """The local alignment of include/nsid.h ("locating a sample") for many pairs in one launch, one workgroup per pair.

    S: flat fp32 scores on the device; pair p's matrix starts at s_off[p], has q_len[p] rows of s_ld[p] floats and x_len[p] columns
    (pair_sim's output, or classifier scores). s_off / s_ld / q_len / x_len: host integer sequences, checked here, then uploaded.
    Returns (occ (pairs, top, 4) int32 = (i0, i1, j0, j1), -1 in unused slots; occ_score (pairs, top) fp32, 0 in unused slots; n_occ
    (pairs,) int32, it can exceed top; row_h, row_j, row_org: the per-row results of all pairs, pair p's at row_off[p] + i; row_off int64
    numpy). A pair with a zero length has n_occ = 0 (and 0, -1, -1 in its rows, if it has any)."""
    if not isinstance(S, torch.Tensor):
        raise TypeError("local_align: S must be a torch tensor on the GPU")
    _chk(S)
    S = S.reshape(-1)
    s_off = _align_seq("local_align", "s_off", s_off)
    npairs = s_off.size
    s_ld, q_len, x_len = (_align_seq("local_align", w, v, npairs) for w, v in (("s_ld", s_ld), ("q_len", q_len), ("x_len", x_len)))
    top = int(top)
    if not 1 <= top <= ALIGN_MAX_TOP:
        raise ValueError(f"local_align: top = {top} is outside [1, {ALIGN_MAX_TOP}]")
    theta, min_score = float(theta), float(min_score)
    if theta != theta or min_score != min_score:
        raise ValueError("local_align: theta or min_score is NaN")
    if npairs and (q_len.min() < 0 or x_len.min() < 0):
        raise ValueError("local_align: a length is negative")
    if npairs and (q_len.max() > ALIGN_MAX_ROWS or x_len.max() > ALIGN_MAX_COLS):
        raise ValueError(f"local_align: a pair of {int(q_len.max())} x {int(x_len.max())} rows is outside the limits "
                         f"({ALIGN_MAX_ROWS} query rows, {ALIGN_MAX_COLS} song rows); longer inputs are refused, not split")
    full = (q_len > 0) & (x_len > 0)
    if npairs and full.any() and (s_off[full].min() < 0 or (s_ld[full] < x_len[full]).any() or s_ld.max() >= 2 ** 31
                                  or (s_off + (q_len - 1) * s_ld + x_len)[full].max() > S.numel()):
        raise ValueError("local_align: a pair's score block (q_len rows of s_ld >= x_len floats) leaves S")
    dev = S.device
    row_off = np.cumsum(q_len) - q_len
    rows = int(q_len.sum())
    occ = torch.empty((npairs, top, 4), device=dev, dtype=torch.int32)
    occ_score = torch.empty((npairs, top), device=dev, dtype=torch.float32)
    n_occ = torch.empty((npairs,), device=dev, dtype=torch.int32)
    row_h = torch.empty((rows,), device=dev, dtype=torch.float32)
    row_j = torch.empty((rows,), device=dev, dtype=torch.int32)
    row_org = torch.empty((rows,), device=dev, dtype=torch.int32)
    if npairs == 0:
        return occ, occ_score, n_occ, row_h, row_j, row_org, row_off
    t32 = torch.from_numpy(np.stack([s_ld, q_len, x_len]).astype(np.int32)).to(dev)
    t64 = torch.from_numpy(np.stack([np.where(full, s_off, 0), row_off])).to(dev)
    cells = float((q_len * x_len).sum())
    _tk("local_align_kernel", 4.0 * cells + 24.0 * rows, lambda: call(
        "nsid_local_align", _p(S), _p(t64[0]), _p(t32[0]), _p(t32[1]), _p(t32[2]), npairs, int(q_len.max()), int(x_len.max()), theta,
        min_score, top, _p(t64[1]), _p(row_h), _p(row_j), _p(row_org), _p(occ), _p(occ_score), _p(n_occ), _stream()),
        (npairs, int(q_len.max()), int(x_len.max()), top))
    return occ, occ_score, n_occ, row_h, row_j, row_org, row_off


ALIGN_OCC_MAX_ROWS = _H["NSID_ALIGN_OCC_MAX_ROWS"]      # rows of one run of align_occurrences at most


def align_carry(x_len, device, long_songs=False):
    """a carry for local_align_strip: ((carry_h fp32, carry_i0 int32, carry_j0 int32) flat device tensors, carry_off int64 numpy);
    pair p's two rows of x_len[p] cells start at carry_off[p]. The content is not initialised: a pair's first strip is fresh.
    long_songs=True: a carry for local_align_panels, lengths up to ALIGN_MAX_SONG_ROWS."""
    x_len = _align_seq("align_carry", "x_len", x_len)
    max_cols = ALIGN_MAX_SONG_ROWS if long_songs else ALIGN_MAX_COLS
    if x_len.size and (x_len.min() < 0 or x_len.max() > max_cols):
        raise ValueError(f"align_carry: a song of {int(x_len.max())} rows is outside [0, {max_cols}]")
    size = 2 * x_len
    n = int(size.sum())
    carry = (torch.empty((n,), device=device, dtype=torch.float32), torch.empty((n,), device=device, dtype=torch.int32),
             torch.empty((n,), device=device, dtype=torch.int32))
    return carry, np.cumsum(size) - size


def _flat_dev(name, what, t, dtype):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: {what} must be a torch tensor on the GPU")
    if not t.is_cuda:
        raise RuntimeError("neuralsampleid_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
    if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous():
        raise RuntimeError(f"{name}: {what} must be a flat contiguous {dtype} tensor")


def local_align_strip(S, s_off, s_ld, q_len, x_len, theta, row_base, fresh, carry, carry_off, rows=None, row_off=None):
    """One strip of the local alignment of include/nsid.h for many pairs in one launch (nsid_local_align_strip): pair p's q_len[p] rows
    are the GLOBAL query rows row_base[p] .. of its matrix, and the walk starts from the pair's carried rows (fresh[p]: from zeros) and
    leaves the last two rows in the carry, in place. Chained over strips of any lengths this is the rule on the whole matrix, bit for
    bit, whatever the cuts.

    S, s_off, s_ld, q_len, x_len, theta: as local_align takes them (q_len: the rows of this strip, at most ALIGN_MAX_ROWS). row_base,
    fresh, carry_off: host integer sequences, one entry per pair. carry: (carry_h fp32, carry_i0 int32, carry_j0 int32), flat device
    tensors of one length (align_carry); pair p's part is [carry_off[p], carry_off[p] + 2 x_len[p]), and the parts must not overlap.
    rows / row_off: four flat device tensors (fp32, int32, int32, int32) and per pair the first element to write the row results into
    (default: new tensors, the pairs one after the other). Returns (row_h, row_j, row_i0, row_j0, row_off int64 numpy, open_h (pairs,)
    fp32 on the device): a row without a passing cell holds 0, -1, -1, -1; the rows of a pair with q_len = 0 are not written; open_h is
    the largest H carried out (0: no path is open)."""
    return _align_strip("local_align_strip", None, S, s_off, s_ld, q_len, x_len, theta, row_base, fresh, carry, carry_off, rows, row_off)


def local_align_panels(S, s_off, s_ld, q_len, x_len, theta, row_base, fresh, carry, carry_off, panel_cols=ALIGN_MAX_COLS, rows=None,
                       row_off=None):
    """local_align_strip for songs of up to ALIGN_MAX_SONG_ROWS rows (nsid_local_align_panels): the same arguments, the same outputs
    and the same bits, the walk going over the song in panels of panel_cols columns (2 .. ALIGN_MAX_COLS) with two carried columns
    between them. The result does not depend on panel_cols. carry: align_carry(..., long_songs=True). The halo workspace
    ((q_len + 2) x 2 cells per pair) is allocated here and dropped after the launch."""
    panel_cols = int(panel_cols)
    if not 2 <= panel_cols <= ALIGN_MAX_COLS:
        raise ValueError(f"local_align_panels: panel_cols = {panel_cols} is outside [2, {ALIGN_MAX_COLS}]")
    return _align_strip("local_align_panels", panel_cols, S, s_off, s_ld, q_len, x_len, theta, row_base, fresh, carry, carry_off, rows,
                        row_off)


def _align_strip(name, panel_cols, S, s_off, s_ld, q_len, x_len, theta, row_base, fresh, carry, carry_off, rows, row_off):
    """the checks and the launch of local_align_strip (panel_cols None) and local_align_panels"""
    max_cols = ALIGN_MAX_COLS if panel_cols is None else ALIGN_MAX_SONG_ROWS
    if not isinstance(S, torch.Tensor):
        raise TypeError(f"{name}: S must be a torch tensor on the GPU")
    _chk(S)
    S = S.reshape(-1)
    s_off = _align_seq(name, "s_off", s_off)
    npairs = s_off.size
    s_ld, q_len, x_len, row_base, fresh, carry_off = (_align_seq(name, w, v, npairs) for w, v in (
        ("s_ld", s_ld), ("q_len", q_len), ("x_len", x_len), ("row_base", row_base), ("fresh", fresh), ("carry_off", carry_off)))
    theta = float(theta)
    if theta != theta:
        raise ValueError(f"{name}: theta is NaN")
    if npairs and (q_len.min() < 0 or x_len.min() < 0):
        raise ValueError(f"{name}: a length is negative")
    if npairs and (q_len.max() > ALIGN_MAX_ROWS or x_len.max() > max_cols):
        raise ValueError(f"{name}: a strip of {int(q_len.max())} x {int(x_len.max())} rows is outside the limits "
                         f"({ALIGN_MAX_ROWS} query rows per strip, {max_cols} song rows)")
    if npairs and (row_base.min() < 0 or (row_base + q_len).max() > 2 ** 31 - 1):
        raise ValueError(f"{name}: every pair needs 0 <= row_base and row_base + q_len <= 2^31 - 1")
    full = (q_len > 0) & (x_len > 0)
    if npairs and full.any() and (s_off[full].min() < 0 or (s_ld[full] < x_len[full]).any() or s_ld.max() >= 2 ** 31
                                  or (s_off + (q_len - 1) * s_ld + x_len)[full].max() > S.numel()):
        raise ValueError(f"{name}: a pair's score block (q_len rows of s_ld >= x_len floats) leaves S")
    if not isinstance(carry, (tuple, list)) or len(carry) != 3:
        raise TypeError(f"{name}: carry must be (carry_h, carry_i0, carry_j0)")
    for what, t, dt in zip(("carry_h", "carry_i0", "carry_j0"), carry, (torch.float32, torch.int32, torch.int32)):
        _flat_dev(name, what, t, dt)
    if not carry[0].numel() == carry[1].numel() == carry[2].numel():
        raise ValueError(f"{name}: the three carry tensors must have one length")
    if npairs:
        order = np.argsort(carry_off, kind="stable")
        lo, hi = carry_off[order], (carry_off + 2 * x_len)[order]
        if lo[0] < 0 or hi.max() > carry[0].numel() or (lo[1:] < hi[:-1]).any():
            raise ValueError(f"{name}: a pair's carry (2 x_len cells at carry_off) leaves the carry tensors or overlaps another's")
    dev = S.device
    total = int(q_len.sum())
    if rows is None:
        if row_off is not None:
            raise ValueError(f"{name}: row_off needs rows")
        row_off = np.cumsum(q_len) - q_len
        rows = (torch.empty((total,), device=dev, dtype=torch.float32),) + tuple(
            torch.empty((total,), device=dev, dtype=torch.int32) for _ in range(3))
    else:
        if not isinstance(rows, (tuple, list)) or len(rows) != 4 or row_off is None:
            raise TypeError(f"{name}: rows must be (row_h, row_j, row_i0, row_j0), given together with row_off")
        for what, t, dt in zip(("row_h", "row_j", "row_i0", "row_j0"), rows, (torch.float32, torch.int32, torch.int32, torch.int32)):
            _flat_dev(name, what, t, dt)
        row_off = _align_seq(name, "row_off", row_off, npairs)
        least = min(t.numel() for t in rows)
        if npairs:
            order = np.argsort(row_off, kind="stable")
            lo, hi = row_off[order], (row_off + q_len)[order]
            if lo[0] < 0 or hi.max() > least or (lo[1:] < hi[:-1]).any():
                raise ValueError(f"{name}: a pair's rows (q_len at row_off) leave the row tensors or overlap another's")
    open_h = torch.empty((npairs,), device=dev, dtype=torch.float32)
    if npairs == 0:
        return rows[0], rows[1], rows[2], rows[3], row_off, open_h
    t32 = torch.from_numpy(np.stack([s_ld, q_len, x_len, row_base, (fresh != 0).astype(np.int64)]).astype(np.int32)).to(dev)
    t64 = torch.from_numpy(np.stack([np.where(full, s_off, 0), carry_off, row_off])).to(dev)
    nbytes = 4.0 * float((q_len * x_len).sum()) + 16.0 * total + 48.0 * float(x_len.sum())
    halo = ()                            # the entry's arguments behind the carry; the panels' (live until the launch is enqueued)
    if panel_cols is not None:
        hsize = 2 * (q_len + 2)
        hn = int(hsize.sum())
        halo = (torch.from_numpy(np.cumsum(hsize) - hsize).to(dev), torch.empty((hn,), device=dev, dtype=torch.float32),
                torch.empty((hn,), device=dev, dtype=torch.int32), torch.empty((hn,), device=dev, dtype=torch.int32))
        nbytes += 24.0 * float(((x_len + panel_cols - 1) // panel_cols).sum()) * float(hn)
    _tk(None, nbytes, lambda: call(
        "nsid_" + name, _p(S), _p(t64[0]), _p(t32[0]), _p(t32[1]), _p(t32[2]), _p(t32[3]), _p(t32[4]), npairs, int(q_len.max()),
        int(x_len.max()), *(() if panel_cols is None else (panel_cols,)), theta, _p(t64[1]), _p(carry[0]), _p(carry[1]), _p(carry[2]),
        *(_p(t) for t in halo), _p(t64[2]), _p(rows[0]), _p(rows[1]), _p(rows[2]), _p(rows[3]), _p(open_h), _stream()),
        (npairs, int(q_len.max()), int(x_len.max()), 1 if panel_cols is None else panel_cols))
    return rows[0], rows[1], rows[2], rows[3], row_off, open_h


def align_occurrences(row_h, row_j, row_i0, row_j0, row_off, n_rows, first_row, min_score=0.0, top=16, span=None):
    """The occurrences of many runs of rows in one launch (nsid_align_occurrences): run p is rows row_off[p] .. row_off[p] + n_rows[p] - 1
    of the four flat device tensors (local_align_strip's row results, the strips of a run one after the other), its local row r is
    global row first_row[p] + r. Grouping by (row_i0, row_j0), a group's best row, min_score, the order and the unused slots as
    local_align has them. span: per run the rows over which one group can stretch, 2 (x_len - 1) against a song of x_len rows (any
    larger value gives the same output); None: nsid_align_occurrences, whose window is that of a song of ALIGN_MAX_COLS rows; given:
    nsid_align_occurrences_span. Returns (occ (runs, top, 4) int32 = (i0, i1, j0, j1) in global rows, occ_score (runs, top) fp32,
    n_occ (runs,) int32, it can exceed top)."""
    name = "align_occurrences"
    for what, t, dt in zip(("row_h", "row_j", "row_i0", "row_j0"), (row_h, row_j, row_i0, row_j0),
                           (torch.float32, torch.int32, torch.int32, torch.int32)):
        _flat_dev(name, what, t, dt)
    row_off = _align_seq(name, "row_off", row_off)
    npairs = row_off.size
    n_rows, first_row = (_align_seq(name, w, v, npairs) for w, v in (("n_rows", n_rows), ("first_row", first_row)))
    top = int(top)
    if not 1 <= top <= ALIGN_MAX_TOP:
        raise ValueError(f"align_occurrences: top = {top} is outside [1, {ALIGN_MAX_TOP}]")
    min_score = float(min_score)
    if min_score != min_score:
        raise ValueError("align_occurrences: min_score is NaN")
    if npairs and (n_rows.min() < 0 or n_rows.max() > ALIGN_OCC_MAX_ROWS):
        raise ValueError(f"align_occurrences: a run of {int(n_rows.max())} rows is outside [0, {ALIGN_OCC_MAX_ROWS}]")
    if npairs and (first_row.min() < 0 or (first_row + n_rows).max() > 2 ** 31 - 1):
        raise ValueError("align_occurrences: every run needs 0 <= first_row and first_row + n_rows <= 2^31 - 1")
    least = min(t.numel() for t in (row_h, row_j, row_i0, row_j0))
    if npairs and (row_off.min() < 0 or (row_off + n_rows).max() > least):
        raise ValueError("align_occurrences: a run (n_rows at row_off) leaves the row tensors")
    if span is not None:
        span = _align_seq(name, "span", span, npairs)
        if npairs and (span.min() < 0 or span.max() > 2 ** 31 - 1):
            raise ValueError("align_occurrences: every span must be in [0, 2^31 - 1]")
    dev = row_h.device
    occ = torch.empty((npairs, top, 4), device=dev, dtype=torch.int32)
    occ_score = torch.empty((npairs, top), device=dev, dtype=torch.float32)
    n_occ = torch.empty((npairs,), device=dev, dtype=torch.int32)
    if npairs == 0:
        return occ, occ_score, n_occ
    t32 = torch.from_numpy(np.stack([n_rows, first_row] + ([] if span is None else [span])).astype(np.int32)).to(dev)
    t64 = torch.from_numpy(np.ascontiguousarray(row_off)).to(dev)
    entry, with_span = ("nsid_align_occurrences", ()) if span is None else ("nsid_align_occurrences_span", (_p(t32[2]),))
    _tk("align_occurrences_kernel", 16.0 * float(n_rows.sum()), lambda: call(
        entry, _p(row_h), _p(row_j), _p(row_i0), _p(row_j0), _p(t64), _p(t32[0]), _p(t32[1]), *with_span, npairs,
        int(n_rows.max()), min_score, top, _p(occ), _p(occ_score), _p(n_occ), _stream()), (npairs, int(n_rows.max()), 0, top))
    return occ, occ_score, n_occ


ALIGN_PATH_MAX = _H["NSID_ALIGN_PATH_MAX"]             # rows, and columns, of a box of align_paths at most


def align_paths(S, s_off, s_ld, n_rows, n_cols, theta, i_base=None, j_base=None):
    """The paths of many occurrences in one launch (nsid_align_paths), one workgroup per box: box p is the n_rows[p] x n_cols[p] cells
    of an occurrence (i1 - i0 + 1 by j1 - j0 + 1) at S[s_off[p]] with row stride s_ld[p], the rule of include/nsid.h runs on the box
    alone with every cell's step kept, and the steps are followed back from the box's last cell; that is cell for cell the path of the
    whole matrix.

    S: flat fp32 scores on the device. s_off / s_ld / n_rows / n_cols / i_base / j_base: host integer sequences, one entry per box,
    checked here, then uploaded; i_base / j_base (default zeros) are added to the output coordinates. Returns (path_len (boxes,) int32,
    path_off int64 numpy, path_i, path_j int32, path_s fp32, end_h (boxes,) fp32): box p's cells in forward order at path_off[p] + t,
    t < path_len[p], of the three flat tensors, which hold min(n_rows, n_cols) slots per box; the slots past path_len are not
    written. path_len = 0: the box has no row or no column; -1: the box is not an occurrence of this S and theta (its last H is not
    positive, or the trace does not end at its first cell); -2: a side is past ALIGN_PATH_MAX, the box was not read (such a box is
    passed on, not refused, and where it lies is not looked at). end_h: the last cell's H, the occurrence's score bit for bit."""
    name = "align_paths"
    if not isinstance(S, torch.Tensor):
        raise TypeError(f"{name}: S must be a torch tensor on the GPU")
    _chk(S)
    S = S.reshape(-1)
    s_off = _align_seq(name, "s_off", s_off)
    nb = s_off.size
    s_ld, n_rows, n_cols = (_align_seq(name, w, v, nb) for w, v in (("s_ld", s_ld), ("n_rows", n_rows), ("n_cols", n_cols)))
    i_base, j_base = (np.zeros(nb, np.int64) if v is None else _align_seq(name, w, v, nb) for w, v in (("i_base", i_base), ("j_base", j_base)))
    theta = float(theta)
    if theta != theta:
        raise ValueError(f"{name}: theta is NaN")
    if nb and (n_rows.min() < 0 or n_cols.min() < 0):
        raise ValueError(f"{name}: a side is negative")
    if nb and (n_rows.max() >= 2 ** 31 or n_cols.max() >= 2 ** 31):
        raise ValueError(f"{name}: a side does not fit an int32")
    ok = (n_rows <= ALIGN_PATH_MAX) & (n_cols <= ALIGN_PATH_MAX)       # the others get -2 from the kernel, which does not read them
    full = ok & (n_rows > 0) & (n_cols > 0)
    if nb and ok.any() and (i_base[ok].min() < 0 or j_base[ok].min() < 0 or (i_base + n_rows)[ok].max() > 2 ** 31 - 1
                            or (j_base + n_cols)[ok].max() > 2 ** 31 - 1):
        raise ValueError(f"{name}: every box needs 0 <= base and base + side <= 2^31 - 1")
    if nb and full.any() and (s_off[full].min() < 0 or (s_ld[full] < n_cols[full]).any() or s_ld[full].max() >= 2 ** 31
                              or (s_off + (n_rows - 1) * s_ld + n_cols)[full].max() > S.numel()):
        raise ValueError(f"{name}: a box (n_rows rows of s_ld >= n_cols floats) leaves S")
    dev = S.device
    slots = np.where(ok, np.minimum(n_rows, n_cols), 0)
    path_off = np.cumsum(slots) - slots
    dsize = np.asarray([lib.nsid_workspace_bytes(b"align_paths", int(r), int(c)) if f else 0 for r, c, f in zip(n_rows, n_cols, full)],
                       dtype=np.int64)
    dir_off = np.cumsum(dsize) - dsize
    total = int(slots.sum())
    path_len = torch.empty((nb,), device=dev, dtype=torch.int32)
    end_h = torch.empty((nb,), device=dev, dtype=torch.float32)
    path_i = torch.empty((total,), device=dev, dtype=torch.int32)
    path_j = torch.empty((total,), device=dev, dtype=torch.int32)
    path_s = torch.empty((total,), device=dev, dtype=torch.float32)
    if nb == 0:
        return path_len, path_off, path_i, path_j, path_s, end_h
    dirs = torch.empty((max(int(dsize.sum()), 1),), device=dev, dtype=torch.uint8)
    keep = np.where(ok, 1, 0)            # a box past the limit keeps its sides (the kernel answers -2) and nothing else
    t32 = torch.from_numpy(np.stack([np.where(full, s_ld, 0), n_rows, n_cols, i_base * keep, j_base * keep]).astype(np.int32)).to(dev)
    t64 = torch.from_numpy(np.stack([np.where(full | ~ok, s_off, 0), path_off, dir_off])).to(dev)
    max_cols = int(n_cols[ok].max()) if ok.any() else 0
    cells = float((n_rows * n_cols)[full].sum())
    _tk(None, 4.25 * cells + 12.0 * total, lambda: call(
        "nsid_align_paths", _p(S), _p(t64[0]), _p(t32[0]), _p(t32[1]), _p(t32[2]), _p(t32[3]), _p(t32[4]), nb, max_cols, theta,
        _p(t64[1]), _p(t64[2]), _p(dirs), _p(path_len), _p(path_i), _p(path_j), _p(path_s), _p(end_h), _stream()),
        (nb, int(n_rows[ok].max()) if ok.any() else 0, max_cols, 1))
    return path_len, path_off, path_i, path_j, path_s, end_h


# ------------------------------------------------------------------------------------------------ classifier re-rank (csrc/rerank.hip)
CLF_C, CLF_KP, CLF_MAX_N, CLF_QCHUNK = _H["NSID_CLF_C"], _H["NSID_CLF_KP"], _H["NSID_CLF_MAX_N"], _H["NSID_CLF_QCHUNK"]
CLF_WIDTHS = (512, 640, 768, 1024)      # in_dim of the four encoder sizes ('t', 's', 'm', default); 4 heads of C / 4
CLF_PW = _H["NSID_CLF_PW"]               # the folded candidate block P: 4 heads x fc.0's 128, at every width
CLF_MAX_N_EVAL = _H["NSID_CLF_MAX_N_EVAL"]     # the _n entries (multi-tile attention), evaluation and training; the others stay at CLF_MAX_N


def _clf_width(C, name) -> int:
    C = int(C)
    if C not in CLF_WIDTHS:
        raise ValueError(f"{name}: width C = {C} is not one of {CLF_WIDTHS}")
    return C


def clf_node_rows(x, pos=None) -> torch.Tensor:
    """(S, C, N) fp32 node matrices -> (S N, C) node rows, plus pos (N, C) on every segment when given. N <= 32: nsid_clf_node_rows;
    33 <= N <= 128 (C one of CLF_WIDTHS): nsid_clf_node_rows_n"""
    _chk(x, pos)
    if x.dim() != 3:
        raise ValueError(f"clf_node_rows: expected (S, C, N) node matrices, got {tuple(x.shape)}")
    S, C, N = x.shape
    if C % 32 or not 1 <= N <= CLF_MAX_N_EVAL:
        raise ValueError(f"clf_node_rows: C = {C}, N = {N} outside C % 32 == 0, 1 <= N <= {CLF_MAX_N_EVAL}")
    if N > CLF_MAX_N:
        _clf_width(C, "clf_node_rows (N > 32)")
    if pos is not None and tuple(pos.shape) != (N, C):
        raise ValueError(f"clf_node_rows: pos must be ({N}, {C}), got {tuple(pos.shape)}")
    rows = torch.empty((S * N, C), device=x.device, dtype=torch.float32)
    if N > CLF_MAX_N:
        _tk("clf_node_rows_kernel<128>", 8.0 * S * C * N,
            lambda: call("nsid_clf_node_rows_n", _p(x), S, C, N, _p(pos), _p(rows), _stream()), (S, C, N, 1))
        return rows
    _tk("clf_node_rows_kernel", 8.0 * S * C * N, lambda: call("nsid_clf_node_rows", _p(x), S, C, N, _p(pos), _p(rows), _stream()),
        (S, C, N, 1))
    return rows


def _clf_pair_plan(name, q, kp, N, tail, q_start, q_count, cand_off, cand_count, ncand):
    """The checks and the layout that clf_pair_scores and clf_pair_scores_dev (name, for the messages) share: the tensors, N, the
    width and the tail; the groups against the segments of q and a candidate list of ncand entries (cand_off None: the groups' lists
    follow one another); the groups' offsets into the scores and into the launch's workgroups. Returns (out, out_off, plan): the
    unwritten score tensor, the groups' int64 offsets into it and, unless there is nothing to launch, _clf_pair_launch's arguments
    with the tables on the device."""
    _chk(q, kp, tail)
    N = int(N)
    if not 1 <= N <= CLF_MAX_N_EVAL:
        raise ValueError(f"{name}: N = {N} is outside [1, {CLF_MAX_N_EVAL}]")
    if q.dim() != 2 or kp.dim() != 2:
        raise ValueError(f"{name}: expected q (S N, C) and kp (S N, C + {CLF_PW}), got {tuple(q.shape)}, {tuple(kp.shape)}")
    C = _clf_width(q.shape[1], name)
    if q.shape[0] % N or kp.shape[1] != C + CLF_PW or kp.shape[0] % N:
        raise ValueError(f"{name}: expected q (S N, {C}) and kp (S N, {C + CLF_PW}), got {tuple(q.shape)}, {tuple(kp.shape)}")
    if tail.numel() != 257:
        raise ValueError(f"{name}: tail must hold g (128), w2 (128) and b2")
    nq_seg, nc_seg = q.shape[0] // N, kp.shape[0] // N
    qs, qn, cn = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (q_start, q_count, cand_count))
    co = np.cumsum(cn) - cn if cand_off is None else np.asarray(cand_off, dtype=np.int64).reshape(-1)
    G = qs.size
    if not qn.size == co.size == cn.size == G:
        raise ValueError(f"{name}: q_start, q_count{' and' if cand_off is None else ', cand_off and'} cand_count differ in length")
    if G and (qs.min() < 0 or qn.min() < 0 or (qs + qn).max() > nq_seg or co.min() < 0 or cn.min() < 0 or (co + cn).max() > ncand):
        raise ValueError(f"{name}: a group's query range or candidate list is out of range")
    sizes = qn * cn
    out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    tiles = cn * ((qn + CLF_QCHUNK - 1) // CLF_QCHUNK)
    tile_off = np.concatenate([[0], np.cumsum(tiles)]).astype(np.int64)
    # grp and tile_off are int32 on the device
    if tile_off[-1] >= 2 ** 31 or max(nq_seg, nc_seg) * N >= 2 ** 31 or (G and (co + cn).max() >= 2 ** 31):
        raise ValueError(f"{name}: too many pairs for one call")
    out = torch.empty((int(out_off[-1]),), device=q.device, dtype=torch.float32)
    if G == 0 or tile_off[-1] == 0:
        return out, out_off[:-1], None
    dev = q.device
    grp = torch.from_numpy(np.stack([qs, qn, co, cn], 1).astype(np.int32).reshape(-1)).to(dev)
    oo = torch.from_numpy(out_off[:-1].copy()).to(dev)
    to = torch.from_numpy(tile_off.astype(np.int32)).to(dev)
    return out, out_off[:-1], (N, C, nq_seg, nc_seg, grp, oo, to, G, int(tile_off[-1]), float(sizes.sum()))


def _clf_pair_launch(q, kp, tail, out, plan, cidx):
    """one launch of a _clf_pair_plan over the int32 device candidate list cidx: nsid_clf_pair_scores_c for N <= 32, else _n"""
    N, C, nq_seg, nc_seg, grp, oo, to, G, ntiles, npairs = plan
    if N > CLF_MAX_N:
        # 33 <= N <= 128, per pair: Q K^T 2 N^2 C on the matrix pipe, the softmax (about 8 per attention weight) and the column sums
        # 4 N^2 each, a P 2 N 512, the tail 512. Bytes: the scores; per workgroup the candidate's P once; per pair the Q rows once per
        # head and the K rows once per query tile (both stream from L2)
        nt = (N + 31) // 32
        kernel, entry = "clf_pair_wide_kernel", "nsid_clf_pair_scores_n"
        flops = (2.0 * N * N * C + 12.0 * 4 * N * N + 2.0 * N * CLF_PW + 512.0) * npairs
        nbytes = 4.0 * npairs + 4.0 * CLF_PW * N * float(ntiles) + 4.0 * N * C * (1 + nt) * npairs
    else:
        # per pair 2 N^2 C (Q K^T on the matrix pipe) + softmax, a P and the folded tail: 1.2 MFLOP at C = 512; bytes: the scores and
        # K / P staged per workgroup
        kernel, entry = "clf_pair_kernel", "nsid_clf_pair_scores_c"
        flops = (1.2e6 + 2.0 * CLF_MAX_N * CLF_MAX_N * (C - CLF_C)) * npairs
        nbytes = 4.0 * npairs + 4.0 * (C + CLF_PW) * N * float(ntiles)
    _timed(kernel, flops, nbytes,
           lambda: call(entry, _p(q), nq_seg, _p(kp), nc_seg, C, N, _p(grp), _p(oo), _p(to), G, ntiles, _p(cidx), _p(tail), _p(out),
                        out.numel(), _stream()), (G, int(npairs), N, 1))


def clf_pair_scores(q, kp, N, tail, q_start, q_count, cand_idx, cand_off, cand_count):
    """Scores of blocked pair lists on the classifier's folded form (csrc/rerank.hip).

    q (nq_seg N, C): projected query rows; kp (nc_seg N, C + 512): the candidates' [K | P] rows; tail (257,): {g, w2, b2}. C is
    q's width, one of CLF_WIDTHS. 1 <= N <= CLF_MAX_N_EVAL nodes per segment: N <= 32 runs nsid_clf_pair_scores_c (one 32 x 32 tile per
    head), 33 .. 128 nsid_clf_pair_scores_n (up to 4 x 4 tiles); the lists and the result have the same form in both.
    Group i pairs query segments [q_start[i], q_start[i] + q_count[i]) with the candidate segments cand_idx[cand_off[i] :
    cand_off[i] + cand_count[i]] (repeats allowed). Host integer sequences, checked here. Returns (out, out_off): the flat fp32
    score tensor and, per group, the int64 offset of its row-major (q_count x cand_count) block."""
    ci = np.asarray(cand_idx, dtype=np.int64).reshape(-1)
    out, out_off, plan = _clf_pair_plan("clf_pair_scores", q, kp, N, tail, q_start, q_count, cand_off, cand_count, ci.size)
    nc_seg = kp.shape[0] // int(N)
    if ci.size and (ci.min() < 0 or ci.max() >= nc_seg):
        raise ValueError(f"clf_pair_scores: candidate indices must lie in [0, {nc_seg})")
    if plan is not None:
        _clf_pair_launch(q, kp, tail, out, plan, torch.from_numpy(ci.astype(np.int32)).to(q.device))
    return out, out_off


def clf_pair_scores_dev(q, kp, N, tail, q_start, q_count, cand_count, cidx):
    """clf_pair_scores with the candidate lists on the device: cidx is a 1-D int32 device tensor (vote_candidates of a search result)
    that holds the groups' lists one after the other, so group i's list starts at the running sum of cand_count. The host still owns
    every size (q_start, q_count, cand_count: host integer sequences, checked here); the entries of cidx are not read by the host:
    the kernels skip, and leave unwritten, a pair whose candidate lies outside [0, nc_seg). Same kernels, same scores and the same
    result form as clf_pair_scores: (out, out_off)."""
    _clf_idx(cidx, "clf_pair_scores_dev cidx")
    # cand_off None: group i's list starts at the running sum of cand_count, so the lists fit when cand_count.sum() <= cidx.numel()
    out, out_off, plan = _clf_pair_plan("clf_pair_scores_dev", q, kp, N, tail, q_start, q_count, None, cand_count, cidx.numel())
    if plan is not None:
        _clf_pair_launch(q, kp, tail, out, plan, cidx)
    return out, out_off


# ------------------------------------------------------------------------------------------------ classifier training (csrc/clf_train.hip)
CLF_HID, CLF_H = _H["NSID_CLF_HID"], _H["NSID_CLF_H"]
CLF_MINE_MAX_ROWS, CLF_MINE_MAX_D = _H["NSID_CLF_MINE_MAX_ROWS"], _H["NSID_CLF_MINE_MAX_D"]


def _clf_idx(t, name):
    if t.dtype != torch.int32 or t.dim() != 1 or not t.is_cuda or not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous 1-D int32 device tensor")


def clf_mine_hard_negatives(zq, za, k) -> torch.Tensor:
    """(nq, d) x (na, d) fp32 -> (nq, k) int64: ranks 1..k of each row of zq za^T in descending order, ties to the smaller index"""
    _chk(zq, za)
    if zq.dim() != 2 or za.dim() != 2 or zq.shape[1] != za.shape[1]:
        raise ValueError(f"clf_mine_hard_negatives: expected (nq, d) and (na, d), got {tuple(zq.shape)}, {tuple(za.shape)}")
    nq, d = zq.shape
    na, k = za.shape[0], int(k)
    if not (4 <= d <= CLF_MINE_MAX_D and d % 4 == 0):
        raise ValueError(f"clf_mine_hard_negatives: d = {d} is outside 4 <= d <= {CLF_MINE_MAX_D}, d % 4 == 0")
    if not 1 <= na <= CLF_MINE_MAX_ROWS:
        raise ValueError(f"clf_mine_hard_negatives: {na} pool rows are outside [1, {CLF_MINE_MAX_ROWS}]")
    if not 1 <= k <= na - 1:
        raise ValueError(f"clf_mine_hard_negatives: ranks 1..{k} need at least {k + 1} pool rows, got {na}")
    out = torch.empty((nq, k), device=zq.device, dtype=torch.int64)
    _timed("clf_mine_kernel", 2.0 * nq * na * d, 4.0 * (nq * d + float(nq) * na * d) + 8.0 * nq * k, lambda: call(
        "nsid_clf_mine_hard_negatives", _p(zq), nq, _p(za), na, d, k, _p(out), _stream()), (nq, na, d, 1))
    return out


def _clf_qkv_width(q, kv, N, name, max_n=CLF_MAX_N) -> int:
    """C of Q rows (S N, C) and [K | V] rows (S N, 2 C), checked against the supported widths before any launch"""
    N = int(N)
    if not 1 <= N <= max_n:
        raise ValueError(f"{name}: N = {N} is outside [1, {max_n}]")
    if q.dim() != 2 or kv.dim() != 2 or kv.shape[1] % 2:
        raise ValueError(f"{name}: expected q (S N, C) and kv (S N, 2 C), got {tuple(q.shape)}, {tuple(kv.shape)}")
    C = _clf_width(kv.shape[1] // 2, name)
    if q.shape[1] != C or q.shape[0] % N or kv.shape[0] % N:
        raise ValueError(f"{name}: expected q (S N, {C}) and kv (S N, {2 * C}), got {tuple(q.shape)}, {tuple(kv.shape)}")
    return C


def _clf_tiles(N) -> int:
    return (int(N) + CLF_MAX_N - 1) // CLF_MAX_N


# The attention and the per-segment sums have two forms each: N <= CLF_MAX_N nodes (one 32 x 32 tile per head; the _c entries) and
# 1 <= N <= CLF_MAX_N_EVAL (nT x nT tiles, the *_wide_kernel forms of clf_train.hip; the _n entries, public names with _n). One body
# per operation holds the checks and the allocations; name is the public function (messages), wide its form.
def _clf_attn_fwd(name, wide, q, kv, N, qi, ci):
    _chk(q, kv)
    _clf_idx(qi, name)
    _clf_idx(ci, name)
    C = _clf_qkv_width(q, kv, N, name, CLF_MAX_N_EVAL if wide else CLF_MAX_N)
    N = int(N)
    P, nT = qi.numel(), _clf_tiles(N)
    dev = q.device
    obar = torch.empty((P, C), device=dev, dtype=torch.float32)
    attn = torch.empty((P, CLF_H, nT, nT, 16, 64) if wide else (P, CLF_H, 16, 64), device=dev, dtype=torch.float32)
    abar = torch.empty((P, CLF_H, CLF_MAX_N_EVAL if wide else CLF_MAX_N), device=dev, dtype=torch.float32)
    # 2 N^2 C (Q K^T) + 2 N C (a V) per pair. Bytes: obar, attn, abar written; read per pair (from L2 mostly) Q, K, V rows once, wide:
    # Q once per head, K once per query tile, V
    if wide:
        kernel, entry = "clf_attn_fwd_wide_kernel", "nsid_clf_attn_fwd_n"
        nbytes = float(P) * (4.0 * N * C * (2 + nT) + 4.0 * C + 4.0 * CLF_H * (32 * nT) ** 2 + 4.0 * CLF_H * CLF_MAX_N_EVAL)
    else:
        kernel, entry = "clf_attn_fwd_kernel", "nsid_clf_attn_fwd_c"
        nbytes = float(P) * (12.0 * N * C + 4.0 * C + 4.0 * CLF_H * 16 * 64 + 4.0 * CLF_H * CLF_MAX_N)
    _timed(kernel, float(P) * (2.0 * N * N * C + 2.0 * N * C), nbytes, lambda: call(
        entry, _p(q), q.shape[0] // N, _p(kv), kv.shape[0] // N, C, N, _p(qi), _p(ci), P, _p(obar), _p(attn), _p(abar), _stream()),
        (P, N, C, 1))
    return obar, attn, abar


def _clf_attn_bwd(name, wide, dobar, attn, q, kv, N, qi, ci):
    _chk(dobar, attn, q, kv)
    _clf_idx(qi, name)
    _clf_idx(ci, name)
    C = _clf_qkv_width(q, kv, N, name, CLF_MAX_N_EVAL if wide else CLF_MAX_N)
    N = int(N)
    P, nT = qi.numel(), _clf_tiles(N)
    if tuple(dobar.shape) != (P, C) or attn.numel() != P * CLF_H * (32 * nT) ** 2:
        raise ValueError(f"{name}: expected dobar ({P}, {C}) and attn ({P}, 4, {f'{nT}, {nT}, ' if wide else ''}16, 64), got "
                         f"{tuple(dobar.shape)}, {tuple(attn.shape)}")
    dev = q.device
    dq = torch.empty((P, N, C), device=dev, dtype=torch.float32)
    dk = torch.empty((P, N, C), device=dev, dtype=torch.float32)
    # 2 N C (da) + 2 N^2 C (dQ) + 2 N^2 C (dK) per pair on the matrix side. Bytes: dQ, dK written; Q, K, V, attn read, wide: V and attn
    # once, K once per query tile, Q once per key tile
    if wide:
        kernel, entry = "clf_attn_bwd_wide_kernel", "nsid_clf_attn_bwd_n"
        nbytes = float(P) * (4.0 * N * C * (1 + 2 * nT) + 4.0 * C + 4.0 * CLF_H * (32 * nT) ** 2 + 8.0 * N * C)
    else:
        kernel, entry = "clf_attn_bwd_kernel", "nsid_clf_attn_bwd_c"
        nbytes = float(P) * (12.0 * N * C + 4.0 * C + 4.0 * CLF_H * 16 * 64 + 8.0 * N * C)
    _timed(kernel, float(P) * (4.0 * N * N * C + 2.0 * N * C), nbytes, lambda: call(
        entry, _p(dobar), _p(attn), _p(q), q.shape[0] // N, _p(kv), kv.shape[0] // N, C, N, _p(qi), _p(ci), P, _p(dq), _p(dk),
        _stream()), (P, N, C, 1))
    return dq, dk


def _clf_seg_reduce(name, wide, dq, dk, abar, dobar, qi, ci, N, nq_seg, nc_seg):
    _chk(dq, dk, abar, dobar)
    _clf_idx(qi, name)
    _clf_idx(ci, name)
    P = qi.numel()
    N = int(N)
    max_n = CLF_MAX_N_EVAL if wide else CLF_MAX_N          # also abar's row: (P, 4, max_n)
    if not 1 <= N <= max_n:
        raise ValueError(f"{name}: N = {N} is outside [1, {max_n}]")
    if dobar.dim() != 2:
        raise ValueError(f"{name}: expected dobar (P, C), got {tuple(dobar.shape)}")
    C = _clf_width(dobar.shape[1], name)
    if dobar.shape[0] != P or dq.numel() != P * N * C or dk.numel() != P * N * C or abar.numel() != P * CLF_H * max_n:
        raise ValueError(f"{name}: expected dq, dk ({P}, {N}, {C}), abar ({P}, 4, {max_n}) and dobar ({P}, {C}), got "
                         f"{tuple(dq.shape)}, {tuple(dk.shape)}, {tuple(abar.shape)}, {tuple(dobar.shape)}")
    dev = dq.device
    dq_seg = torch.empty((nq_seg * N, C), device=dev, dtype=torch.float32)
    dkv_seg = torch.empty((nc_seg * N, 2 * C), device=dev, dtype=torch.float32)
    # wide: every node tile of a segment scans the pair list and reads dobar again
    nT = _clf_tiles(N) if wide else 1
    kernel, entry = ("clf_seg_reduce_wide_kernel", "nsid_clf_seg_reduce_n") if wide else ("clf_seg_reduce_kernel", "nsid_clf_seg_reduce_c")
    _tk(kernel, float(P) * (8.0 * N * C + 4.0 * C * nT) + 4.0 * (nq_seg + nc_seg) * (P * nT + N * C) + 4.0 * nc_seg * N * C,
        lambda: call(entry, _p(dq), _p(dk), _p(abar), _p(dobar), _p(qi), _p(ci), P, C, N, nq_seg, nc_seg, _p(dq_seg), _p(dkv_seg),
                     _stream()), (P, N, nq_seg + nc_seg, 1))
    return dq_seg, dkv_seg


def clf_attn_fwd(q, kv, N, qi, ci):
    """per pair (qi[p], ci[p]): (obar (P, C), attn (P, 4, 16, 64), abar (P, 4, 32)); q (Sq N, C) Q rows, kv (Sc N, 2 C) [K | V]
    rows, C one of CLF_WIDTHS; qi, ci int32 device lists, in range (checked by the caller)"""
    return _clf_attn_fwd("clf_attn_fwd", False, q, kv, N, qi, ci)


def clf_attn_fwd_n(q, kv, N, qi, ci):
    """clf_attn_fwd for 1 <= N <= 128: (obar (P, C), attn (P, 4, nT, nT, 16, 64), abar (P, 4, 128)), nT = ceil(N / 32)"""
    return _clf_attn_fwd("clf_attn_fwd_n", True, q, kv, N, qi, ci)


def clf_attn_bwd(dobar, attn, q, kv, N, qi, ci):
    """per-pair (dQ (P, N, C), dK (P, N, C)) from dobar (P, C) = dL/dobar and the forward's attn"""
    return _clf_attn_bwd("clf_attn_bwd", False, dobar, attn, q, kv, N, qi, ci)


def clf_attn_bwd_n(dobar, attn, q, kv, N, qi, ci):
    """clf_attn_bwd for 1 <= N <= 128, from clf_attn_fwd_n's attn: per-pair (dQ (P, N, C), dK (P, N, C))"""
    return _clf_attn_bwd("clf_attn_bwd_n", True, dobar, attn, q, kv, N, qi, ci)


def clf_seg_reduce(dq, dk, abar, dobar, qi, ci, N, nq_seg, nc_seg):
    """per-segment sums in pair order: (dQ (nq_seg N, C), [dK | dV] (nc_seg N, 2 C)); C is dobar's width (P, C)"""
    return _clf_seg_reduce("clf_seg_reduce", False, dq, dk, abar, dobar, qi, ci, N, nq_seg, nc_seg)


def clf_seg_reduce_n(dq, dk, abar, dobar, qi, ci, N, nq_seg, nc_seg):
    """clf_seg_reduce for 1 <= N <= 128, abar (P, 4, 128) from clf_attn_fwd_n: (dQ (nq_seg N, C), [dK | dV] (nc_seg N, 2 C))"""
    return _clf_seg_reduce("clf_seg_reduce_n", True, dq, dk, abar, dobar, qi, ci, N, nq_seg, nc_seg)


def clf_head_fwd(hid, keep, w2, b2) -> torch.Tensor:
    """(P, 128) pre-activations and keep mask -> (P,) sigmoid(w2 . (relu(hid) keep) + b2)"""
    _chk(hid, keep, w2, b2)
    P = hid.shape[0]
    s = torch.empty((P,), device=hid.device, dtype=torch.float32)
    _tk("clf_head_fwd_kernel", 8.0 * P * CLF_HID + 4.0 * P, lambda: call(
        "nsid_clf_head_fwd", _p(hid), _p(keep), _p(w2), _p(b2), P, _p(s), _stream()), (P, CLF_HID, 1, 1))
    return s


def clf_head_bwd(ds, s, hid, keep, w2):
    """-> (dH (P, 128), dz (P,), dw2 (128,), db2 (1,)), the weight gradients in pair order"""
    _chk(ds, s, hid, keep, w2)
    P = hid.shape[0]
    dev = hid.device
    dh = torch.empty((P, CLF_HID), device=dev, dtype=torch.float32)
    dz = torch.empty((P,), device=dev, dtype=torch.float32)
    dw2 = torch.empty((CLF_HID,), device=dev, dtype=torch.float32)
    db2 = torch.empty((1,), device=dev, dtype=torch.float32)
    _tk("clf_head_bwd_kernel", 20.0 * P * CLF_HID + 12.0 * P, lambda: call(
        "nsid_clf_head_bwd", _p(ds), _p(s), _p(hid), _p(keep), _p(w2), P, _p(dh), _p(dz), _p(dw2), _p(db2), _stream()),
        (P, CLF_HID, 1, 1))
    return dh, dz, dw2, db2


# ------------------------------------------------------------------------------------------------ ResNet-IBN baseline (csrc/resnet.hip)
GEM_EPS = 1e-6
IN_EPS = 1e-5


def conv_out_size(n: int, ksize: int, stride: int) -> int:
    """output extent of Conv2d(ksize, stride, padding=ksize // 2) (and of MaxPool2d(3, 2, 1), Conv2d(7, 2, 3)) on an extent of n"""
    return (n + 2 * (ksize // 2) - ksize) // stride + 1


def pack_conv_bn(w, gamma=None, beta=None, running_mean=None, running_var=None, eps=BN_EPS):
    """Host routine (torch ops on whatever device the tensors live on; once per checkpoint, off the hot path): conv weight
    (Cout, C, KH, KW) -> the packed (Cout, KH*KW*C) matrix nsid_conv2d_fwd reads (tap-major, channel fastest), with the eval-mode
    BatchNorm behind the conv folded in: BN(conv(x)) = conv_{s w}(x) + (beta - mean s), s = gamma / sqrt(var + eps).
    Returns (packed weight, bias); gamma None: no BatchNorm, bias None."""
    with torch.no_grad():
        wp = w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], -1)
        if gamma is None:
            return wp.contiguous(), None
        s = gamma.detach() / torch.sqrt(running_var + eps)
        return (wp * s[:, None]).contiguous(), (beta.detach() - running_mean * s).contiguous()


def packed_conv_bn(conv_w, gamma, beta, running_mean, running_var, eps=BN_EPS):
    """pack_conv_bn through the _FOLDED cache (keyed by the versions of the five tensors and the state epochs; bf16 shadow included)"""
    return folded_conv_bn(lambda: pack_conv_bn(conv_w)[0], None, gamma, beta, running_mean, running_var, eps, source=conv_w)


def conv2d_fwd(x, B, H, W, C, wp, bias, Cout, ksize, stride=1, addend=None, relu=False) -> torch.Tensor:
    """x (B*H*W, C) rows -> (B*Ho*Wo, Cout) rows; wp (Cout, ksize*ksize*C) fp32 packed (pack_conv_bn): its bf16 shadow is the
    operand under bf16 storage"""
    _chk(wp, bias)
    dt = _act(x, addend)
    Ho, Wo = conv_out_size(H, ksize, stride), conv_out_size(W, ksize, stride)
    M, K = B * Ho * Wo, ksize * ksize * C
    if tuple(x.shape) != (B * H * W, C) or tuple(wp.shape) != (Cout, K) or (addend is not None and tuple(addend.shape) != (M, Cout)):
        raise ValueError(f"conv2d_fwd: x {tuple(x.shape)} / wp {tuple(wp.shape)} do not match B={B} H={H} W={W} C={C} Cout={Cout} k={ksize}")
    out = torch.empty((M, Cout), device=x.device, dtype=x.dtype)
    wop = SHADOWS.operand(wp) if dt == BF16 else wp
    esz = x.element_size()
    _timed("conv2d_fwd_kernel<%dx%d,s%d>" % (ksize, ksize, stride), 2.0 * M * Cout * K,
           esz * (B * H * W * C + M * Cout * (2 if addend is not None else 1)) + float(wop.element_size()) * Cout * K,
           lambda: call("nsid_conv2d_fwd", _p(x), B, H, W, C, _p(wop), dt, _p(bias), _p(addend), _p(out), Cout, ksize, stride,
                        ACT_RELU if relu else ACT_NONE, dt, _stream()), (M, Cout, K, 1))
    return out


def ibn_relu_fwd(x, B, HW, C, in_gamma, in_beta, bn_aff: "BNAffine", eps=IN_EPS, out=None) -> torch.Tensor:
    """relu(IBN(x)) on rows (B*HW, C): instance norm (this clip's statistics) on channels [0, C/2), the eval BatchNorm affine on the rest"""
    _chk(in_gamma, in_beta, bn_aff.scale, bn_aff.shift)
    dt = _act(x, out)
    if tuple(x.shape) != (B * HW, C) or in_gamma.numel() != C // 2 or bn_aff.scale.numel() != C - C // 2:
        raise ValueError("ibn_relu_fwd: shapes do not match")
    if out is None:
        out = torch.empty_like(x)
    _tk("ibn_relu_kernel", 4.0 * x.element_size() * x.numel(), lambda: call(
        "nsid_ibn_relu_fwd", _p(x), B, HW, C, _p(in_gamma), _p(in_beta), eps, _p(bn_aff.scale), _p(bn_aff.shift), _p(out), dt,
        _stream()), (B * HW, C, 0, 1))
    return out


def stem7_pool_fwd(x, w49, bias, out_dtype=torch.float32):
    """x (B, H, W) fp32 -> (rows (B*Hp*Wp, 64), Hp, Wp): Conv 7x7 s2 p3 (w49: (64, 49), BatchNorm folded) + ReLU + MaxPool 3x3 s2 p1"""
    _chk(x, w49, bias)
    B, H, W = x.shape
    Hp, Wp = conv_out_size(conv_out_size(H, 7, 2), 3, 2), conv_out_size(conv_out_size(W, 7, 2), 3, 2)
    if tuple(w49.shape) != (64, 49) or bias.numel() != 64:
        raise ValueError("stem7_pool_fwd: the stem is Conv2d(1, 64, 7)")
    out = torch.empty((B * Hp * Wp, 64), device=x.device, dtype=out_dtype)
    _timed("stem7_pool_kernel", 2.0 * 49 * 64 * B * conv_out_size(H, 7, 2) * conv_out_size(W, 7, 2),
           4.0 * x.numel() + float(out.element_size()) * out.numel(), lambda: call(
        "nsid_stem7_pool_fwd", _p(x), B, H, W, _p(w49), _p(bias), _p(out), _act(out), _stream()), (B * Hp * Wp, 64, 49, 1))
    return out, Hp, Wp


def gem_pool_fwd(x, B, HW, C, p, eps=GEM_EPS) -> torch.Tensor:
    """rows (B*HW, C) -> (B, C) fp32 generalised-mean pooling; p: the (1,) parameter, read on the device"""
    _chk(p)
    dt = _act(x)
    if tuple(x.shape) != (B * HW, C) or p.numel() != 1:
        raise ValueError("gem_pool_fwd: shapes do not match")
    out = torch.empty((B, C), device=x.device, dtype=torch.float32)
    _tk("gem_pool_kernel", float(x.element_size()) * x.numel(), lambda: call(
        "nsid_gem_pool_fwd", _p(x), B, HW, C, _p(p), eps, _p(out), dt, _stream()), (B * HW, C, 0, 1))
    return out


def gem_pool_bwd(x, dy, B, HW, C, p, eps=GEM_EPS):
    """backward of gem_pool_fwd: rows x (B*HW, C) fp32 or bf16, dy (B, C) fp32 -> (dx (B*HW, C) fp32, dp (1,))"""
    _chk(p, dy)
    dt = _act(x)
    if tuple(x.shape) != (B * HW, C) or tuple(dy.shape) != (B, C) or p.numel() != 1:
        raise ValueError("gem_pool_bwd: shapes do not match")
    dx = torch.empty((B * HW, C), device=x.device, dtype=torch.float32)
    part = torch.empty((B * ((C + 63) // 64),), device=x.device, dtype=torch.float32)
    dp = torch.empty((1,), device=x.device, dtype=torch.float32)
    _tk("gem_pool_bwd_kernel", float(2 * x.element_size() + 4) * x.numel(), lambda: call(
        "nsid_gem_pool_bwd", _p(x), _p(dy), B, HW, C, _p(p), eps, _p(dx), _p(part), _p(dp), dt, _stream()), (B * HW, C, 0, 1))
    return dx, dp


# ------------------------------------------------------------------------------------------------ ResNet-IBN baseline, training
# Packed conv weights WITHOUT a BatchNorm folded in (training mode normalises with batch statistics): the forward packing of
# pack_conv_bn and the backward-data packing, cached per weight tensor until its version or the weight epoch moves.
_PACKED = {}      # (id(conv_w), kind) -> (weakref(conv_w), (data_ptr, version, WEIGHT_EPOCH), packed)


def pack_conv_bwd(w) -> torch.Tensor:
    """Host routine: conv weight (Cout, C, KH, KW) -> the (C, KH*KW*Cout) matrix nsid_conv2d_bwd_data reads (tap-major, Cout fastest)"""
    with torch.no_grad():
        return w.detach().permute(1, 2, 3, 0).reshape(w.shape[1], -1).contiguous()


def unpack_conv_wgrad(dwp, C, ksize) -> torch.Tensor:
    """Host routine: the packed gradient (Cout, KH*KW*C) of nsid_conv2d_bwd_weight -> conv.weight's (Cout, C, KH, KW)"""
    return dwp.view(dwp.shape[0], ksize, ksize, C).permute(0, 3, 1, 2).contiguous()


def _packed(conv_w, kind):
    import weakref
    key = (id(conv_w), kind)
    versions = (conv_w.data_ptr(), conv_w._version, WEIGHT_EPOCH)
    e = _PACKED.get(key)
    if e is not None and e[0]() is conv_w and e[1] == versions:
        return e[2]
    wp = pack_conv_bn(conv_w)[0] if kind == "fwd" else pack_conv_bwd(conv_w)
    if wp.numel() % 8 == 0:
        SHADOWS.register(wp, f32_to_bf16(wp), owner=wp, fresh=True)
    if not torch.cuda.is_current_stream_capturing():    # as folded_conv_bn: nothing is inserted under capture, an earlier entry is used
        _cache_constants(_PACKED, key, (weakref.ref(conv_w), versions, wp))
    return wp


def packed_conv(conv_w) -> torch.Tensor:
    """pack_conv_bn(conv_w) without a BatchNorm, cached (bf16 shadow included)"""
    return _packed(conv_w, "fwd")


def packed_conv_bwd(conv_w) -> torch.Tensor:
    """pack_conv_bwd(conv_w), cached (bf16 shadow included)"""
    return _packed(conv_w, "bwd")


def conv2d_bwd_data(dy, B, H, W, C, wt, Cout, ksize, stride=1, addend=None) -> torch.Tensor:
    """gradient of conv2d_fwd's input: dy (B*Ho*Wo, Cout) rows -> dx (B*H*W, C) rows (+ addend); wt (C, ksize*ksize*Cout) fp32 from
    pack_conv_bwd: its bf16 shadow is the operand under bf16 storage"""
    _chk(wt)
    dt = _act(dy, addend)
    Ho, Wo = conv_out_size(H, ksize, stride), conv_out_size(W, ksize, stride)
    M, K = B * H * W, ksize * ksize * Cout
    if tuple(dy.shape) != (B * Ho * Wo, Cout) or tuple(wt.shape) != (C, K) or (addend is not None and tuple(addend.shape) != (M, C)):
        raise ValueError(f"conv2d_bwd_data: dy {tuple(dy.shape)} / wt {tuple(wt.shape)} do not match B={B} H={H} W={W} C={C} "
                         f"Cout={Cout} k={ksize} s={stride}")
    dx = torch.empty((M, C), device=dy.device, dtype=dy.dtype)
    wop = SHADOWS.operand(wt) if dt == BF16 else wt
    esz = dy.element_size()
    _timed("conv2d_bwd_data_kernel<%dx%d,s%d>" % (ksize, ksize, stride), 2.0 * M * C * K,
           esz * (B * Ho * Wo * Cout + M * C * (2 if addend is not None else 1)) + float(wop.element_size()) * C * K,
           lambda: call("nsid_conv2d_bwd_data", _p(dy), B, H, W, C, _p(wop), dt, _p(addend), _p(dx), Cout, ksize, stride, dt,
                        _stream()), (M, C, K, 1))
    return dx


def conv2d_bwd_weight(dy, x, dwp, B, H, W, C, Cout, ksize, stride=1) -> None:
    """dwp += the packed weight gradient (Cout, ksize*ksize*C) fp32 of conv2d_fwd (unpack_conv_wgrad turns it into conv.weight's layout)"""
    _chk(dwp)
    dt = _act(dy, x)
    Ho, Wo = conv_out_size(H, ksize, stride), conv_out_size(W, ksize, stride)
    M, K = B * Ho * Wo, ksize * ksize * C
    if tuple(dy.shape) != (M, Cout) or tuple(x.shape) != (B * H * W, C) or tuple(dwp.shape) != (Cout, K):
        raise ValueError(f"conv2d_bwd_weight: dy {tuple(dy.shape)} / x {tuple(x.shape)} / dw {tuple(dwp.shape)} do not match B={B} "
                         f"H={H} W={W} C={C} Cout={Cout} k={ksize} s={stride}")
    nws = lib.nsid_workspace_bytes(b"conv2d_bwd_weight", M, Cout * K)
    ws = torch.empty((nws // 4,), device=dy.device, dtype=torch.float32) if nws > 0 else None
    esz = dy.element_size()
    _timed("conv2d_wgrad_kernel<%dx%d,s%d>" % (ksize, ksize, stride), 2.0 * M * Cout * K,
           esz * (M * Cout + B * H * W * C) + 8.0 * Cout * K + 2.0 * nws,
           lambda: call("nsid_conv2d_bwd_weight", _p(dy), _p(x), B, H, W, C, _p(dwp), _p(ws), Cout, ksize, stride, dt, _stream()),
           (M, Cout, K, 1))


def col_stat(x, M, C) -> torch.Tensor:
    """per-channel sum and sum of squares of rows x (M, C) (a column slice of a wider matrix is fine) per 128-row tile:
    the (2, row_tiles(M), C) fp32 buffer bn_finalize reads. One launch."""
    if not x.is_cuda:
        raise RuntimeError("neuralsampleid_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
    if x.dtype not in (torch.float32, torch.bfloat16) or x.dim() != 2 or x.stride(1) != 1 or tuple(x.shape) != (M, C):
        raise RuntimeError(f"col_stat: expected float32/bfloat16 rows ({M}, {C}) with unit column stride, got {x.dtype} {tuple(x.shape)}")
    dt = BF16 if x.dtype == torch.bfloat16 else F32
    stat = torch.empty((2, row_tiles(M), C), device=x.device, dtype=torch.float32)
    _tk("col_stat_kernel", float(x.element_size()) * M * C, lambda: call(
        "nsid_col_stat", _p(x), x.stride(0), M, C, _p(stat), dt, _stream()), (M, C, 0, 1))
    return stat


def _stem_dims(x, w):
    if not x.is_cuda:
        raise RuntimeError("neuralsampleid_amd ops need tensors on the MI355X (cuda) device; there is no CPU path")
    if x.dim() != 3 or tuple(w.shape) != (64, 49):
        raise ValueError("the stem is Conv2d(1, 64, 7) on (B, H, W) segments: w (64, 49)")
    B, H, W = x.shape
    Hc, Wc = conv_out_size(H, 7, 2), conv_out_size(W, 7, 2)
    return B, H, W, Hc, Wc, conv_out_size(Hc, 3, 2), conv_out_size(Wc, 3, 2)


def stem7_stat(x, w49):
    """x (B, H, W) fp32, w49 (64, 49) the RAW conv1 weight -> (stat, tiles, N): per-channel sum and sum of squares of the raw 7x7
    stride-2 conv output over its N = B*Hc*Wc pixels as (2, tiles, 64) partial sums: bn_finalize(stat, N, ..., tiles=tiles). The conv
    output is not stored. One launch."""
    _chk(x, w49)
    B, H, W, Hc, Wc, Hp, Wp = _stem_dims(x, w49)
    tiles = int(lib.nsid_stem7_partials(B * Hp, Wp, 0))
    stat = torch.empty((2, tiles, 64), device=x.device, dtype=torch.float32)
    _timed("stem7_stat_kernel", 2.0 * 49 * 64 * B * Hc * Wc, 4.0 * x.numel() + 4.0 * stat.numel(), lambda: call(
        "nsid_stem7_stat", _p(x), B, H, W, _p(w49), _p(stat), _stream()), (B * Hc * Wc, 64, 49, 1))
    return stat, tiles, B * Hc * Wc


def stem7_pool_train_fwd(x, w49, aff: "BNAffine", out_dtype=torch.float32):
    """training-mode stem forward: x (B, H, W) fp32 -> (rows (B*Hp*Wp, 64), Hp, Wp) with the BATCH affine aff (bn_finalize of
    stem7_stat) folded into the raw weight w49 on the device (no host read), then stem7_pool_fwd's kernel"""
    _chk(x, w49, aff.scale, aff.shift)
    B, H, W, Hc, Wc, Hp, Wp = _stem_dims(x, w49)
    if aff.scale.numel() != 64:
        raise ValueError("stem7_pool_train_fwd: the stem is Conv2d(1, 64, 7)")
    out = torch.empty((B * Hp * Wp, 64), device=x.device, dtype=out_dtype)
    wf = torch.empty((64, 49), device=x.device, dtype=torch.float32)
    _timed("stem7_pool_kernel<train>", 2.0 * 49 * 64 * B * Hc * Wc, 4.0 * x.numel() + float(out.element_size()) * out.numel(),
           lambda: call("nsid_stem7_pool_train_fwd", _p(x), B, H, W, _p(w49), _p(aff.scale), _p(aff.shift), _p(wf), _p(out),
                        _act(out), _stream()), (B * Hp * Wp, 64, 49, 1))
    return out, Hp, Wp


def stem7_bwd(dpool, x, w49, aff: "BNAffine", gamma):
    """backward of the training-mode stem: dpool (B*Hp*Wp, 64) rows fp32 or bf16, x (B, H, W), the raw weight w49, the batch affine
    of the forward and bn1.weight -> (dW (64, 49), dgamma (64,), dbeta (64,)) fp32. The conv output is recomputed from x (nothing
    of it was stored); ReLU mask and window winner are the forward's bit for bit; no atomics (bitwise reproducible)."""
    _chk(x, w49, aff.scale, aff.shift, aff.mean, aff.invstd, gamma)
    dt = _act(dpool)
    B, H, W, Hc, Wc, Hp, Wp = _stem_dims(x, w49)
    if tuple(dpool.shape) != (B * Hp * Wp, 64) or gamma.numel() != 64 or aff.scale.numel() != 64:
        raise ValueError(f"stem7_bwd: dpool {tuple(dpool.shape)} does not match x {tuple(x.shape)}")
    nws = lib.nsid_workspace_bytes(b"stem7_bwd", B * Hp, Wp)
    ws = torch.empty((nws // 4,), device=x.device, dtype=torch.float32)
    out = torch.empty((64 * 49 + 128,), device=x.device, dtype=torch.float32)
    dw, dg, db = out[:64 * 49].view(64, 49), out[64 * 49:64 * 49 + 64], out[64 * 49 + 64:]
    _timed("stem7_bwd_kernel", 2.0 * 64 * 49 * (1.5 * 3 * B * Hc * Wc + B * Hp * Wp),
           4.0 * x.numel() + float(dpool.element_size()) * dpool.numel() + 2.0 * nws,
           lambda: call("nsid_stem7_bwd", _p(dpool), dt, _p(x), B, H, W, _p(w49), _p(aff.scale), _p(aff.shift), _p(aff.mean),
                        _p(aff.invstd), _p(gamma), _p(ws), _p(dw), _p(dg), _p(db), _stream()), (B * Hc * Wc, 64, 49, 1))
    return dw, dg, db


def ibn_relu_bwd(dy, r, B, HW, C, in_gamma, in_beta, bn_aff: "BNAffine", d_in_gamma, d_in_beta, d_bn_gamma, d_bn_beta,
                 eps=IN_EPS, out=None) -> torch.Tensor:
    """backward of ibn_relu_fwd with batch statistics in the BatchNorm half (bn_aff from bn_finalize: scale, shift, mean, invstd):
    returns dr; the four parameter gradients are accumulated"""
    _chk(in_gamma, in_beta, bn_aff.scale, bn_aff.shift, bn_aff.mean, bn_aff.invstd, d_in_gamma, d_in_beta, d_bn_gamma, d_bn_beta)
    dt = _act(dy, r, out)
    half = C // 2
    if (tuple(dy.shape) != (B * HW, C) or tuple(r.shape) != (B * HW, C) or in_gamma.numel() != half or bn_aff.scale.numel() != C - half
            or d_in_gamma.numel() != half or d_in_beta.numel() != half or d_bn_gamma.numel() != C - half or d_bn_beta.numel() != C - half):
        raise ValueError("ibn_relu_bwd: shapes do not match")
    if out is None:
        out = torch.empty_like(dy)
    ws = torch.empty((lib.nsid_workspace_bytes(b"ibn_relu_bwd", B, C) // 4,), device=dy.device, dtype=torch.float32)
    _tk("ibn_relu_bwd_kernel", 7.0 * dy.element_size() * dy.numel(), lambda: call(
        "nsid_ibn_relu_bwd", _p(dy), _p(r), B, HW, C, _p(in_gamma), _p(in_beta), eps, _p(bn_aff.scale), _p(bn_aff.shift),
        _p(bn_aff.mean), _p(bn_aff.invstd), _p(out), _p(ws), _p(d_in_gamma), _p(d_in_beta), _p(d_bn_gamma), _p(d_bn_beta), dt,
        _stream()), (B * HW, C, 0, 1))
    return out


def bn_add_relu_fwd(r3, aff3: "BNAffine", identity, aff_d: Optional["BNAffine"] = None) -> torch.Tensor:
    """relu(BN3(r3) + identity), identity = BN_d(identity) when aff_d is given: the tail of a training-mode residual block"""
    dt = _act(r3, identity)
    M, C = r3.shape
    if tuple(identity.shape) != (M, C):
        raise ValueError("bn_add_relu_fwd: shapes do not match")
    _chk(aff3.scale, aff3.shift, None if aff_d is None else aff_d.scale, None if aff_d is None else aff_d.shift)
    out = torch.empty_like(r3)
    _tk("bn_add_relu_kernel", 3.0 * r3.element_size() * M * C, lambda: call(
        "nsid_bn_add_relu_fwd", _p(r3), _p(aff3.scale), _p(aff3.shift), _p(identity), None if aff_d is None else _p(aff_d.scale),
        None if aff_d is None else _p(aff_d.shift), _p(out), M, C, dt, _stream()), (M, C, 0, 1))
    return out


def relu_bwd(dy, y) -> torch.Tensor:
    """dy where the stored ReLU output y is positive, else 0"""
    dt = _act(dy, y)
    if dy.shape != y.shape:
        raise ValueError("relu_bwd: shapes do not match")
    g = torch.empty_like(dy)
    _tk("relu_bwd_kernel", 3.0 * dy.element_size() * dy.numel(), lambda: call(
        "nsid_relu_bwd", _p(dy), _p(y), _p(g), dy.numel(), dt, _stream()), tuple(dy.shape) + (0, 1))
    return g
