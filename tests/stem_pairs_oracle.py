"""CPU oracle of the stem-pair path (csrc/stems.hip, modules/data.py): numpy restatements of DESIGN.md "Stem pairs" -- the sinc
resampler in fp64 on the fp32-rounded table with its dot-product error bound, and the sampler (SNR gate with fp64 sums, key-ordered
split, crops, silence) -- plus the reference's fp32 pipeline (data.py:92-150) restated in torch and the inputs of the GPU tests, which
the CPU tests check for their gate margin."""
import math

import numpy as np
import torch

WIDTH, ROLLOFF = 6, 0.99


# ---- resampler ------------------------------------------------------------------------------------------------------------------------
def ratio(orig, new):
    g = math.gcd(orig, new)
    orig, new = orig // g, new // g
    base = min(orig, new) * ROLLOFF
    return orig, new, int(math.ceil(WIDTH * orig / base)), base


def table64(orig, new):
    """(k (new, 2 width + orig) fp64, live (same shape) bool): the filter before its one rounding to fp32, and where the clamp did not fire"""
    orig, new, width, base = ratio(orig, new)
    p = np.arange(new, dtype=np.float64)[:, None]
    j = np.arange(2 * width + orig, dtype=np.float64)[None, :]
    t = (-p / new + (j - width) / orig) * base
    live = np.abs(t) < WIDTH
    t = np.clip(t, -WIDTH, WIDTH)
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(np.pi * t) / (np.pi * t))
    return sinc * np.cos(np.pi * t / 12) ** 2 * base / orig, live


def out_len(T, orig, new):
    return -((-new * T) // orig)                      # ceil(new T / orig); the gcd cancels


def mono32(x):
    """fp32 sum of the channels in channel order, divided by C"""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 1:
        return x
    m = x[0].copy()
    for c in range(1, x.shape[0]):
        m = m + x[c]
    return (m / np.float32(x.shape[0])).astype(np.float32)


def _frames(m64, orig, new, width, T_out):
    Q = -(-T_out // new)
    need = (Q - 1) * orig + 2 * width + orig          # never past the `width + orig` zeros behind the signal
    xpad = np.zeros(max(need, width + m64.size), dtype=np.float64)
    xpad[width:width + m64.size] = m64
    idx = np.arange(Q)[:, None] * orig + np.arange(2 * width + orig)[None, :]
    return xpad[idx]                                  # (Q, taps)


def resample(x, orig, new, k32=None):
    """(y64, bound): y in fp64 from the fp32 table and the fp32 mono signal, and the issue's per-sample bound
    1.01 n 2^-24 sum_j |k_j| |x_j| + 1e-20 max|x| with n the phase's live tap count"""
    m = mono32(x)
    T = m.size
    T_out = out_len(T, orig, new)
    if orig == new:
        return m.astype(np.float64), np.zeros(T)
    o, n, width, _ = ratio(orig, new)
    k64, live = table64(orig, new)
    k = (k64.astype(np.float32) if k32 is None else k32).astype(np.float64)
    fr = _frames(m.astype(np.float64), o, n, width, T_out)
    y = (fr @ k.T).reshape(-1)[:T_out]                # [q][p] -> q new + p
    s = (np.abs(fr) @ np.abs(k).T).reshape(-1)[:T_out]
    ntap = np.tile(live.sum(1), fr.shape[0])[:T_out]
    bound = 1.01 * ntap * 2.0 ** -24 * s + 1e-20 * float(np.abs(m).max())
    return y, bound


def resample_compact_walk(x, orig, new, rows, first, live_n):
    """the kernel's walk, only the live taps of the compact table, as an exactly rounded fp64 sum (math.fsum: no summation order)"""
    m = mono32(x).astype(np.float64)
    T = m.size
    o, n, width, _ = ratio(orig, new)
    T_out = out_len(T, orig, new)
    y = np.zeros(T_out)
    for i in range(T_out):
        q, p = divmod(i, n)
        j0 = q * o + int(first[p]) - width
        y[i] = math.fsum(float(rows[p, a]) * m[j0 + a] for a in range(int(live_n[p])) if 0 <= j0 + a < T)
    return y


def resample_full_walk(x, orig, new, k32):
    """every tap of the full table, as an exactly rounded fp64 sum"""
    m = mono32(x).astype(np.float64)
    o, n, width, _ = ratio(orig, new)
    T_out = out_len(m.size, orig, new)
    fr = _frames(m, o, n, width, T_out)
    k = k32.astype(np.float64)
    return np.array([math.fsum((fr[i // n] * k[i % n]).tolist()) for i in range(T_out)])


def tones(T, sr, C=1, seed=0):
    """tones plus a 0.05 noise floor, (T,) or (C, T) fp32"""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(T, dtype=np.float64) / sr
    out = []
    for c in range(C):
        x = 0.4 * np.sin(2 * np.pi * 440.0 * t + c) + 0.25 * np.sin(2 * np.pi * 3300.0 * t) + 0.1 * np.sin(2 * np.pi * 97.0 * t + 0.3)
        out.append((x + 0.05 * rng.standard_normal(T)).astype(np.float32))
    return out[0] if C == 1 else np.stack(out)


# ---- sampler --------------------------------------------------------------------------------------------------------------------------
def gate(seg):
    """seg (3, W) fp32 -> (snr64 (3,), valid (3,)): fp32 tot / sig / d, exact squares summed in fp64"""
    seg = np.asarray(seg, dtype=np.float32)
    W = seg.shape[1]
    tot = (seg[0] + seg[1]) + seg[2]
    snr, valid = np.zeros(3), np.zeros(3, dtype=bool)
    for c in range(3):
        sig = tot - seg[c]
        d = sig - seg[c]
        p_sig = math.fsum((sig.astype(np.float64) ** 2).tolist())
        p_n = math.fsum((d.astype(np.float64) ** 2).tolist())
        with np.errstate(divide="ignore"):
            snr[c] = -np.inf if p_sig == 0 else 10.0 * np.log10((p_sig / W) / (p_n / W + 1e-8))
        valid[c] = p_sig >= 0.1 * (p_n + 1e-8 * W)
    return snr, valid


def clip(track_rows, start, key, off_i, off_j, L, O, silence):
    """one clip -> (x_i (L,), x_j (L,), status, snr32 (3,), snr64 (3,)); rejected clips are zero"""
    W = L + O
    seg = np.asarray(track_rows, dtype=np.float32)[:, start:start + W]
    assert seg.shape[1] == W and 0 <= off_i < O and 0 <= off_j < O
    snr, valid = gate(seg)
    zero = np.zeros(L, dtype=np.float32)
    snr32 = snr.astype(np.float32)
    order = sorted([c for c in range(3) if valid[c]], key=lambda c: (np.float32(key[c]), c))
    if len(order) < 2:
        return zero, zero, 1, snr32, snr
    x_i = seg[order[-1]]
    x_j = seg[order[0]] if len(order) == 2 else seg[order[0]] + seg[order[1]]
    x_i, x_j = x_i[off_i:off_i + L], x_j[off_j:off_j + L]
    if np.float32(np.abs(x_i).max()) < np.float32(silence) or np.float32(np.abs(x_j).max()) < np.float32(silence):
        return zero, zero, 2, snr32, snr
    return x_i.copy(), x_j.copy(), 0, snr32, snr


def pairs(tracks, params, L, O, silence):
    """params: dict of numpy arrays track, start, key, off_i, off_j -> (x_i (N, L), x_j, status (N,), snr32 (N, 3), snr64 (N, 3))"""
    N = len(params["track"])
    out = [clip(tracks[int(params["track"][b])], int(params["start"][b]), params["key"][b], int(params["off_i"][b]),
                int(params["off_j"][b]), L, O, silence) for b in range(N)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32),
            np.stack([o[3] for o in out]), np.stack([o[4] for o in out]))


def pack(x_i, x_j, status, B):
    """batch(): the accepted rows in order in the first rows of (B, L), zeros behind them"""
    ok = np.flatnonzero(status == 0)[:B]
    o_i, o_j = np.zeros((B, x_i.shape[1]), np.float32), np.zeros((B, x_i.shape[1]), np.float32)
    o_i[:len(ok)], o_j[:len(ok)] = x_i[ok], x_j[ok]
    return o_i, o_j, len(ok)


def fp32_pipeline(seg, key, off_i, off_j, L, silence):
    """What the reference's dataset computes for one stacked (3, W) segment, restated in torch fp32 in its operation order (data.py:
    92-150): the mix is the dim-0 sum, powers are fp32 means, the verdict is `10 log10(P_sig / (P_n + 1e-8)) >= -10`, the pair sides
    are dim-0 sums of the chosen rows. The shuffle is replaced by the order of `key` (ties to the lower index) and the two crop
    offsets are given. -> (snr (3,) floats, valid stems, x_i, x_j), the last two None where the reference draws again."""
    seg = torch.as_tensor(seg)
    mix = seg.sum(dim=0)
    snr = []
    for c in range(3):
        rest = mix - seg[c]
        snr.append(float(10 * torch.log10(torch.mean(rest ** 2) / (torch.mean((rest - seg[c]) ** 2) + 1e-8))))
    valid = [c for c in range(3) if snr[c] >= -10]
    if len(valid) < 2:
        return snr, valid, None, None
    order = sorted(valid, key=lambda c: (np.float32(key[c]), c))
    x_i = seg[order[-1:]].sum(dim=0)[off_i:off_i + L]
    x_j = seg[order[:-1]].sum(dim=0)[off_j:off_j + L]
    if x_i.abs().max() < silence or x_j.abs().max() < silence:
        return snr, valid, None, None
    return snr, valid, x_i.numpy(), x_j.numpy()


# ---- the inputs of tests/test_stem_pairs_gpu.py (tests/test_stem_pairs_cpu.py checks their gate margin) ------------------------------
CFG_A = {"fs": 16000, "dur": 0.2601, "offset": 0.05, "silence": 1e-5}          # L = 4161 (odd), O = 800, W = 4961
CFG_B = {"fs": 16000, "dur": 0.2601, "offset": 0.0001, "silence": 1e-5}        # O = 1: every offset is 0
AMPLITUDES = [(1, 1, 1), (1, 1, 10), (1e-4, 1e-4, 1e-4), (0, 0, 1), (0, 1, 1), (0, 0, 0)]


def frames(cfg):
    L, O = int(cfg["fs"] * cfg["dur"]), int(cfg["fs"] * cfg["offset"])
    return L, O, L + O


def gaussian_stems(amps, T, seed):
    rng = np.random.default_rng(seed)
    return np.stack([(rng.standard_normal(T) * (0.1 * a)).astype(np.float32) for a in amps])


def bank_main():
    """six tracks: lengths W, W + 1, 3 W + 7 and three of about 2 W; three-valid, two-valid, status-1 and status-2 material"""
    W = frames(CFG_A)[2]
    spec = [((1, 1, 1), W), ((1, 1, 10), W + 1), ((1, 1, 1), 3 * W + 7), ((1e-4, 1e-4, 1e-4), 2 * W + 3), ((0, 0, 1), 2 * W + 11),
            ((0, 1, 1), 2 * W - 1)]
    return [gaussian_stems(a, T, 10 + i) for i, (a, T) in enumerate(spec)]


def bank_rejecting():
    """mostly rejected: all-zero, quiet, one-stem tracks and a single good one"""
    W = frames(CFG_A)[2]
    spec = [((0, 0, 0), W + 5), ((1e-4, 1e-4, 1e-4), W + 9), ((0, 0, 1), 2 * W), ((1, 1, 1), W + 2), ((0, 0, 0), W), ((0, 0, 1), W + 1)]
    return [gaussian_stems(a, T, 30 + i) for i, (a, T) in enumerate(spec)]


def draw(lengths, W, O, N, seed):
    from neuralsampleid_amd.modules.data import draw_stem_pairs
    g = torch.Generator().manual_seed(seed)
    return {k: v.numpy() for k, v in draw_stem_pairs(lengths, W, O, N, g)._asdict().items()}


def explicit_params():
    """main bank, CFG_A: the last legal start, off = O - 1, equal keys, every key order of a three-valid clip, each track at both ends"""
    L, O, W = frames(CFG_A)
    lengths = [t.shape[1] for t in bank_main()]
    rows = []
    for perm in ((0.1, 0.5, 0.9), (0.1, 0.9, 0.5), (0.5, 0.1, 0.9), (0.5, 0.9, 0.1), (0.9, 0.1, 0.5), (0.9, 0.5, 0.1)):
        rows.append((2, lengths[2] - W, perm, O - 1, O - 1))
    rows.append((2, lengths[2] - W, (0.5, 0.5, 0.5), O - 1, 0))
    rows.append((2, 17, (0.7, 0.2, 0.2), 0, O - 1))
    rows.append((2, 1, (0.2, 0.7, 0.7), 3, 5))
    for t in range(6):
        for keys in ((0.3, 0.6, 0.9), (0.9, 0.6, 0.3), (0.6, 0.9, 0.3)):
            rows.append((t, 0, keys, 0, O - 1))
            rows.append((t, lengths[t] - W, keys, O - 1, 1))
    return {"track": np.array([r[0] for r in rows], np.int32), "start": np.array([r[1] for r in rows], np.int32),
            "key": np.array([r[2] for r in rows], np.float32), "off_i": np.array([r[3] for r in rows], np.int32),
            "off_j": np.array([r[4] for r in rows], np.int32)}


def wild_params():
    """(params outside their ranges, the same clamped as the kernels clamp them): main bank, CFG_A"""
    _, O, W = frames(CFG_A)
    lengths = [t.shape[1] for t in bank_main()]
    key = np.array([(0.1, 0.5, 0.9), (0.9, 0.1, 0.5), (0.5, 0.5, 0.1), (0.2, 0.8, 0.4), (0.6, 0.3, 0.7)], np.float32)
    wild = {"track": np.array([-3, 99, 2, 2, 1], np.int32), "start": np.array([5, -7, 2 ** 30, -1, 1 << 20], np.int32), "key": key,
            "off_i": np.array([-1, O, 5, 2 ** 30, 0], np.int32), "off_j": np.array([O + 5, -9, 0, 1, 2], np.int32)}
    tr = np.clip(wild["track"], 0, len(lengths) - 1)
    clamped = {"track": tr, "start": np.clip(wild["start"], 0, np.array([lengths[t] for t in tr]) - W).astype(np.int32), "key": key,
               "off_i": np.clip(wild["off_i"], 0, O - 1), "off_j": np.clip(wild["off_j"], 0, O - 1)}
    return wild, clamped


def gpu_cases():
    """name -> (cfg, bank name, params): every sampler input of the GPU tests"""
    la = [t.shape[1] for t in bank_main()]
    lr = [t.shape[1] for t in bank_rejecting()]
    _, Oa, Wa = frames(CFG_A)
    _, Ob, Wb = frames(CFG_B)
    return {
        "draw1": (CFG_A, "main", draw(la, Wa, Oa, 1, 1)),
        "draw5": (CFG_A, "main", draw(la, Wa, Oa, 5, 2)),
        "draw64": (CFG_A, "main", draw(la, Wa, Oa, 64, 3)),
        "draw5b": (CFG_A, "main", draw(la, Wa, Oa, 5, 6)),
        "draw10": (CFG_A, "main", draw(la, Wa, Oa, 10, 11)),
        "clamped": (CFG_A, "main", wild_params()[1]),
        "explicit": (CFG_A, "main", explicit_params()),
        "o1": (CFG_B, "main", draw(la, Wb, Ob, 5, 4)),
        "rejecting": (CFG_A, "rejecting", draw(lr, Wa, Oa, 16, 5)),
    }


BANKS = {"main": bank_main, "rejecting": bank_rejecting}
