"""Test helper (like augment_oracle.py): the baseline's waveform effects of DESIGN.md "Baseline waveform augmentations" -- the
reference's fx_util Compressor, BandEQ and FrameLevelCorruption and the chain x_i_out = T2(T1(x_j) + x_i) -- restated in plain numpy /
Python on the CPU. Written from that description; no scipy, no audiomentations. The vocoder options come from augment_oracle.py.

    compress(x, threshold, ratio, attack, release)    fp64 level follower, one rounded operation at a time -> float32
    cascade(x, table, dt)                             table (n, 6) = b0, b1, b2, a1, a2, post per section, transposed direct form II in
                                                      dt (np.float64 or np.longdouble), unfused, sosfilt's order -> dt
    band_eq(x, bands, dt)                             bands = [(sections (order, 5), gain_db)], the EQ as the reference applies it -> dt
    frames(x, frame_size, ops)                        frame duplicate / remove / silence -> edited clip (any length)
    augment(x_i, x_j, clip, L_frames)                 the whole chain for one clip -> float64 (float32 values where the chain is exact)"""
import numpy as np

import augment_oracle as A

T1_EQ, T1_COMPRESS, T1_GAIN = 0, 1, 2
OP_DUPLICATE, OP_REMOVE, OP_SILENCE = 1, 2, 4


def clamp_cmp(c):
    """the kernel's parameter ranges: threshold >= 0, ratio >= 1, attack and release in [0, 1]; NaN -> the lower end"""
    def lo(v, a):
        return a if not v >= a else v
    thr, ratio, att, rel = (float(v) for v in c)
    return lo(thr, 0.0), lo(ratio, 1.0), min(lo(att, 0.0), 1.0), min(lo(rel, 0.0), 1.0)


def compress(x, threshold, ratio, attack, release):
    """fx_util.Compressor.apply: Python floats are IEEE doubles, every operation below rounds once"""
    x = np.asarray(x, np.float32)
    y = np.empty_like(x)
    g = 1.0
    oma, omr = 1.0 - attack, 1.0 - release
    for n, v in enumerate(x.astype(np.float64).tolist()):
        a = abs(v)
        if a > threshold:
            t = threshold + (a - threshold) / ratio
            g = attack * g + oma * t if g > t else release * g + omr * t
        y[n] = v * g                                 # one rounding to fp64, one to fp32
    return y


def cascade(x, table, dt=np.float64):
    """y = b0 u + z1; z1 = (b1 u - a1 y) + z2; z2 = b2 u - a2 y; the section hands on y * post"""
    y = np.asarray(x).astype(dt)
    plain = dt == np.float64
    for row in np.asarray(table):
        b0, b1, b2, a1, a2, post = (float(v) for v in row) if plain else (dt(v) for v in row)
        z1 = z2 = 0.0 if plain else dt(0)
        src = y.tolist() if plain else list(y)
        dst = []
        for u in src:
            v = b0 * u + z1
            z1 = (b1 * u - a1 * v) + z2
            z2 = b2 * u - a2 * v
            dst.append(v * post)
        y = np.array(dst, dt)
    return y


def band_table(bands):
    """[(sections (order, 5), gain_db)] -> (n, 6): the band's gain 10^(g/20) on its last section, 1 elsewhere"""
    rows = []
    for sec, gain_db in bands:
        sec = np.asarray(sec, np.float64)
        post = np.ones(len(sec))
        post[-1] = 10.0 ** (gain_db / 20.0)
        rows.append(np.concatenate([sec, post[:, None]], 1))
    return np.concatenate(rows, 0) if rows else np.zeros((0, 6))


def band_eq(x, bands, dt=np.float64):
    return cascade(x, band_table(bands), dt)


def frames(x, frame_size, ops):
    """fx_util.FrameLevelCorruption.apply with the three draws of frame f given as ops[f] bits: doubled, then dropped, then zeroed"""
    x = np.asarray(x)
    out, i, f = [], 0, 0
    while i < len(x):
        fr = x[i:i + frame_size]
        if ops[f] & OP_DUPLICATE:
            fr = np.concatenate((fr, fr))
        if ops[f] & OP_REMOVE:
            fr = fr[:0]
        if ops[f] & OP_SILENCE:
            fr = np.zeros_like(fr)
        out.append(fr)
        i += frame_size
        f += 1
    return np.concatenate(out)


def clamp_frame_size(frame_size, L, F):
    return min(max(int(frame_size), -(-L // F)), L)


def to_length(y, L):
    return y[:L] if len(y) >= L else np.pad(y, (0, L - len(y)))


def t1(x_j, clip, dt=np.float64):
    """T1 of the sample stems, float32 (the gain option is applied in the mix)"""
    x_j = np.asarray(x_j, np.float32)
    if clip["mode1"] == T1_EQ:
        n = min(max(int(clip["n_sec"]), 0), len(clip["sos"]))
        return cascade(x_j, clip["sos"][:n], dt).astype(np.float32)
    if clip["mode1"] == T1_COMPRESS:
        return compress(x_j, *clamp_cmp(clip["cmp"]))
    return x_j


def mix32(x_i, s, gain):
    """float32: the product rounded, then the sum rounded (one fp32 add at gain 1)"""
    return (np.float32(gain) * np.asarray(s, np.float32)).astype(np.float32) + np.asarray(x_i, np.float32)


def augment(x_i, x_j, clip, dt=np.float64):
    """clip: dict of mode1, gain, cmp (4,), sos (S, 6), n_sec, mode2, rate, frame_size, frame_ops (F,) -> (L,) float64"""
    L = len(x_i)
    s = t1(x_j, clip, dt)
    if 2 <= clip["mode2"] <= 4:
        fsz = clamp_frame_size(clip["frame_size"], L, len(clip["frame_ops"]))
        return to_length(frames(mix32(x_i, s, clip["gain"]), fsz, clip["frame_ops"]), L).astype(np.float64)
    return A.augment(np.asarray(x_i, np.float32), s, np.float32(clip["gain"]), 1 if clip["mode2"] == 1 else 0, clip["rate"])


def rel(a, b):
    return A.rel(a, b)
