"""GPU: csrc/stems.hip through ops.resample_sinc / ops.stem_pairs and modules/data.py (GPUResample, StemBank, GPUStemPairSampler)
against tests/stem_pairs_oracle.py. The sampler's inputs come from the oracle module (tests/test_stem_pairs_cpu.py checks their gate
margin); every oracle result is computed once per module.

Measured on an MI355X (docs/experiments.md "Stem pairs"; the tests print every figure): the resampler's worst error is 0.17-0.27 of its
per-sample bound at the four downsampling ratios and 0.36 at 8000 -> 16000, 0 at 16000 -> 16000; the sampler's status, x_i and x_j
equal the oracle's bit for bit and its snr is within 0.47 x 2^-23 (relative)."""
import numpy as np
import pytest
import torch

import stem_pairs_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATIOS = [(44100, 16000), (44100, 22050), (22050, 16000), (48000, 22050), (8000, 16000), (16000, 16000)]
LENGTHS = [1, 440, 441, 442, 4417, 50001]


# ---- resampler ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("orig,new", RATIOS)
def test_resample_against_fp64(orig, new, C):
    """exact length; per output sample |y - y64| <= 1.01 n 2^-24 sum |k_j| |x_j| + 1e-20 max|x| (any summation order)"""
    from neuralsampleid_amd.modules.data import GPUResample
    res = GPUResample(orig, new)
    for T in LENGTHS:
        full = O.tones(T + 3, orig, C, seed=T % 97)
        x, xd = full[..., :T], torch.from_numpy(full).to(DEV)[..., :T]      # a two-channel case has a row stride larger than T
        assert C == 1 or xd.stride(0) == T + 3
        y = res(xd)
        y64, bound = O.resample(x, orig, new)
        assert y.dtype == torch.float32 and y.shape == (O.out_len(T, orig, new),) == y64.shape
        err = np.abs(y.cpu().numpy().astype(np.float64) - y64)
        print(orig, new, C, T, "max err / bound", float((err / np.maximum(bound, 1e-300)).max()) if orig != new else float(err.max()))
        assert (err <= bound).all()
        if orig == new and C == 1:
            assert y.data_ptr() == xd.data_ptr()      # the input itself


def test_resample_refusals():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.modules.data import GPUResample
    with pytest.raises(RuntimeError):
        ops.resample_sinc(torch.zeros(100), 44100, 16000)                              # host tensor
    with pytest.raises(RuntimeError):
        GPUResample(44100, 16000)(torch.zeros(100))
    with pytest.raises(RuntimeError):
        ops.resample_sinc(torch.zeros((9, 100), device=DEV), 44100, 16000)             # C = 9
    with pytest.raises(RuntimeError):
        ops.resample_sinc(torch.zeros((2, 100), device=DEV, dtype=torch.float64), 44100, 16000)
    with pytest.raises(RuntimeError, match="LDS"):
        ops.resample_sinc(torch.zeros(100, device=DEV), 44100, 44101)                  # 44101 phases
    with pytest.raises(RuntimeError, match="LDS"):
        GPUResample(44100, 44101)


def test_resample_c_abi_refusals():
    from neuralsampleid_amd import _lib, ops
    x = torch.zeros((2, 128), device=DEV)
    rows, first, ntap, ts, width, o, n = ops._resample_tables(44100, 16000, x.device)
    T_out = O.out_len(128, 44100, 16000)
    y = torch.empty(T_out, device=DEV)
    P, s = ops._p, ops._stream()
    good = (P(x), 128, 2, 128, o, n, width, P(rows), P(first), ntap, ts, P(y), T_out, s)
    assert _lib.lib.nsid_resample_sinc(*good) == 0
    bad = [dict(i=2, v=9), dict(i=2, v=0), dict(i=3, v=0), dict(i=3, v=1 << 31), dict(i=1, v=127), dict(i=12, v=T_out + 1),
           dict(i=5, v=2000), dict(i=9, v=ts + 1), dict(i=0, v=None), dict(i=11, v=None)]
    for b in bad:
        args = list(good)
        args[b["i"]] = b["v"]
        assert _lib.lib.nsid_resample_sinc(*args) == -1, b
    torch.cuda.synchronize()


# ---- sampler --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    """banks on the device, samplers, and the oracle's result of every case"""
    from neuralsampleid_amd.modules.data import GPUStemPairSampler, StemBank, StemPairParams
    tracks = {k: f() for k, f in O.BANKS.items()}
    banks = {}
    for name, ts in tracks.items():
        for cfg_name, cfg in (("A", O.CFG_A), ("B", O.CFG_B)):
            bank = StemBank(cfg, DEV, capacity=40000)          # grows more than once while it is filled
            for t in ts:
                bank.add_resampled(torch.from_numpy(t).to(DEV))
            banks[(name, cfg_name)] = bank
    w = {"tracks": tracks, "banks": banks, "cases": {}}
    for name, (cfg, bank, params) in O.gpu_cases().items():
        cfg_name = "A" if cfg is O.CFG_A else "B"
        L, Ocf, _ = O.frames(cfg)
        sampler = GPUStemPairSampler(cfg, banks[(bank, cfg_name)])
        dev = StemPairParams(*(torch.from_numpy(params[k]).to(DEV) for k in StemPairParams._fields))
        w["cases"][name] = (sampler, dev, params, O.pairs(tracks[bank], params, L, Ocf, cfg["silence"]))
    return w


def _check(got, want):
    x_i, x_j, status, snr = got
    w_i, w_j, w_st, w_snr32, w_snr64 = want
    assert status.dtype == torch.int32 and snr.dtype == torch.float32
    assert np.array_equal(status.cpu().numpy(), w_st)
    assert torch.equal(x_i.cpu(), torch.from_numpy(w_i)) and torch.equal(x_j.cpu(), torch.from_numpy(w_j))
    s = snr.cpu().numpy().astype(np.float64)
    inf = np.isneginf(w_snr64)
    assert np.array_equal(np.isneginf(s), inf)
    err = np.abs(s[~inf] - w_snr64[~inf]) / np.maximum(1.0, np.abs(w_snr64[~inf]))
    print("snr: max relative error", float(err.max(initial=0.0)), "in units of 2^-23:", float(err.max(initial=0.0)) * 2 ** 23)
    assert (err <= 2.0 ** -23).all()
    rej = w_st != 0
    assert not x_i.cpu().numpy()[rej].any() and not x_j.cpu().numpy()[rej].any()


@pytest.mark.parametrize("case", ["draw1", "draw5", "draw64", "explicit", "o1", "rejecting"])
def test_forward_equals_oracle(world, case):
    sampler, dev, _, want = world["cases"][case]
    got = sampler(dev)
    assert got[0].shape == got[1].shape == (len(want[2]), sampler.L)
    _check(got, want)
    again = sampler(dev)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, again))      # bitwise, run to run


def test_cases_hold_every_kind_of_clip(world):
    st = np.concatenate([world["cases"][c][3][2] for c in ("draw64", "explicit")])
    assert {0, 1, 2} <= set(st.tolist())
    snr = world["cases"]["explicit"][3][4]
    valid = (snr >= -10).sum(1)
    assert {0, 2, 3} <= set(valid.tolist())


def test_batch_independence(world):
    """a clip's row does not depend on its neighbours or on the batch size"""
    from neuralsampleid_amd.modules.data import StemPairParams
    sampler, dev, _, _ = world["cases"]["draw64"]
    full = sampler(dev)
    for rows in ([7], [63, 0, 31], list(range(40, 45))):
        idx = torch.tensor(rows, device=DEV)
        sub = sampler(StemPairParams(*(t[idx].contiguous() for t in dev)))
        for a, b in zip(full, sub):
            assert torch.equal(a[idx].view(torch.int32), b.view(torch.int32))


def test_batch_packs_the_accepted_rows(world):
    sampler, dev, _, want = world["cases"]["draw64"]
    for B in (8, 64):                                 # more accepted than B; fewer than B
        x_i, x_j, n_ok = sampler.batch(B, params=dev)
        w_i, w_j, w_n = O.pack(want[0], want[1], want[2], B)
        assert x_i.shape == x_j.shape == (B, sampler.L) and n_ok.dtype == torch.int32 and n_ok.dim() == 0 and n_ok.is_cuda
        assert int(n_ok) == w_n and (w_n == B if B == 8 else 0 < w_n < B)
        assert torch.equal(x_i.cpu(), torch.from_numpy(w_i)) and torch.equal(x_j.cpu(), torch.from_numpy(w_j))
    sampler, dev, _, want = world["cases"]["rejecting"]       # oversample 1.0 on a bank of mostly rejected tracks
    x_i, x_j, n_ok = sampler.batch(16, params=dev)
    w_i, w_j, w_n = O.pack(want[0], want[1], want[2], 16)
    assert int(n_ok) == w_n < 16 and not x_i[w_n:].any() and not x_j[w_n:].any()
    assert torch.equal(x_i.cpu(), torch.from_numpy(w_i)) and torch.equal(x_j.cpu(), torch.from_numpy(w_j))


def test_batch_draws_its_own_candidates(world):
    sampler = world["cases"]["draw64"][0]
    g = torch.Generator().manual_seed(11)
    x_i, x_j, n_ok = sampler.batch(8, generator=g, oversample=1.25)
    params = sampler.draw(10, torch.Generator().manual_seed(11))
    assert all(np.array_equal(getattr(params, k).cpu().numpy(), v) for k, v in world["cases"]["draw10"][2].items())
    f_i, f_j, st, _ = sampler(params)
    ok = torch.nonzero(st == 0).flatten()[:8]
    assert int(n_ok) == len(ok) and torch.equal(x_i[:len(ok)], f_i[ok]) and torch.equal(x_j[:len(ok)], f_j[ok])
    assert not x_i[len(ok):].any()


def test_forward_and_batch_under_graph_capture(world):
    """captured on one stream; a replay reads the params' current contents"""
    from neuralsampleid_amd.modules.data import StemPairParams
    sampler, dev_a, _, _ = world["cases"]["draw5"]
    _, dev_b, _, want_b = world["cases"]["draw5b"]
    live = StemPairParams(*(t.clone() for t in dev_a))
    sampler(live)                                     # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = sampler(live)
            packed = sampler.batch(4, params=live)
    torch.cuda.current_stream().wait_stream(s)
    for dst, src in zip(live, dev_b):
        dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    _check(out, want_b)
    w_i, w_j, w_n = O.pack(want_b[0], want_b[1], want_b[2], 4)
    assert int(packed[2]) == w_n and torch.equal(packed[0].cpu(), torch.from_numpy(w_i)) and torch.equal(packed[1].cpu(), torch.from_numpy(w_j))
    eager = sampler(dev_b)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, eager))


def test_out_of_range_params_are_clamped(world):
    """no index leaves a track: wild params give the clamped clip's result"""
    from neuralsampleid_amd.modules.data import StemPairParams
    sampler, _, _, want = world["cases"]["clamped"]
    wild, _ = O.wild_params()
    _check(sampler(StemPairParams(*(torch.from_numpy(wild[k]).to(DEV) for k in StemPairParams._fields))), want)


def test_sampler_refusals(world):
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.modules.data import StemPairParams
    sampler, dev, _, _ = world["cases"]["draw5"]
    with pytest.raises(RuntimeError):
        sampler(StemPairParams(*(t.cpu() for t in dev)))                               # host params
    with pytest.raises(RuntimeError):
        sampler(dev._replace(key=dev.key[:, :2].contiguous()))
    with pytest.raises(RuntimeError):
        sampler(dev._replace(start=dev.start.long()))
    b = sampler.bank
    with pytest.raises(RuntimeError):
        ops.stem_pairs(b.buf.cpu(), b.base, b.length, *dev, sampler.L, sampler.O, 1e-5)
    with pytest.raises(RuntimeError):
        ops.stem_pairs(b.buf, b.base, b.length, *dev, sampler.L, 0, 1e-5)               # O < 1


def test_track_table_outside_the_bank_is_rejected_unread(world):
    """status 3: a table entry that does not lie inside the bank (not reachable through StemBank) is not read; its rows are zero"""
    from neuralsampleid_amd import ops
    sampler, dev, params, want = world["cases"]["explicit"]
    b = sampler.bank
    args = (*dev, sampler.L, sampler.O, 1e-5)
    for base, length in ((b.base + b.buf.numel(), b.length), (-b.base - 1, b.length), (b.base, torch.full_like(b.length, 2 ** 30))):
        x_i, x_j, status, snr = ops.stem_pairs(b.buf, base.contiguous(), length, *args)
        assert (status == 3).all() and not x_i.any() and not x_j.any() and torch.isnan(snr).all()
    base = b.base.clone()
    base[2] = b.buf.numel() - 3 * b.lengths[2] + 1    # one float past the end
    x_i, x_j, status, snr = ops.stem_pairs(b.buf, base, b.length, *args)
    bad = params["track"] == 2
    st = status.cpu().numpy()
    assert bad.any() and (st[bad] == 3).all() and np.array_equal(st[~bad], want[2][~bad])
    assert not x_i.cpu().numpy()[bad].any() and np.array_equal(x_i.cpu().numpy()[~bad], want[0][~bad])
    assert np.array_equal(x_j.cpu().numpy()[~bad], want[1][~bad])
    x_p, _, n_ok, _, _ = ops.stem_pairs(b.buf, base, b.length, *args, pack=len(st))
    assert int(n_ok) == int((st == 0).sum()) and not x_p[int(n_ok):].any()


def test_sampler_c_abi_refusals(world):
    """NSID_EINVAL before any launch"""
    from neuralsampleid_amd import _lib, ops
    sampler, dev, _, _ = world["cases"]["draw5"]
    b, P, s = sampler.bank, ops._p, ops._stream()
    N, L, Ocf = 5, sampler.L, sampler.O
    status, plan = torch.empty(N, device=DEV, dtype=torch.int32), torch.empty(N, device=DEV, dtype=torch.int32)
    snr, n_ok = torch.empty((N, 3), device=DEV), torch.empty((), device=DEV, dtype=torch.int32)
    x_i, x_j = torch.empty((N, L), device=DEV), torch.empty((N, L), device=DEV)
    gate = [P(b.buf), b.buf.numel(), P(b.base), P(b.length), len(b), P(dev.track), P(dev.start), P(dev.key), P(dev.off_i), P(dev.off_j),
            N, L, Ocf, 1e-5, P(status), P(snr), P(plan), s]
    build = [P(b.buf), b.buf.numel(), P(b.base), P(b.length), len(b), P(dev.track), P(dev.start), P(dev.off_i), P(dev.off_j), P(status),
             P(plan), N, L, Ocf, 0, 0, P(x_i), L, P(x_j), L, None, s]
    assert _lib.lib.nsid_stem_pairs_gate(*gate) == 0 and _lib.lib.nsid_stem_pairs_build(*build) == 0
    for i, v in ((0, None), (1, 0), (2, None), (2, P(b.base) + 4), (4, 0), (5, None), (10, 0), (10, 65536), (11, 0), (12, 0),
                 (11, 1 << 30), (14, None), (16, None)):
        args = list(gate)
        args[i] = v
        assert _lib.lib.nsid_stem_pairs_gate(*args) == -1, (i, v)
    for i, v in ((0, None), (4, 0), (9, None), (10, None), (11, 0), (12, 0), (13, 0), (14, 2), (14, 1), (16, None), (17, L - 1),
                 (19, L - 1)):
        args = list(build)
        args[i] = v
        assert _lib.lib.nsid_stem_pairs_build(*args) == -1, (i, v)
    packed = list(build)
    packed[14], packed[15], packed[20] = 1, 65536, P(n_ok)
    assert _lib.lib.nsid_stem_pairs_build(*packed) == -1
    torch.cuda.synchronize()


# ---- bank -----------------------------------------------------------------------------------------------------------------------------
def test_bank_add_equals_the_composition(world):
    """add() on a stereo 44100 Hz dict = add_resampled of resample, bass + other, cut to the common length: bit for bit"""
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.modules.data import StemBank
    cfg = O.CFG_A
    T = 17000                                         # 6 168 samples at 16 kHz >= W
    stems = {n: torch.from_numpy(O.tones(T - 10 * i, 44100, 2, seed=40 + i)) for i, n in enumerate(("bass", "other", "vocals", "drums"))}
    stems["mix"] = torch.zeros(3)                     # ignored
    a, b = StemBank(cfg, DEV, capacity=16), StemBank(cfg, DEV)
    assert a.add(stems, 44100) == 0
    r = {n: ops.resample_sinc(stems[n].to(DEV), 44100, 16000) for n in ("bass", "other", "vocals", "drums")}
    n_bo = min(r["bass"].numel(), r["other"].numel())
    Tm = min(n_bo, r["vocals"].numel(), r["drums"].numel())
    b.add_resampled(torch.stack(((r["bass"][:n_bo] + r["other"][:n_bo])[:Tm], r["vocals"][:Tm], r["drums"][:Tm])))
    assert a.lengths == b.lengths == [O.out_len(T - 30, 44100, 16000)] and torch.equal(a.track(0), b.track(0))
    y64, bound = O.resample(stems["vocals"].numpy(), 44100, 16000)
    assert (np.abs(a.track(0)[1].cpu().numpy() - y64[:Tm]) <= bound[:Tm]).all()
    assert a.length.dtype == torch.int32 and a.base.dtype == torch.int64 and a.base.tolist() == [0] and a.nbytes() == 12 * Tm


def test_bank_growth_keeps_earlier_tracks(world):
    bank, tracks = world["banks"][("main", "A")], world["tracks"]["main"]
    assert bank.buf.numel() >= bank.used > 40000 and len(bank) == 6
    off = 0
    for t, rows in enumerate(tracks):
        assert torch.equal(bank.track(t).cpu(), torch.from_numpy(rows))
        assert bank.base[t].item() == off and bank.length[t].item() == rows.shape[1]
        off += 3 * rows.shape[1]


def test_bank_refuses_a_short_track():
    from neuralsampleid_amd.modules.data import StemBank
    bank = StemBank(O.CFG_A, DEV)
    W = O.frames(O.CFG_A)[2]
    with pytest.raises(ValueError, match="shorter"):
        bank.add_resampled(torch.zeros((3, W - 1), device=DEV))
    with pytest.raises(ValueError, match="shorter"):
        bank.add({n: torch.zeros(1000) for n in ("bass", "other", "vocals", "drums")}, 44100)
    with pytest.raises(RuntimeError):
        StemBank(O.CFG_A, "cpu")
    assert len(bank) == 0
    bank.add_resampled(torch.zeros((3, W), device=DEV))
    assert len(bank) == 1
