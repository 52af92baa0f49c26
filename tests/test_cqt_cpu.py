"""CPU: the constant-Q front end of the ResNet-IBN baseline (csrc/cqt.hip, nsid_cqt) without a GPU — the definition itself
(tests/cqt_oracle.py against the structural facts and the analytic responses of nnAudio's CQT1992v2), the host-side tables of
frontend.CQTFrontEnd against that oracle, the binding, and the module shell modules/transformations.GPUTransformCQT."""
import inspect
import math

import numpy as np
import pytest
import torch

from cqt_oracle import CQTOracle, tone

CFG = {"fs": 22050, "hop_len": 512, "n_frames": 216, "overlap": 0.5, "arch": "resnet-ibn"}


@pytest.fixture(scope="module")
def oracle():
    return CQTOracle(22050, 512)


def unpack(front):
    """the packed table of CQTFrontEnd read back through its group descriptors (include/nsid.h nsid_cqt): dense (84, width)
    complex64 taps, and how many times every bin was covered"""
    hopP = (front.hop + 255) // 256 * 256
    table = front.taps.cpu().numpy()
    dense = np.zeros((front.n_bins, front.width), dtype=np.complex64)
    covered = np.zeros(front.n_bins, dtype=np.int64)
    used = 0
    for bin0, nbins, tap0, extent, off in front.groups:
        assert off == used and off % 4 == 0 and 1 <= nbins <= 8 and tap0 >= 0 and tap0 + extent <= front.width
        Q = (extent - 1) // front.hop + 1
        rows = table[off:off + Q * hopP * 16].reshape(-1, 16, 4).transpose(0, 2, 1).reshape(Q * hopP, 16)   # [row/4][column][row%4]
        used += Q * hopP * 16
        r = np.arange(Q * hopP) % hopP
        n = tap0 + np.arange(Q * hopP) // hopP * front.hop + r
        assert not rows[r >= front.hop].any()                                 # padding rows of the hop
        assert not rows[(r < front.hop) & (n >= tap0 + extent)].any()         # nothing outside the extent
        assert not rows[:, 2 * nbins:].any()                                  # unused columns
        keep = (r < front.hop) & (n < front.width)
        for j in range(nbins):
            dense[bin0 + j, n[keep]] = rows[keep, 2 * j] + 1j * rows[keep, 2 * j + 1]
            covered[bin0 + j] += 1
    assert used == table.size
    return dense, covered


def test_structural_numbers(oracle):
    assert oracle.width == 16384
    assert oracle.lengths[0] == 11341 and oracle.lengths[12] == 5671 and oracle.lengths[83] == 94      # l_0 from 11340.007
    assert int(oracle.lengths.sum()) == 200505
    assert abs(oracle.freqs[83] - 3950.68) < 5e-3
    assert [int(oracle.starts[k]) for k in (0, 1, 2, 83)] == [2521, 2840, 3140, 8145]
    assert oracle.taps.dtype == np.complex64 and oracle.taps.shape == (84, 16384)
    nz = oracle.taps != 0
    for k in (0, 1, 12, 83):                                                   # odd and even lengths
        s, l = int(oracle.starts[k]), int(oracle.lengths[k])
        assert not nz[k, :s].any() and not nz[k, s + l:].any() and nz[k, s + 1:s + l].all()
    assert oracle.n_frames_of(110250) == 216
    for L in (8193, 9001, 9254, 110250):
        assert oracle(torch.zeros(L)).shape == (1, 84, 1 + L // 512)
    assert CQTOracle(22050, 500)(torch.zeros(9001)).shape == (1, 84, 19)


def test_tone_response(oracle):
    """A cos(2 pi f_k n / fs) reads (A / 2) sqrt(l_k) at bin k of an interior frame (measured error 5-8e-6 relative)"""
    L, A = 32768, 0.7
    for k in (0, 30, 83):
        out = oracle(tone(22050, float(oracle.freqs[k]), L, A), torch.float64)[0]
        want = 0.5 * A * math.sqrt(float(oracle.lengths[k]))
        t = (L // 2) // 512                                                    # frame centred mid-signal: no reflection in its window
        assert abs(float(out[k, t]) - want) <= 1e-4 * want, (k, float(out[k, t]), want)


def test_unit_impulse_reads_the_taps(oracle):
    """out[k, t] == |taps_k[p - t hop + width/2]| sqrt(l_k) for a unit impulse at p. The reflection mirrors sample p to -p and to
    2 (L - 1) - p: the edge samples p = 0 and p = L - 1 are their own images (not duplicated), and at L = 20000 the interior
    p = 9216 (a multiple of the hop, so that a frame centres on it and the 94-tap bin sees it) has both images outside the padding of width/2 = 8192, so the plain formula holds at all three."""
    L, W = 20000, 16384
    sq = torch.sqrt(torch.from_numpy(oracle.lengths.astype(np.float32))).double().numpy()
    for p in (0, 9216, L - 1):
        x = torch.zeros(L)
        x[p] = 1.0
        out = oracle(x, torch.float64)[0].numpy()
        assert out.shape == (84, 40) and (out > 0).any(1).all()
        for t in range(out.shape[1]):
            n = p - t * 512 + W // 2
            want = np.abs(oracle.taps[:, n].astype(np.complex128)) * sq if 0 <= n < W else np.zeros(84)
            assert np.abs(out[:, t] - want).max() <= 1e-12, (p, t)


def test_front_end_tables_equal_the_oracle():
    from neuralsampleid_amd.frontend import CQTFrontEnd
    for fs, hop in ((22050, 512), (22050, 500), (8000, 256)):
        front, want = CQTFrontEnd(dict(CFG, fs=fs, hop_len=hop), "cpu"), CQTOracle(fs, hop)
        assert front.width == want.width and np.array_equal(front.lengths, want.lengths)
        assert np.array_equal(front.starts, want.starts) and np.array_equal(front.freqs, want.freqs)
        dense, covered = unpack(front)
        assert (covered == 1).all()                                            # every bin exactly once
        assert np.array_equal(dense.view(np.float32), want.taps.view(np.float32))          # bit for bit
        assert front.taps.dtype == torch.float32 and front.groups.dtype == np.int32 and front.groups.shape[1] == 5
        assert torch.equal(front.scale, torch.sqrt(torch.from_numpy(want.lengths.astype(np.float32))))
        # long groups first: the extents fall
        assert (np.diff(front.groups[:, 3]) < 0).all() and front.groups[0, 0] == 0
    assert front.width == 8192                                                 # the fs 8000 table
    assert CQTFrontEnd(CFG, "cpu").n_frames_of(110250) == 216


def test_top_bin_above_nyquist_is_refused():
    from neuralsampleid_amd.frontend import CQTFrontEnd
    with pytest.raises(ValueError):
        CQTFrontEnd(dict(CFG, fs=7000), "cpu")
    with pytest.raises(ValueError):
        CQTOracle(7000, 512)


def test_batch_refuses_host_tensors():
    from neuralsampleid_amd.frontend import CQTFrontEnd
    front = CQTFrontEnd(CFG, "cpu")
    with pytest.raises(RuntimeError):
        front.batch(torch.zeros(2, 9254))
    with pytest.raises(RuntimeError):
        front.cqt(torch.zeros(9254))


def test_entry_point_is_bound_and_counted():
    import ctypes
    from neuralsampleid_amd import _lib
    from neuralsampleid_amd.frontend import CQTFrontEnd
    assert _lib.SIGNATURES["nsid_cqt"] == "pliliiipiplpplls" and "nsid_cqt" in _lib.EXPORTS
    assert hasattr(_lib.lib, "nsid_cqt")
    assert _lib.launch_counters()["cqt"] == 0
    front = CQTFrontEnd(CFG, "cpu")
    g = front.groups
    host = (ctypes.c_float * 32)()                        # a non-null, 16-byte-aligned stand-in: every case below is refused on
    ptr = (ctypes.addressof(host) + 15) // 16 * 16        # the host, before anything would read it
    n, T = front.taps.numel(), 19

    def entry(wave=ptr, stride=9254, B=1, L=9254, hop=512, groups=g, n_groups=len(g), taps=ptr, taps_len=n, scale=ptr, out=ptr):
        return _lib.lib.nsid_cqt(wave, stride, B, L, hop, 16384, 84, groups.ctypes.data if groups is not None else None, n_groups,
                                 taps, taps_len, scale, out, 84 * T, T, None)
    # bad arguments are refused on the host before any launch: NSID_EINVAL = -1, and nothing is counted
    assert entry(wave=None) == -1 and entry(taps=None) == -1 and entry(scale=None) == -1 and entry(out=None) == -1
    assert entry(groups=None) == -1
    assert entry(B=0) == -1 and entry(hop=0) == -1
    assert entry(L=8192, stride=8192) == -1                                    # L <= width/2
    assert entry(stride=9253) == -1                                            # in_stride < L
    assert entry(n_groups=len(g) - 1) == -1                                    # the groups do not cover n_bins
    assert entry(groups=np.ascontiguousarray(g[::-1])) == -1                   # ... or not in order
    assert entry(taps=ptr + 4) == -1                                           # misaligned table
    assert entry(taps_len=n - 1) == -1                                         # a group's rows leave the table
    assert entry(hop=64, taps_len=1 << 40) == -1                                        # staged rows would not fit the LDS
    assert _lib.launch_counters()["cqt"] == 0


def test_module_shell_keeps_the_reference_signature():
    from neuralsampleid_amd.modules.transformations import GPUTransformCQT
    sig = inspect.signature(GPUTransformCQT.__init__)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("self", inspect.Parameter.empty), ("cfg", inspect.Parameter.empty), ("ir_dir", None), ("train", True), ("cpu", False),
        ("max_transforms_1", 1), ("max_transforms_2", 1)]
    assert list(inspect.signature(GPUTransformCQT.forward).parameters) == ["self", "x_i", "x_j"]
    m = GPUTransformCQT(CFG, ir_dir="irs", train=False)
    assert m.train is False and m.ir_dir == "irs" and m.n_frames == 216 and m.overlap == 0.5 and m.sample_rate == 22050
    assert list(m.parameters()) == [] and list(m.buffers()) == [] and m.state_dict() == {}
    with pytest.raises(NotImplementedError, match="audiomentations"):
        GPUTransformCQT(CFG, cpu=True)


def test_the_log_mel_module_still_refuses_resnet_ibn():
    from neuralsampleid_amd.modules.transformations import GPUTransformSampleID
    with pytest.raises(NotImplementedError, match="resnet-ibn") as e:
        GPUTransformSampleID(dict(CFG, n_fft=1024, win_len=1024, n_mels=64))
    assert "GPUTransformCQT" in str(e.value)
