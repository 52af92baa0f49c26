"""GPU: the three alignment entries against each other, bit for bit. local_align, local_align_strip and local_align_panels run one walk
(csrc/align.hip al_walk); their other tests reach each of them through an oracle of its own. Here the same dyadic score blocks (ties
and paths occur) go through all three at the edges the shared code has: the block of 8 rows the walk loads at a time, a strip of one
row (the carry's second row is then the row before the strip), one column, the 256 threads' stride, and the switch from 256 to 1024
threads."""
import numpy as np
import pytest
import torch

from locate_oracle import dyadic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THETA = 0.5
LQS = (1, 2, 7, 8, 9, 17)
LRS = (1, 2, 3, 256, 257, 1024, 1025)
SHAPES = [(lq, lr) for lr in LRS for lq in LQS]
# the pairs of a launch: every pair that 256 threads take, every pair that needs 1024, and both kinds together (1024 threads for all)
LAUNCHES = {"narrow": [p for p, s in enumerate(SHAPES) if s[1] <= 1024], "wide": [p for p, s in enumerate(SHAPES) if s[1] > 1024],
            "mixed": list(range(len(SHAPES)))}
PANEL_COLS = (2, 3, 1024, 1025)
CUTS = ("whole", "row 1", "last row")


@pytest.fixture(autouse=True)
def _fp32_switches():
    from neuralsampleid_amd import functional as F_
    from neuralsampleid_amd import ops
    F_.set_activation_dtype(torch.float32)      # process-wide switches other tests move
    ops.set_gemm_precision("fp32")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class _Launch:
    """the pairs of one launch on the device, local_align's results for them (the reference of this file, computed once per top) and
    one fresh strip's"""

    def __init__(self, ops, mats):
        self.ops = ops
        self.q_len = np.array([m.shape[0] for m in mats], dtype=np.int64)
        self.x_len = np.array([m.shape[1] for m in mats], dtype=np.int64)
        self.s_ld = self.x_len + np.array([(p % 3) * 5 for p in range(len(mats))])
        size = self.q_len * self.s_ld
        self.s_off = np.cumsum(size) - size + 11
        flat = np.full(int(size.sum()) + 11, np.nan, dtype=np.float32)     # what lies between the columns is never read: NaN would show
        for m, o, ld in zip(mats, self.s_off, self.s_ld):
            for i in range(m.shape[0]):
                flat[o + i * ld:o + i * ld + m.shape[1]] = m[i]
        self.S = torch.from_numpy(flat).to(DEV)
        self.row_off = np.cumsum(self.q_len) - self.q_len
        self._whole = {}
        self._strip = None

    def whole(self, top):
        """local_align: (occ, occ_score, n_occ, row_h, row_j, row_org) on the host"""
        if top not in self._whole:
            res = self.ops.local_align(self.S, self.s_off, self.s_ld, self.q_len, self.x_len, THETA, min_score=0.0, top=top)
            assert np.array_equal(res[6], self.row_off)
            self._whole[top] = tuple(t.cpu().numpy() for t in res[:6])
        return self._whole[top]

    def strips(self, entry, cut, long_songs=False):
        """every pair from fresh through `entry` in the strips of `cut`, one launch per strip: (the four row results, the carry's three
        tensors, open_h after the last strip) on the host, and the row tensors on the device"""
        ops, P = self.ops, self.q_len.size
        first = {"whole": self.q_len, "row 1": np.minimum(1, self.q_len), "last row": self.q_len - 1}[cut]
        carry, carry_off = ops.align_carry(self.x_len, DEV, long_songs=long_songs)
        for t in carry:
            t.fill_(-7)                                                    # a fresh pair reads none of it
        total = int(self.q_len.sum())
        rows = (torch.full((total,), -7.0, device=DEV),) + tuple(torch.full((total,), -7, device=DEV, dtype=torch.int32) for _ in range(3))
        done, started, open_h = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=bool), None
        for n in ([first] if cut == "whole" else [first, self.q_len - first]):
            res = entry(self.S, self.s_off + done * self.s_ld, self.s_ld, n, self.x_len, THETA, done, (~started).astype(np.int64), carry,
                        carry_off, rows=rows, row_off=self.row_off + done)
            open_h = res[5].cpu().numpy()
            done += n
            started |= n > 0
        assert (done == self.q_len).all()
        return tuple(t.cpu().numpy() for t in rows), tuple(t.cpu().numpy() for t in carry), open_h, rows

    def strip(self):
        if self._strip is None:
            self._strip = self.strips(self.ops.local_align_strip, "whole")
        return self._strip


@pytest.fixture(scope="module")
def launches():
    from neuralsampleid_amd import ops
    rng = np.random.default_rng(2024)
    mats = [dyadic(rng, lq, lr) for lq, lr in SHAPES]
    return {name: _Launch(ops, [mats[p] for p in which]) for name, which in LAUNCHES.items()}


def _assert_rows_equal_local_align(launch, rows, msg):
    _, _, _, row_h, row_j, row_org = launch.whole(16)
    np.testing.assert_array_equal(_bits(rows[0]), _bits(row_h), err_msg=msg)
    np.testing.assert_array_equal(rows[1], row_j, err_msg=msg)
    has = row_j >= 0
    np.testing.assert_array_equal(row_org[has], (rows[2][has] << 16) | rows[3][has], err_msg=msg)
    for t in (row_org, rows[2], rows[3]):
        assert (t[~has] == -1).all(), msg
    return has


def _assert_carry_equal(got, want, msg):
    np.testing.assert_array_equal(_bits(got[1][0]), _bits(want[1][0]), err_msg=msg)
    np.testing.assert_array_equal(got[1][1], want[1][1], err_msg=msg)
    np.testing.assert_array_equal(got[1][2], want[1][2], err_msg=msg)
    np.testing.assert_array_equal(_bits(got[2]), _bits(want[2]), err_msg=msg)


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("name", list(LAUNCHES))
def test_strip_equals_local_align(launches, name, cut):
    launch = launches[name]
    got = launch.strip() if cut == "whole" else launch.strips(launch.ops.local_align_strip, cut)
    has = _assert_rows_equal_local_align(launch, got[0], f"{name}, strip cut at {cut}")
    _assert_carry_equal(got, launch.strip(), f"{name}, strip cut at {cut}")
    # the blocks do what they are here for: rows with and without a cell, paths over several rows
    rows_of = np.concatenate([np.arange(n) for n in launch.q_len])
    assert has.any() and (got[0][2][has] < rows_of[has]).any()
    assert (~has).any() or name == "wide"                                 # 3 cells of 8 pass: every row of 1025 columns has one
    assert not (got[1][0] == -7).any() and (got[2] >= 0).all()            # the whole carry and every open_h were written


@pytest.mark.parametrize("pc", PANEL_COLS)
@pytest.mark.parametrize("name", list(LAUNCHES))
def test_panels_equal_strip_and_local_align(launches, name, pc):
    launch = launches[name]
    ops = launch.ops
    before = ops.launch_counters()["local_align_panels"]
    got = launch.strips(lambda *a, **kw: ops.local_align_panels(*a, panel_cols=pc, **kw), "whole", long_songs=True)
    assert ops.launch_counters()["local_align_panels"] == before + 1
    _assert_rows_equal_local_align(launch, got[0], f"{name}, panels of {pc}")
    _assert_carry_equal(got, launch.strip(), f"{name}, panels of {pc}")


@pytest.mark.parametrize("top", [1, 16])
@pytest.mark.parametrize("name", list(LAUNCHES))
def test_occurrences_of_the_strip_rows_equal_local_align(launches, name, top):
    launch = launches[name]
    occ, sc, n_occ = launch.whole(top)[:3]
    rows = launch.strip()[3]
    got = launch.ops.align_occurrences(*rows, launch.row_off, launch.q_len, np.zeros_like(launch.q_len), min_score=0.0, top=top)
    np.testing.assert_array_equal(got[0].cpu().numpy(), occ)
    np.testing.assert_array_equal(_bits(got[1].cpu().numpy()), _bits(sc))
    np.testing.assert_array_equal(got[2].cpu().numpy(), n_occ)
    assert (n_occ > 1).any()                                             # with top = 1: more occurrences than slots
