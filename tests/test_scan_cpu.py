"""CPU: the strip-chained oracle of the scan against the cell loop of the whole matrix, the occurrence rule over unpacked origins, the
active-set rule by hand, and every name, limit and refusal of the scan's entries without a device."""
import numpy as np
import pytest
import torch

from locate_oracle import align_cells, align_rows, dyadic, occurrences
from scan_oracle import align_chained, occurrences_unpacked, replay_active, rows_from_cells

CUTS = [(37,), (1,) * 37, (2, 0, 1, 30, 4), (36, 1)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("cuts", CUTS, ids=lambda c: "x".join(map(str, c[:5])))
@pytest.mark.parametrize("Lr", [1, 2, 3, 33])
@pytest.mark.parametrize("row_base", [0, 32760])
def test_chained_oracle_equals_the_cell_loop_on_the_whole_matrix(Lr, cuts, row_base):
    Lq = 37
    S = dyadic(np.random.default_rng(1000 + Lr), Lq, Lr)
    H, org = align_cells(S, 0.5)
    want = rows_from_cells(S, 0.5, H, org, row_base)
    got = align_chained(S, 0.5, cuts, row_base)
    np.testing.assert_array_equal(_bits(want[0]), _bits(got[0]))
    for u in (1, 2, 3):
        np.testing.assert_array_equal(want[u], got[u])
    # the carry after the last strip is the last two rows of the whole matrix, and open_h their largest H
    ch, ci, cj = got[4]
    for r in (0, 1):
        i = Lq - 1 - r
        np.testing.assert_array_equal(_bits(ch[r]), _bits(H[i]))
        np.testing.assert_array_equal(ci[r], np.where(org[i] >= 0, (org[i] >> 16) + row_base, -1))
        np.testing.assert_array_equal(cj[r], np.where(org[i] >= 0, org[i] & 0xffff, -1))
    assert got[5][-1] == max(H[Lq - 1].max(), H[Lq - 2].max())
    if Lr == 33:
        assert (got[2] >= 0).sum() > 10 and len(set(got[0][got[0] > 0].tolist())) < (got[0] > 0).sum()      # paths, and exact ties


def test_occurrences_unpacked_equals_the_packed_rule():
    S = dyadic(np.random.default_rng(5), 80, 40)
    row_h, row_j, row_org = align_rows(S, 0.5)
    i0 = np.where(row_org >= 0, row_org >> 16, -1)
    j0 = np.where(row_org >= 0, row_org & 0xffff, -1)
    for top, min_score in ((1, 0.0), (16, 0.75), (64, 0.0)):
        a = occurrences(row_h, row_j, row_org, min_score, top)
        b = occurrences_unpacked(row_h, row_j, i0, j0, 0, min_score, top)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(_bits(a[1]), _bits(b[1]))
        assert a[2] == b[2] and a[2] > 1
    occ, _, _ = occurrences_unpacked(row_h, row_j, i0 + 500, j0, 500, 0.0, 16)             # a run that starts at global row 500
    want = occurrences(row_h, row_j, row_org, 0.0, 16)[0]
    np.testing.assert_array_equal(occ[:, :2], np.where(want[:, :2] >= 0, want[:, :2] + 500, -1))


def test_active_set_rule_by_hand():
    votes = [[3, 1], [1, 4], [], [2], [2]]
    opens = [{3: 2.0, 1: 0.0}, {3: 1.0, 1: 1.0, 4: 0.5}, {1: 0.0, 3: 0.0, 4: 3.0}, {4: 0.0, 2: 1.0}, {2: 0.0}]
    active, closed, runs = replay_active(votes, opens, n_songs=2, max_active=64)
    # window 1: 3 continues (open), 1 is voted again although nothing of it is open: it goes behind the continuing song and its run goes on
    assert active == [[3, 1], [3, 1, 4], [1, 3, 4], [4, 2], [2]]
    assert closed == 0
    assert runs == [(1, 0, 2), (3, 0, 2), (4, 1, 3), (2, 3, 4)]
    active, closed, _ = replay_active(votes, opens, n_songs=1, max_active=64)
    assert active[0] == [3] and active[1] == [3, 1]
    active, closed, _ = replay_active([[3, 1], [1]], [{3: 2.0}, {3: 1.0}], n_songs=2, max_active=1)
    assert active == [[3], [3]] and closed == 2


# ------------------------------------------------------------------------------------------------ names, limits, refusals
def test_names_and_counters():
    from neuralsampleid_amd import _lib, ops
    assert "nsid_local_align_strip" in _lib.SIGNATURES and "nsid_align_occurrences" in _lib.SIGNATURES
    assert _lib.SIGNATURES["nsid_local_align_strip"] == "ppppppp" + "iii" + "f" + "pppppppppp" + "s"
    assert _lib.SIGNATURES["nsid_align_occurrences"] == "ppppppp" + "ii" + "f" + "i" + "ppp" + "s"
    c = ops.launch_counters()
    assert "local_align_strip" in c and "align_occurrences" in c
    keys = list(c)
    assert keys[keys.index("local_align"):][:3] == ["local_align", "local_align_strip", "align_occurrences"]    # beside their family
    assert ops.ALIGN_OCC_MAX_ROWS == _lib.DEFINES["NSID_ALIGN_OCC_MAX_ROWS"] >= 1 << 17     # a day of rows and more


def test_c_entries_refuse_before_any_launch():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd._lib import DEFINES, lib
    before = ops.launch_counters()
    einval = DEFINES["NSID_EINVAL"]
    N = None

    def c_strip(npairs=1, max_q=8, max_x=9, theta=0.5, ptr=None):
        return lib.nsid_local_align_strip(ptr, ptr, ptr, ptr, ptr, ptr, ptr, npairs, max_q, max_x, theta, ptr, ptr, ptr, ptr, ptr, ptr,
                                          ptr, ptr, ptr, ptr, N)

    def c_occ(npairs=1, max_rows=8, min_score=0.0, top=16, ptr=None):
        return lib.nsid_align_occurrences(ptr, ptr, ptr, ptr, ptr, ptr, ptr, npairs, max_rows, min_score, top, ptr, ptr, ptr, N)

    assert c_strip(npairs=0) == 0 and c_occ(npairs=0) == 0                                 # nothing to do
    assert c_strip() == einval and c_occ() == einval                                       # null pointers
    assert c_strip(ptr=0x1002) == einval and c_occ(ptr=0x1002) == einval                   # misaligned (refused before anything is read)
    assert c_strip(ptr=0x1004) == einval and c_occ(ptr=0x1004) == einval                   # the int64 tables need 8 bytes
    for kw in ({"max_q": 4097}, {"max_x": 4097}, {"npairs": -1}, {"max_q": -1}, {"max_x": -1}, {"theta": float("nan")}):
        assert c_strip(**{"npairs": 0, **kw}) == einval, kw                                # refused although there is no pair to run
    for kw in ({"max_rows": DEFINES["NSID_ALIGN_OCC_MAX_ROWS"] + 1}, {"max_rows": -1}, {"top": 0}, {"top": 65}, {"npairs": -1},
               {"min_score": float("nan")}):
        assert c_occ(**{"npairs": 0, **kw}) == einval, kw
    assert ops.launch_counters() == before


def test_ops_refuse_before_the_device():
    from neuralsampleid_amd import ops
    before = ops.launch_counters()
    S = torch.zeros(72)
    carry = (torch.zeros(18), torch.zeros(18, dtype=torch.int32), torch.zeros(18, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        ops.local_align_strip(S, [0], [9], [8], [9], 0.5, [0], [1], carry, [0])             # CPU tensors
    with pytest.raises(TypeError):
        ops.local_align_strip(S.numpy(), [0], [9], [8], [9], 0.5, [0], [1], carry, [0])
    rows = (torch.zeros(8), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        ops.align_occurrences(*rows, [0], [8], [0])
    with pytest.raises(TypeError):
        ops.align_occurrences(rows[0].numpy(), *rows[1:], [0], [8], [0])
    with pytest.raises(ValueError, match="4096"):
        ops.align_carry([4097], "cpu")
    assert ops.launch_counters() == before


def test_scanner_refuses_before_the_device():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd.identify import SampleIndex
    before = ops.launch_counters()
    idx = SampleIndex(None)
    with pytest.raises(ValueError, match="threshold"):
        idx.scanner()
    with pytest.raises(ValueError, match="threshold"):
        idx.scan(fp=torch.zeros(10, 128))
    with pytest.raises(ValueError):
        idx.scanner(threshold=float("nan"))
    for top in (0, 65):
        with pytest.raises(ValueError, match="top"):
            idx.scanner(threshold=0.5, top=top)
    with pytest.raises(KeyError):
        idx.scanner(threshold=0.5, songs=["no such song"])
    with pytest.raises(KeyError):
        idx.scanner(threshold=0.5, exclude="no such song")
    with pytest.raises(TypeError):
        idx.scanner(threshold=0.5, songs="abc")
    with pytest.raises(ValueError):
        idx.scanner(threshold=0.5, songs=[], exclude="x")
    for kw in ({"n_songs": 0}, {"max_active": 0}, {"k_probe": 65}, {"window_rows": 0}, {"row_hop_s": 0.5}):
        with pytest.raises(ValueError):
            idx.scanner(threshold=0.5, **kw)
    sc = idx.scanner(threshold=0.5)
    assert sc.window_rows == ops.VOTE_MAX_CAND // 20
    assert idx.scanner(threshold=0.5, window_rows=100000, k_probe=1).window_rows == ops.ALIGN_MAX_ROWS
    assert idx.scanner(threshold=0.5, window_rows=300).window_rows == ops.VOTE_MAX_CAND // 20
    with pytest.raises(RuntimeError):
        sc.push(torch.zeros(10, 128))                                                      # a CPU tensor
    with pytest.raises(ValueError):
        sc.push(torch.zeros(10, 100))                                                      # d outside the search's widths
    with pytest.raises(ValueError):
        sc.push(torch.zeros(10))
    assert sc.finish() == [] and sc.stats["windows"] == 0
    with pytest.raises(RuntimeError):
        sc.push(torch.zeros(0, 128))
    assert ops.launch_counters() == before
