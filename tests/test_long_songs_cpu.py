"""CPU: songs past 4096 rows -- the limit, the names and the refusals of nsid_local_align_panels / nsid_align_occurrences_span
(include/nsid.h), of their ops wrappers and of SampleIndex(long_songs=True). Nothing here launches anything."""
import pytest
import torch


def test_names_limit_and_counters():
    from neuralsampleid_amd import _lib, ops
    assert ops.ALIGN_MAX_SONG_ROWS == _lib.DEFINES["NSID_ALIGN_MAX_SONG_ROWS"] == 16384
    # the two packing arguments of csrc/align.hip at that bound: j0 in 16 bits, i - i0 <= 2 (Lr - 1) below 2^15
    assert ops.ALIGN_MAX_SONG_ROWS <= 1 << 16 and 2 * (ops.ALIGN_MAX_SONG_ROWS - 1) < 1 << 15 <= 2 * ops.ALIGN_MAX_SONG_ROWS
    assert _lib.SIGNATURES["nsid_local_align_panels"] == "ppppppp" + "iiii" + "f" + "pppp" + "pppp" + "pppppp" + "s"
    assert _lib.SIGNATURES["nsid_align_occurrences_span"] == "pppppppp" + "ii" + "f" + "i" + "ppp" + "s"
    c = ops.launch_counters()
    assert "local_align_panels" in c and "align_occurrences_span" in c


def test_c_entries_refuse_before_any_launch():
    from neuralsampleid_amd import ops
    from neuralsampleid_amd._lib import DEFINES, lib
    before = ops.launch_counters()
    einval = DEFINES["NSID_EINVAL"]
    N = None

    def c_panels(npairs=1, max_q=8, max_x=9, panel_cols=4, theta=0.5, ptr=None):
        return lib.nsid_local_align_panels(ptr, ptr, ptr, ptr, ptr, ptr, ptr, npairs, max_q, max_x, panel_cols, theta, ptr, ptr, ptr, ptr,
                                           ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, N)

    def c_occ(npairs=1, max_rows=8, min_score=0.0, top=16, ptr=None):
        return lib.nsid_align_occurrences_span(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, npairs, max_rows, min_score, top, ptr, ptr, ptr, N)

    assert c_panels(npairs=0) == 0 and c_occ(npairs=0) == 0                                # nothing to do
    assert c_panels(npairs=0, max_x=16384, max_q=4096, panel_cols=4096) == 0 and c_panels(npairs=0, panel_cols=2) == 0
    assert c_panels() == einval and c_occ() == einval                                      # null pointers
    assert c_panels(ptr=0x1002) == einval and c_occ(ptr=0x1002) == einval                  # misaligned (refused before anything is read)
    assert c_panels(ptr=0x1004) == einval and c_occ(ptr=0x1004) == einval                  # the int64 tables need 8 bytes
    for kw in ({"max_q": 4097}, {"max_x": 16385}, {"panel_cols": 1}, {"panel_cols": 4097}, {"panel_cols": 0}, {"npairs": -1},
               {"max_q": -1}, {"max_x": -1}, {"theta": float("nan")}):
        assert c_panels(**{"npairs": 0, **kw}) == einval, kw                               # refused although there is no pair to run
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
        ops.local_align_panels(S, [0], [9], [8], [9], 0.5, [0], [1], carry, [0])            # CPU tensors
    with pytest.raises(TypeError):
        ops.local_align_panels(S.numpy(), [0], [9], [8], [9], 0.5, [0], [1], carry, [0])
    for pc in (1, 4097):
        with pytest.raises(ValueError, match="panel_cols"):
            ops.local_align_panels(S, [0], [9], [8], [9], 0.5, [0], [1], carry, [0], panel_cols=pc)
    rows = (torch.zeros(8), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        ops.align_occurrences(*rows, [0], [8], [0], span=[14])
    # lengths past 16384, by number; the calls without the keyword refuse what they refused
    with pytest.raises(ValueError, match="16384"):
        ops.align_carry([16385], "cpu", long_songs=True)
    with pytest.raises(ValueError, match="4096"):
        ops.align_carry([4097], "cpu")
    assert ops.align_carry([16384, 5], "cpu", long_songs=True)[1].tolist() == [0, 32768]
    q = torch.zeros(8, 128)
    with pytest.raises(ValueError, match="16384"):
        ops.pair_sim(q, q, [0], [8], [0], [16385], long_songs=True)
    with pytest.raises(ValueError, match="4096"):
        ops.pair_sim(q, q, [0], [8], [0], [4097])
    with pytest.raises(ValueError, match="4096"):
        ops.pair_sim(q, q, [0], [4097], [0], [8], long_songs=True)                          # the query side of one strip stays
    assert ops.launch_counters() == before


def test_ops_refuse_bad_values_on_cpu_tensors_too():
    """with CPU tensors the tensor check comes first (test_long_songs_gpu.py has these on the device, as ValueError); what must hold
    here is that the call is refused and nothing launches"""
    from neuralsampleid_amd import ops
    before = ops.launch_counters()
    S = torch.zeros(72)
    carry = (torch.zeros(18), torch.zeros(18, dtype=torch.int32), torch.zeros(18, dtype=torch.int32))
    with pytest.raises((RuntimeError, ValueError)):
        ops.local_align_panels(S, [0], [9], [8], [9], float("nan"), [0], [1], carry, [0])
    with pytest.raises((RuntimeError, ValueError)):
        ops.local_align_panels(S, [0], [16385], [1], [16385], 0.5, [0], [1], carry, [0])
    assert ops.launch_counters() == before


def _fake_index(long_songs, rows):
    from neuralsampleid_amd.identify import SampleIndex
    idx = SampleIndex(None, long_songs=long_songs)
    idx._d = 128
    for code, (name, n) in enumerate(rows):
        idx.names.append(name)
        idx._code[name] = code
        idx._song_rows.append((sum(r for _, r in rows[:code]), n, 0))
    return idx


def test_index_refuses_a_song_past_the_bound_by_name_and_number():
    from neuralsampleid_amd import ops
    before = ops.launch_counters()
    idx = _fake_index(True, [("short", 100), ("a mix", 16385)])
    assert idx.long_songs
    fp = torch.zeros(10, 128)
    with pytest.raises(ValueError, match=r"'a mix' has 16385 rows.*16384"):
        idx.align(fp, ["a mix"], threshold=0.5)
    with pytest.raises(ValueError, match=r"'a mix' has 16385 rows.*16384"):
        idx.locate(fp=fp, songs=["short", "a mix"], threshold=0.5)
    with pytest.raises(ValueError, match=r"'a mix' has 16385 rows.*16384"):
        idx.scanner(threshold=0.5, songs=["a mix"])
    with pytest.raises(ValueError, match=r"query of 16385 rows.*16384"):
        idx.align(torch.zeros(16385, 128), ["short"], threshold=0.5)
    # the default index on the same table: today's limit, today's words
    idx = _fake_index(False, [("short", 100), ("a mix", 4097)])
    assert not idx.long_songs
    with pytest.raises(ValueError, match=r"'a mix' has 4097 rows, past the limit of 4096; longer inputs are refused, not split"):
        idx.align(fp, ["a mix"], threshold=0.5)
    with pytest.raises(ValueError, match=r"'a mix' has 4097 rows, past the limit of 4096"):
        idx.scanner(threshold=0.5, songs=["a mix"])
    with pytest.raises(ValueError, match=r"query of 4097 rows is past the limit of 4096"):
        idx.align(torch.zeros(4097, 128), ["short"], threshold=0.5)
    assert ops.launch_counters() == before
