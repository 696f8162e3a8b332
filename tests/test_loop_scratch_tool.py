"""tools/loop_scratch.py: the per-segment LDS wait accounting (full lgkmcnt waits, ds_read, exposed ds_read) on hand-written ISA lines.
Nothing is compiled here."""
import importlib.util
import os

_P = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "loop_scratch.py")
_spec = importlib.util.spec_from_file_location("loop_scratch_tool", _P)
ls = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ls)


def _asm(*lines):
    return ["\t" + l if not l.startswith((".", ";")) else l for l in lines]


VALU = ["v_add_f32_e32 v%d, v%d, v%d" % (i, i, i + 1) for i in range(12)]


def test_serial_reads_are_exposed():
    # read -> full wait -> 3 adds, twice: two waits, two reads, both exposed
    seg = _asm("ds_read_b128 v[24:27], v5 offset:96", "s_waitcnt lgkmcnt(0)", *VALU[:3],
               "ds_read_b128 v[24:27], v5 offset:112", "s_waitcnt lgkmcnt(0)", *VALU[3:6])
    assert ls.lds_wait_counts(seg) == (2, 2, 2)


def test_batched_reads_share_one_wait():
    # four reads back to back, then one full wait: one wait, four reads; LDS instructions between a read and the wait do not hide it
    seg = _asm(*["ds_read_b128 v[%d:%d], v5 offset:%d" % (8 * i, 8 * i + 3, 16 * i) for i in range(4)], "s_waitcnt lgkmcnt(0)", *VALU[:4])
    assert ls.lds_wait_counts(seg) == (1, 4, 4)


def test_partial_waits_and_distance():
    # a counted wait (lgkmcnt(1)) is not a full wait; a full wait 8 or more non-LDS instructions behind the read does not expose it
    seg = _asm("ds_read_b32 v1, v5", "ds_read_b32 v2, v5 offset:4", "s_waitcnt lgkmcnt(1)", *VALU[:8], "s_waitcnt lgkmcnt(0)")
    assert ls.lds_wait_counts(seg) == (1, 2, 0)
    seg = _asm("ds_read_b32 v1, v5", *VALU[:7], "s_waitcnt vmcnt(0) lgkmcnt(0)")
    assert ls.lds_wait_counts(seg) == (1, 1, 1)
    seg = _asm("ds_read_b32 v1, v5", *VALU[:7], "ds_write_b32 v5, v1", "s_waitcnt lgkmcnt(0)")      # the LDS store is not counted as cover
    assert ls.lds_wait_counts(seg) == (1, 1, 1)


def test_comments_labels_and_stores_are_not_reads():
    seg = _asm("; ds_read_b32 v1, v5", ".LBB0_3:", "ds_write_b128 v5, v[0:3]", "s_waitcnt lgkmcnt(0)", "s_waitcnt vmcnt(0)")
    assert ls.lds_wait_counts(seg) == (1, 0, 0)


def test_step_loop_and_segments():
    L = _asm(".LBB0_1:                                ; =>This Loop Header: Depth=1",
             "ds_read_b128 v[0:3], v9", "s_waitcnt lgkmcnt(0)", "v_mfma_f32_16x16x4_f32 a[0:3], v0, v1, a[0:3]",
             "s_waitcnt lgkmcnt(0)", "s_barrier",
             "ds_read_b32 v4, v9", *VALU[:9], "s_waitcnt lgkmcnt(0)",
             "s_cbranch_scc1 .LBB0_1",
             ".LBB0_2:                                ;   in Loop: Header=BB0_1 Depth=1",
             "v_mfma_f32_16x16x4_f32 a[0:3], v0, v1, a[0:3]",
             "s_branch .LBB0_1",
             ".LBB0_3:",
             "s_endpgm")
    lo, hi, n, h = ls.step_loop(L)
    assert (lo, h, n) == (0, 0, 2) and L[hi + 1] == ".LBB0_3:"
    segs = ls.segments(L, h, hi)
    assert len(segs) == 2
    assert ls.lds_wait_counts(L[segs[0][0]:segs[0][1]]) == (2, 1, 1)
    assert ls.lds_wait_counts(L[segs[1][0]:segs[1][1]]) == (1, 1, 0)
