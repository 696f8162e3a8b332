"""tools/loop_scratch.py --loop-by instr: the step loop of a kernel without MFMAs (the persistent rollout) is the depth-1 loop with the most
instructions; the default still picks the loop that holds the MFMAs.  Hand-written ISA lines, nothing is compiled here."""
import importlib.util
import os

import pytest

_P = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "loop_scratch.py")
_spec = importlib.util.spec_from_file_location("loop_scratch_tool_rollout", _P)
ls = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ls)


def _asm(*lines):
    return ["\t" + l if not l.startswith((".", ";")) else l for l in lines]


VALU = ["v_add_f64 v[%d:%d], v[%d:%d], v[%d:%d]" % (2 * i, 2 * i + 1, 2 * i, 2 * i + 1, 2 * i + 2, 2 * i + 3) for i in range(12)]

# loop A (header BB0_1): short, two MFMAs (a weight-load loop in front of the step loop);
# loop B (header BB0_4): long, no MFMA, two barrier segments and a nested depth-2 poll loop that belongs to it
_TEXT = _asm(
    ".LBB0_1:                                ; =>This Loop Header: Depth=1",
    "v_mfma_f32_16x16x4_f32 a[0:3], v0, v1, a[0:3]",
    "s_cbranch_scc0 .LBB0_3",
    ".LBB0_2:                                ;   in Loop: Header=BB0_1 Depth=1",
    "v_mfma_f32_16x16x4_f32 a[0:3], v0, v1, a[0:3]",
    "s_branch .LBB0_1",
    ".LBB0_3:",
    "s_mov_b32 s4, 0",
    ".LBB0_4:                                ; =>This Loop Header: Depth=1",
    "ds_read_b64 v[0:1], v9", "s_waitcnt lgkmcnt(0)", *VALU[:6], "v_readlane_b32 s5, v40, 3",
    "s_barrier",
    ".LBB0_5:                                ;   Parent Loop BB0_4 Depth=1",
    "                                        ; =>  This Inner Loop Header: Depth=2",
    "buffer_load_dwordx4 v[20:23], v8, s[12:15], 0 offen",
    "s_cbranch_vccnz .LBB0_5",
    ".LBB0_6:                                ;   in Loop: Header=BB0_4 Depth=1",
    "ds_read_b64 v[2:3], v9 offset:8", *VALU[:9], "s_waitcnt lgkmcnt(0)",
    "v_div_fixup_f64 v[4:5], v[4:5], v[6:7], v[2:3]",
    "s_cbranch_scc1 .LBB0_4",
    ".LBB0_7:",
    "s_endpgm")


def test_default_still_picks_the_mfma_loop():
    lo, hi, n, h = ls.step_loop(_TEXT)
    assert (lo, h, n) == (0, 0, 2) and _TEXT[hi + 1] == ".LBB0_3:"
    assert ls.step_loop(_TEXT, "mfma") == (lo, hi, n, h)


def test_loop_by_instr_picks_the_longest_depth1_loop():
    lo, hi, n, h = ls.step_loop(_TEXT, "instr")
    head = _TEXT.index(".LBB0_4:                                ; =>This Loop Header: Depth=1")
    assert (lo, h, n) == (head, head, 0) and _TEXT[hi + 1] == ".LBB0_7:"
    # the nested poll loop's lines are inside the range
    assert any("buffer_load_dwordx4" in l for l in _TEXT[lo:hi])
    segs = ls.segments(_TEXT, h, hi)
    assert len(segs) == 2
    assert ls.lds_wait_counts(_TEXT[segs[0][0]:segs[0][1]]) == (1, 1, 1)
    assert ls.lds_wait_counts(_TEXT[segs[1][0]:segs[1][1]]) == (1, 1, 0)


def test_main_prints_the_chosen_loop_and_its_segments(tmp_path, capsys):
    p = tmp_path / "k.s"
    p.write_text("\n".join(_TEXT))
    ls.main(str(p))
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("loop lines 0..") and "2 MFMAs" in out[0] and len(out) == 2
    ls.main(str(p), "instr")
    out = capsys.readouterr().out.splitlines()
    assert "0 MFMAs" in out[0] and len(out) == 3
    assert out[1].rstrip().endswith("readlane 1 f64div 0 barriers 0")      # a segment ends in front of its barrier
    assert out[2].rstrip().endswith("readlane 0 f64div 1 barriers 1")


def test_unknown_selector_is_refused():
    with pytest.raises(ValueError):
        ls.step_loop(_TEXT, "longest")
