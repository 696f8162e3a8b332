"""in-loop scratch traffic and LDS waits of an update kernel's ISA (tools/asm_dump.sh output):  python tools/loop_scratch.py kernel.s [--loop-by instr]
prints, for the optimiser-step loop (the depth-1 loop that holds the MFMAs; --loop-by instr: the depth-1 loop with the most instructions, for kernels
without MFMAs such as the persistent rollout, whose env-step loop it then finds), per barrier segment: the scratch loads / stores and v_accvgpr moves, the
`s_waitcnt` with lgkmcnt(0), the ds_read and how many of them are EXPOSED — followed by a full lgkmcnt wait with fewer than EXPOSED_WINDOW non-LDS
instructions in between, i.e. the wave sits out (most of) the LDS latency of that read"""
import re, sys

EXPOSED_WINDOW = 8


def is_instr(l):
    return l.startswith("\t") and not l.strip().startswith((";", "."))


def is_lds(l):
    return is_instr(l) and l.strip().startswith("ds_")


def is_ds_read(l):
    return is_instr(l) and l.strip().startswith(("ds_read", "ds_load"))


def is_full_lgkm_wait(l):
    return is_instr(l) and "s_waitcnt" in l and re.search(r"lgkmcnt\(0\)", l) is not None


def lds_wait_counts(seg, window=EXPOSED_WINDOW):
    """(full lgkmcnt waits, ds_read, exposed ds_read) of a list of ISA lines"""
    ins = [l for l in seg if is_instr(l)]
    waits = sum(is_full_lgkm_wait(l) for l in ins)
    reads = exposed = 0
    for i, l in enumerate(ins):
        if not is_ds_read(l):
            continue
        reads += 1
        other = 0
        for m in ins[i + 1:]:
            if is_full_lgkm_wait(m):
                exposed += 1
                break
            if not is_lds(m):
                other += 1
                if other >= window:
                    break
    return waits, reads, exposed


def step_loop(L, by="mfma"):
    """(first line, last line, MFMAs, header line) of the depth-1 loop with the most MFMAs (by="instr": with the most instructions)"""
    if by not in ("mfma", "instr"):
        raise ValueError(f"--loop-by {by}: mfma or instr")
    best = None
    for h, l in enumerate(L):
        m = re.match(r"^\.(LBB\d+_\d+):\s*; =>This Loop Header: Depth=1", l)
        if not m:
            continue
        tag = "Header=" + m.group(1)[1:]
        members = [i for i, x in enumerate(L) if tag in x]
        if not members:
            continue
        lo, hi = min(h, min(members)), max(members)
        # the last member block runs until the next label
        while hi + 1 < len(L) and not re.match(r"^\.LBB\d+_\d+:", L[hi + 1]):
            hi += 1
        n = sum(1 for x in L[lo:hi] if "v_mfma" in x)
        key = n if by == "mfma" else sum(1 for x in L[lo:hi] if is_instr(x))
        if best is None or key > best[0]:
            best = (key, lo, hi, n, h)
    return best[1:] if best is not None else None


def segments(L, h, hi):
    bars = [h] + [i for i in range(h, hi) if "s_barrier" in L[i]] + [hi]
    return list(zip(bars, bars[1:]))


def main(path, by="mfma"):
    L = open(path).read().split("\n")
    lo, hi, n, h = step_loop(L, by)
    w, r, e = lds_wait_counts(L[lo:hi])
    print(f"loop lines {lo}..{hi} (header {h}): {hi - lo} lines, {n} MFMAs, scratch {sum('scratch_' in l for l in L[lo:hi])}, "
          f"instr {sum(is_instr(l) for l in L[lo:hi])}, lgkm0 {w}, ds_read {r}, exposed {e}")
    for a, b in segments(L, h, hi):
        seg = L[a:b]
        ins = sum(1 for l in seg if is_instr(l))
        w, r, e = lds_wait_counts(seg)
        print(f"  [{a}-{b}] instr {ins} scratch_load {sum('scratch_load' in l for l in seg)} scratch_store {sum('scratch_store' in l for l in seg)} "
              f"accvgpr {sum('v_accvgpr' in l for l in seg)} ds {sum(chr(9) + 'ds_' in l for l in seg)} mfma {sum('v_mfma' in l for l in seg)} branches {sum('s_cbranch' in l for l in seg)} "
              f"lgkm0 {w} ds_read {r} exposed {e}" +
              (f" readlane {sum('v_readlane' in l for l in seg)} f64div {sum('v_div_fixup_f64' in l for l in seg)} barriers {sum('s_barrier' in l for l in seg)}" if by == "instr" else ""))


if __name__ == "__main__":
    args = sys.argv[1:]
    by = "mfma"
    if "--loop-by" in args:
        i = args.index("--loop-by")
        by = args[i + 1]
        del args[i:i + 2]
    main(args[0], by)
