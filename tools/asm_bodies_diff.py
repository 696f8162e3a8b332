#!/usr/bin/env python
"""Function bodies of two device-only assembly listings of one source, compared kernel by kernel:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -S --cuda-device-only icrl_amd/csrc/rollout.hip -o tree.s      (tools/asm_dump.sh's line)
    python tools/asm_bodies_diff.py parent.s tree.s [name-substring ...]

A body is what lies between a function's label and its .Lfunc_end.  Comments are dropped and the function number is taken out of the local labels
(.LBB<fn>_<block>: it moves when a kernel is added in front), so that equal means: the same instructions, operands and block structure.  Prints
the counts, every function that differs, disappeared or is new, and — for each name substring given — how many matching bodies are identical.
Exit status 1 when a function of the first listing differs or is missing in the second."""
import re
import sys


def bodies(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
        elif name is not None:
            if line.startswith(".Lfunc_end"):
                out[name], name = body, None
            else:
                line = re.sub(r"\.L(BB|tmp|func_begin|JTI)\d+", r".L\1", line.split(";")[0].rstrip())
                if line:
                    body.append(line)
    return out


def main(argv):
    a, b = bodies(argv[1]), bodies(argv[2])
    same = [k for k in a if a[k] == b.get(k)]
    diff = [k for k in a if k in b and a[k] != b[k]]
    gone = [k for k in a if k not in b]
    new = [k for k in b if k not in a]
    print(f"{argv[1]}: {len(a)} functions, {argv[2]}: {len(b)}; identical {len(same)}, different {len(diff)}, missing {len(gone)}, new {len(new)}")
    for tag, names, src in (("DIFF", diff, b), ("GONE", gone, a), ("NEW ", new, b)):
        for k in names:
            print(tag, k, f"{len(src[k])} lines" + (f" (was {len(a[k])})" if tag == "DIFF" else ""))
    for pat in argv[3:]:
        hit = [k for k in a if pat in k]
        print(f"{pat}: {sum(k in same for k in hit)} of {len(hit)} identical")
    return 1 if diff or gone else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
