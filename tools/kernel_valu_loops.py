#!/usr/bin/env python3
"""Static VALU and lane-move counts of ONE kernel, per loop and per source function (no GPU needed).

Reads a device-only assembly build with line tables (built here with the library's flags plus
-gline-tables-only when no .s file is given) and prints, for the first kernel whose mangled name
contains every FILTER word:

  * the whole kernel, and its prologue (everything before the first loop);
  * every loop -- a backward branch to a label; the loop is the text from the label to the branch --
    with the source line and function of its backward branch (the for / while statement, or what was
    inlined there), its nesting depth, the VALU instructions (v_*) and the lane moves among them
    (v_readlane_b32 / v_writelane_b32: scalar registers parked in VGPR lanes) of the whole loop and of
    the loop without its inner loops ("own");
  * the same two counts per source function, from the .loc line of each instruction (the function whose
    definition precedes the line in its file; inlined code counts for the function it was written in).

Static counts: weigh them by trip counts before comparing.  --weights takes
"FIRST-LAST=W,..." -- loops named by the instruction range the listing prints -- and prints
sum(W * the loop's lane moves, inner loops included), the figure the rounds compare (the item loop x 1,
the box-scan loop x 1, the resolve loop x 3.79 tiles per busy group; the resolve loop holds two bodies, of which a
wave runs one: read its listing before weighing its VALU count).

usage: tools/kernel_valu_loops.py [--asm FILE.s] [--src csrc/shs_legacy.hip] [--extra "-DFLAG"]
                                  [--weights "243-4974=1,713-969=1,2818-4002=3.79"] FILTER [FILTER ...]
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "leisure-software-renderer_amd")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S", "-gline-tables-only"]
LANE = ("v_readlane_b32", "v_writelane_b32")
FUNC_RE = re.compile(r"^\s*(?:template\s*<[^>]*>\s*)?(?:static\s+|inline\s+)*(?:__device__|__global__|__host__)\b[^;=]*?\b(\w+)\s*\($")


def build_asm(src, extra):
    cmd = ["/opt/rocm/bin/hipcc"] + FLAGS + extra.split() + ["-o", "-", src]
    return subprocess.run(cmd, cwd=ROOT, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout


def function_starts(path):
    """[(line, name)] of the function definitions of a source file, by a crude match of their first line."""
    out = []
    try:
        with open(path) as f:
            for n, line in enumerate(f, 1):
                head = line.split("(")[0] + "(" if "(" in line else line
                m = FUNC_RE.match(head.rstrip())
                if m and not line.rstrip().endswith(";"):
                    out.append((n, m.group(1)))
    except OSError:
        pass
    return out


def function_of(starts, line):
    name = "?"
    for n, f in starts:
        if n > line:
            break
        name = f
    return name


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm")
    ap.add_argument("--src", default="csrc/shs_legacy.hip")
    ap.add_argument("--extra", default="")
    ap.add_argument("--weights", default="")
    ap.add_argument("filter", nargs="+")
    a = ap.parse_args()
    text = open(a.asm).read() if a.asm else build_asm(a.src, a.extra)
    lines = text.split("\n")

    files = {}
    for l in lines:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            d, f = (m.group(2), m.group(3)) if m.group(3) else ("", m.group(2))
            p = os.path.join(d, f)
            files[int(m.group(1))] = p if os.path.isabs(p) else os.path.join(ROOT, p)

    start = end = None
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if start is None and m and all(w in m.group(1) for w in a.filter):
            start, name = i, m.group(1)
        elif start is not None and l.startswith(".Lfunc_end"):
            end = i
            break
    if start is None:
        sys.exit("no kernel matches " + " ".join(a.filter))

    # instructions: (is lane move, file, line); labels and branches by instruction index
    insts, label_at, branches = [], {}, []
    loc = (0, 0)
    for l in lines[start + 1:end]:
        t = l.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            loc = (int(m.group(1)), int(m.group(2)))
            continue
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            label_at[m.group(1)] = len(insts)
            continue
        if not t or t[0] in ".;":
            continue
        op = t.split(None, 1)[0]
        if op.startswith("s_cbranch") or op == "s_branch":
            branches.append((len(insts), t.split()[1]))
        insts.append((op.startswith("v_"), op in LANE, loc))

    loops = sorted({(label_at[lb], at) for at, lb in branches if lb in label_at and label_at[lb] <= at})
    # merge back-edges that share a header: the loop runs to the last of them
    merged = {}
    for lo, hi in loops:
        merged[lo] = max(hi, merged.get(lo, hi))
    loops = sorted(merged.items(), key=lambda r: (r[0], -r[1]))

    def count(lo, hi, skip=()):
        v = m = 0
        for i in range(lo, hi + 1):
            if any(s <= i <= e for s, e in skip):
                continue
            v += insts[i][0]
            m += insts[i][1]
        return v, m

    starts = {k: function_starts(p) for k, p in files.items()}

    def where(i):
        f, ln = insts[i][2]
        return f"{os.path.basename(files.get(f, '?'))}:{ln}", function_of(starts.get(f, []), ln), ln

    print(name)
    v, m = count(0, len(insts) - 1)
    print(f"  whole kernel                         VALU={v:5d} lane_moves={m:4d}")
    if loops:
        v, m = count(0, loops[0][0] - 1)
        print(f"  prologue (before the first loop)     VALU={v:5d} lane_moves={m:4d}")
    print("  loops (named by the source line and function of their backward branch)")
    by_range = {}
    for lo, hi in loops:
        depth = sum(1 for s, e in loops if s <= lo and hi <= e and (s, e) != (lo, hi))
        inner = [(s, e) for s, e in loops if lo <= s and e <= hi and (s, e) != (lo, hi)]
        vi, mi = count(lo, hi)
        vx, mx = count(lo, hi, inner)
        # the loop's source line: the line of its back-edge branch (the for / while statement)
        w, fn, ln = where(hi)
        by_range[f"{lo}-{hi}"] = mi
        print(f"  {'  ' * depth}loop @{w:22s} {fn:22s} insts {lo:5d}-{hi:5d}  VALU={vi:5d} lane_moves={mi:4d}"
              f"   own: VALU={vx:5d} lane_moves={mx:4d}")
    print("  per source function")
    per = {}
    for i, (isv, isl, _) in enumerate(insts):
        if isv:
            fn = where(i)[1]
            r = per.setdefault(fn, [0, 0])
            r[0] += 1
            r[1] += isl
    for fn, (v, m) in sorted(per.items(), key=lambda r: -r[1][0]):
        print(f"    {fn:28s} VALU={v:5d} lane_moves={m:4d}")
    if a.weights:
        tot = 0.0
        for part in a.weights.split(","):
            rng, w = part.split("=")
            if rng not in by_range:
                sys.exit(f"no loop over instructions {rng}")
            n = by_range[rng]
            tot += float(w) * n
            print(f"  weight {float(w):5.2f} x {n:4d} lane moves (loop {rng})")
        print(f"  weighted lane moves: {tot:.0f}")


if __name__ == "__main__":
    main()
