#!/usr/bin/env python3
"""Instruction mix of the loops of AMDGPU assembly, as `hipcc -O3 -S --cuda-device-only --offload-arch=gfx950 x.hip` writes it.

A kernel that one wavefront per SIMD runs is bounded by instruction issue, not by bytes or flops, so what
matters in its hot loops is how many instructions of which class they hold.  This finds the loops of every function by their
backward branches (a branch to a label defined earlier in the function: the loop is the text between label and branch) and
prints, per loop, a count per instruction class.  Nothing here knows the band kernels: give any assembly file.

  band_loop_mix.py band.s --kernel Li527E --min 1000      # the loops of 1000 instructions and more of the functions matching
  band_loop_mix.py band.s --kernel Li527E --min 1000 --regular   # ... each without the text of the loops nested in it: in the band
                                                          # kernels' epoch loops those are the unrolled residual-row loops (rows
                                                          # i > 0 of a step), which a regular step never enters
  band_loop_mix.py band.s --resources                     # registers, spills and scratch bytes of every kernel (metadata)
  band_loop_mix.py band.s --digest                        # a hash of every function's instructions (cuid lines and comments
                                                          # dropped): equal hashes = identical device code in two builds
"""
import argparse
import hashlib
import re
import sys

LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
CLASSES = ("fp64", "valu", "salu", "smem", "waitcnt", "branch", "gload", "gstore", "lds", "scratch", "other")


def classify(op):
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_endpgm")):
        return "branch"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith(("global_load", "flat_load", "buffer_load")):
        return "gload"
    if op.startswith(("global_store", "flat_store", "buffer_store", "global_atomic", "flat_atomic")):
        return "gstore"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("v_"):
        return "fp64" if re.search(r"_f64(_|$)", op) and not op.startswith(("v_cmp", "v_cvt")) else "valu"
    return "other"


def functions(text):
    """[(name, [(label or None, opcode or None, line)])] of the functions of an assembly file"""
    out, cur, name = [], None, None
    for line in text.splitlines():
        code = line.split(";")[0].rstrip()
        if code.strip().startswith(".amdgpu_metadata"):   # YAML from here on
            break
        m = LABEL.match(code)
        if m and not m.group(1).startswith((".L", "L")):
            if cur:
                out.append((name, cur))
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        if m:
            cur.append((m.group(1), None, code))
            continue
        s = code.strip()
        if s.startswith((".Lfunc_end", ".section", ".rodata", ".amdgpu_metadata")):
            if cur:
                out.append((name, cur))
            cur, name = None, None
            continue
        if not s or s.startswith("."):
            continue
        cur.append((None, s.split()[0], s))
    if cur:
        out.append((name, cur))
    return [(n, b) for n, b in out if any(op for _, op, _ in b)]


def loops(body):
    """[(first, last)] index ranges of the loops of a function body: a branch to a label defined before it"""
    at = {lab: i for i, (lab, _, _) in enumerate(body) if lab}
    out = []
    for i, (_, op, line) in enumerate(body):
        if op and op.startswith(("s_cbranch", "s_branch")):
            tgt = line.split()[-1]
            if tgt in at and at[tgt] < i:
                out.append((at[tgt], i))
    # one loop per header: the widest range (several back edges to one header are one loop)
    best = {}
    for a, b in out:
        best[a] = max(best.get(a, b), b)
    return sorted(best.items())


def mix(body, a, b, skip=()):
    """instruction classes of body[a .. b], the index ranges of `skip` left out"""
    c = dict.fromkeys(CLASSES, 0)
    for i in range(a, b + 1):
        op = body[i][1]
        if op and not any(x <= i <= y for x, y in skip):
            c[classify(op)] += 1
    c["total"] = sum(c[k] for k in CLASSES)
    return c


def resources(text):
    pat = re.compile(r"- \.agpr_count:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?"
                     r"\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", re.S)
    return [dict(name=m.group(2), agpr=int(m.group(1)), scratch_bytes=int(m.group(3)), sgpr=int(m.group(4)), sgpr_spills=int(m.group(5)),
                 vgpr=int(m.group(6)), vgpr_spills=int(m.group(7))) for m in pat.finditer(text)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="", help="only functions whose name contains this")
    ap.add_argument("--min", type=int, default=0, help="only loops of at least this many instructions")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--digest", action="store_true")
    ap.add_argument("--regular", action="store_true", help="count a loop without the loops nested in it (the path a regular step runs)")
    a = ap.parse_args()
    text = open(a.asm).read()
    if a.resources:
        for r in resources(text):
            if a.kernel in r["name"]:
                print(r["name"], " ".join(f"{k}={v}" for k, v in r.items() if k != "name"))
        return 0
    for name, body in functions(text):
        if a.kernel not in name:
            continue
        if a.digest:
            h = hashlib.sha256("\n".join(line for _, _, line in body if "cuid" not in line).encode()).hexdigest()[:16]
            print(name, sum(1 for _, op, _ in body if op), h)
            continue
        ls = loops(body)
        print(f"{name}: {sum(1 for _, op, _ in body if op)} instructions, {len(ls)} loops")
        for lo, hi in ls:
            if mix(body, lo, hi)["total"] < a.min:
                continue
            inner = [(x, y) for x, y in ls if lo <= x and y <= hi and (x, y) != (lo, hi)] if a.regular else []
            c = mix(body, lo, hi, inner)
            depth = sum(1 for x, y in ls if x <= lo and hi <= y) - 1
            print(f"  loop {body[lo][0]} depth {depth}: " + " ".join(f"{k}={c[k]}" for k in ("total",) + CLASSES)
                  + (f"  [without {len(inner)} nested loops]" if a.regular else ""))
    if a.regular and not a.digest:
        print("note: --regular leaves out the nested loops only.  What a regular step of the band kernels also skips and this count still holds:\n"
              "the peeled iterations and remainders of those row loops, and the border-pivot blocks (the only blocks with a scalar load).")
    return 0


if __name__ == "__main__":
    sys.exit(main())
