#!/usr/bin/env python3
"""Two builds of the library on the headline workload of bench.py, alternated launch burst by launch burst.

bench.py in fresh processes compares two builds a few seconds apart, and an MI355X changes its level by several per cent on that
scale (machines that slowed down by 0.5 ms for both builds in the middle of a comparison).  This tool keeps ONE
process per build alive — each with its own handle and its own copy of the problems on the device, set up as bench.py sets them up —
and lets them take turns: `--burst` launches of build A, the same of build B, and so on for `--rounds` rounds, one build running at a
time.  A pair of bursts is about 0.1 s apart, so a change of level hits both builds alike, and the tool reports the per-round
difference beside the two medians.  It does not replace bench.py's number; it tells a small gain from the machine's drift.

  time_band_ab.py --a path/to/parent/libcannoles_hip.so --b cannoles.jl_amd/libcannoles_hip.so [--rounds 40] [--burst 5] [--batch 16384]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(args):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    s = syn.band_structure(args.n, args.ncon, name="cfg3")
    rows, cols = s.kkt_pattern()
    stream = torch.cuda.Stream(device=dev)
    vals = torch.empty((args.batch, s.nnzNS), dtype=torch.float64, device=dev)
    rhs = torch.empty((args.batch, s.N), dtype=torch.float64, device=dev)
    for b0, vh, rh in bench.band_chunks(s, 0, args.batch):
        vals[b0:b0 + len(vh)].copy_(torch.from_numpy(vh))
        rhs[b0:b0 + len(vh)].copy_(torch.from_numpy(rh))
    prob = bench.DeviceProblem(torch, hipldl, s, rows, cols, vals, rhs, args.batch, 0, stream, options=bench.parse_options(hipldl, "batch_layout=1"))
    prob.timed(2, 3)
    print(json.dumps({"ready": True, "lib": hipldl.LIB_PATH, "config": prob.L.config, "success": prob.counts()}), flush=True)
    for line in sys.stdin:
        if line.strip() == "quit":
            break
        print(json.dumps({"ms": prob.timed(int(line), 0)}), flush=True)
    prob.L.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", help="library of build A (the parent)")
    ap.add_argument("--b", help="library of build B (the branch)")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--burst", type=int, default=5, help="launches per turn")
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--ncon", type=int, default=50)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    procs = []
    for lib in (args.a, args.b):
        env = dict(os.environ, CANNOLES_HIP_LIB=os.path.abspath(lib))
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--batch", str(args.batch), "--n", str(args.n), "--ncon", str(args.ncon)],
                             stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
        procs.append(p)
    try:
        for p in procs:   # (set up one after the other's start, both before the first timed burst)
            hello = json.loads(p.stdout.readline())
            assert hello["ready"] and hello["success"][0] == hello["success"][1], hello
            print("#", hello["lib"], "mover table" if hello["config"].get("band_mover_table") else "no mover table", flush=True)
        ms = ([], [])
        for r in range(args.rounds):
            for k, p in enumerate(procs):
                p.stdin.write(f"{args.burst}\n")
                p.stdin.flush()
                ms[k].append(json.loads(p.stdout.readline())["ms"])
            print(f"round {r + 1:2d}  A {ms[0][-1]:.4f}  B {ms[1][-1]:.4f}  ({100 * (ms[1][-1] / ms[0][-1] - 1):+.2f} %)", flush=True)
    finally:
        for p in procs:
            try:
                p.stdin.write("quit\n")
                p.stdin.flush()
            except Exception:
                pass
        for p in procs:
            p.wait(timeout=60)
    rel = [100 * (b / a - 1) for a, b in zip(*ms)]
    for name, v in zip("AB", ms):
        print(f"{name}  median {statistics.median(v):.4f}  min {min(v):.4f}  max {max(v):.4f}  spread {max(v) - min(v):.4f}")
    print(f"B against A per round: median {statistics.median(rel):+.2f} %  min {min(rel):+.2f} %  max {max(rel):+.2f} %  B faster in {sum(x < 0 for x in rel)} of {len(rel)} rounds")
    return 0


if __name__ == "__main__":
    sys.exit(main())
