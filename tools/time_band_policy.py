#!/usr/bin/env python3
"""The cache policies of the band kernel's mover-table instance (tuning band_cache_policy) on the headline workload of bench.py,
alternated launch burst by launch burst inside ONE process.

tools/time_band_ab.py compares two libraries from two processes; the policies are instances of one library, so one process holds
ONE copy of the problems on the device — set up as bench.DeviceProblem sets them up — and one handle per policy, each with its own
factor records.  The handles take turns: `--burst` launches of one, then of the next, for `--rounds` rounds, in an order that
rotates every round, so that a change of the machine's level hits every arm alike.  TWO handles of policy 0 serve as the control:
what one differs from the other by is what the method cannot tell from nothing.  (Every policy computes the same bits, so the shared
`vals` — whose rho slots a launch rewrites — are the same array whichever handle ran last.)

It reports per-policy medians, the per-round difference of every arm to the first policy-0 handle, the rounds each arm won, and the
control's own difference, as text and as one JSON line.

  time_band_policy.py [--policies 1,3,7] [--rounds 40] [--burst 5] [--batch 16384] [--opt band_problems_per_group=32]

Without --policies every mask from 1 to 31 is tried and those the library has no instance for are skipped (csrc/band.hip,
BAND_POLICY_MASKS, names the masks that are built).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--policies", default="", help="comma-separated masks (default: every mask the library has an instance for)")
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--burst", type=int, default=5, help="launches per turn")
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--ncon", type=int, default=50)
    ap.add_argument("--opt", default="", help="further tuning keys of every handle, key=value[,key=value] (e.g. band_problems_per_group=32)")
    args = ap.parse_args()
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

    extra = {k: int(v) for k, v in (item.split("=", 1) for item in args.opt.split(",") if item)}

    def options(mask):
        return hipldl.Options(batch_layout=1, band_cache_policy=mask, **extra)

    # the problems, the outputs and the first control handle: bench.DeviceProblem as bench.py makes it
    prob = bench.DeviceProblem(torch, hipldl, s, rows, cols, vals, rhs, args.batch, 0, stream, options=options(0))
    if not prob.L.config["band_mover_table"]:
        # (8 192 problems and fewer run 16 problems per workgroup by default: --opt band_problems_per_group=32 forces the instance)
        print(f"# batch {args.batch}: the handle does not run the mover-table instance, the key is ignored: nothing to compare  {prob.L.config}")
        prob.close()
        return 0
    masks = [int(x) for x in args.policies.split(",") if x] if args.policies else list(range(1, 32))
    arms = [("0", prob.L), ("0'", hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=args.batch, device=0, options=options(0)))]
    for m in masks:
        try:
            L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=args.batch, device=0, options=options(m))
        except hipldl.CnlError as e:
            if args.policies:
                raise
            print(f"# policy {m}: skipped ({e})", flush=True)
            continue
        arms.append((str(m), L))
    for name, L in arms:
        want = 0 if name in ("0", "0'") else int(name)
        assert L.config["band_mover_table"] and L.config["band_cache_policy"] == want, (name, L.config)

    def burst(L, steps, warmup=0):
        prob.L = L
        return prob.timed(steps, warmup)

    # (the first launches write the rho slots of the problems that climb the ladder; from then on every launch starts from the same `vals`)
    burst(arms[0][1], 3, 2)
    ref = None
    for name, L in arms:   # warm-up, and every arm leaves what the first left
        burst(L, 3, 2)
        got = (prob.counts(), prob.d.clone(), prob.rho.clone(), prob.nfact.clone())
        if ref is None:
            ref = got
        assert got[0] == ref[0] and all(torch.equal(x, y) for x, y in zip(got[1:], ref[1:])), f"policy {name} differs from policy 0"
    print(f"# batch {args.batch}: {len(arms)} handles, success {ref[0]}, outputs of every arm bit-equal to policy 0", flush=True)
    ms = {name: [] for name, _ in arms}
    for r in range(args.rounds):
        k = r % len(arms)
        for name, L in arms[k:] + arms[:k]:
            ms[name].append(burst(L, args.burst))
        print(f"round {r + 1:2d}  " + "  ".join(f"{name} {ms[name][-1]:.4f}" for name, _ in arms), flush=True)
    prob.L = arms[0][1]
    for name, L in arms[1:]:
        L.close()
    base = ms["0"]
    out = {"batch": args.batch, "rounds": args.rounds, "burst": args.burst, "arms": {}}
    print(f"{'policy':>6s} {'median ms':>10s} {'min':>8s} {'max':>8s}   per round against policy 0: median / min / max %   rounds won")
    for name, _ in arms:
        v = ms[name]
        rel = [100 * (x / b - 1) for x, b in zip(v, base)]
        won = sum(x < b for x, b in zip(v, base))
        out["arms"][name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rel_median_pct": statistics.median(rel),
                             "rel_min_pct": min(rel), "rel_max_pct": max(rel), "rounds_won": won}
        print(f"{name:>6s} {statistics.median(v):10.4f} {min(v):8.4f} {max(v):8.4f}   {statistics.median(rel):+7.2f} / {min(rel):+6.2f} / {max(rel):+6.2f}"
              f"   {won:2d} of {len(v)}" + ("   (the control's own difference)" if name == "0'" else ""))
    print(json.dumps(out), flush=True)
    prob.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
