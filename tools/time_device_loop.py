"""Times the device-resident lockstep outer loop (row f3) against the single-problem host loop with the CPU oracle.
  --dtype float32|float64   element type of the family and the run (default float64)
  --shape n,p,B             one workload instead of the built-in list (repeatable)
  --out PATH                where the JSON list of records goes instead of the default file
  --profile                 wall time per section of a global step
  --compact                 run every global step on the active problems only (solve_batch_device(compact=True)); the record then also
                            holds compactions, problem_steps and its share of steps * B, handle_shrunk
  --min-finished K          compact_min_finished (default: the loop's own, max(32, working batch // 8))
  --no-host-loop            skip the single-problem host loop with the CPU oracle
  --method NAME             Newton (default), Newton_noFHess or Newton_vanishing (the latter adds cnl_outer_hess_mask_dev to every step)"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
torch.zeros(1, device="cuda")
import cannoles_jl_amd  # noqa
from cannoles_jl_amd import device_loop as DL, synthetic as syn, outer_loop, hipldl

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["float32", "float64"], default="float64")
    ap.add_argument("--shape", action="append", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--compact", action="store_true")
    ap.add_argument("--min-finished", type=int, default=None)
    ap.add_argument("--no-host-loop", action="store_true")
    ap.add_argument("--method", default="Newton")
    args = ap.parse_args()
    dtype = np.dtype(args.dtype)
    shapes = [tuple(int(v) for v in sh.split(",")) for sh in args.shape] if args.shape else \
        [(300, 4, 256), (300, 4, 2048), (300, 4, 8192), (2000, 10, 1024), (1000, 10, 16384)]
    out = []
    kw = dict(compact=True, compact_min_finished=args.min_finished) if args.compact else {}
    if args.method != "Newton":
        kw["method"] = args.method
    for (n, p, B) in shapes:
        s = syn.band_structure(n, p)
        fam = DL.BandQuadFamily(s, B, seed=7, torch=torch, device="cuda:0", curvature=1.5, start=1.0, noise=0.5, dtype=dtype)
        prm = hipldl.default_params(dtype)
        DL.solve_batch_device(fam, prm, **kw)
        if args.profile:
            DL.PROFILE = True
            print("profile", (n, p, B), json.dumps(DL.solve_batch_device(fam, prm, **kw)["profile_ms_per_step"]), flush=True)
            DL.PROFILE = False
        t0 = time.perf_counter()
        got = DL.solve_batch_device(fam, prm, **kw)
        dt = time.perf_counter() - t0
        rec = {"n": n, "p": p, "B": B, "dtype": got["dtype"], "seconds": dt, "problems_per_s": B / dt, "steps": got["steps"], "ms_per_step": 1e3 * got["loop_seconds"] / got["steps"], "setup_seconds": dt - got["loop_seconds"],
               "newton_systems": int(got["nlinsolve"].sum()), "factorisations": int(got["nfact"].sum()),
               "first_order": sum(st == "first_order" for st in got["status"]), "kernel": got["kernel"], "vals_layout": got.get("vals_layout"), "method": args.method}
        if args.compact:
            rec.update(compact=True, compact_min_finished=args.min_finished, compactions=got["compactions"], problem_steps=got["problem_steps"],
                       problem_step_share=got["problem_steps"] / (got["steps"] * B), handle_shrunk=got["handle_shrunk"])
        if os.path.isdir("oracle") and not args.no_host_loop:
            from tests.test_oracle_pinning import oracle_newton, oracle_solver
            t0 = time.perf_counter()
            k = min(B, 64)
            for b in range(k):
                outer_loop.solve(fam.host_model(b), oracle_solver, oracle_newton, hipldl.default_params())   # (the host loop is Float64)
            rec["host_loop_cpu_oracle_problems_per_s_1core"] = k / (time.perf_counter() - t0)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)
        return
    os.makedirs("gpurun_out", exist_ok=True)
    json.dump(out, open("gpurun_out/device_loop_timing.json", "w"), indent=1)

main()
