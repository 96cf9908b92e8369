"""Host-pointer cnl_newton_system (the literal drop-in call) at small batches: pageable against pinned caller arrays.
  --dtype float32|float64   element type of the handle and the arrays (default float64); float32 also times the two-call sequence
                            (try_to_factorize, solve_ldl!) at batch 1 and 512"""
import argparse, os, sys, time, json
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
torch.zeros(1, device="cuda")
import cannoles_jl_amd  # noqa
from cannoles_jl_amd import hipldl, synthetic as syn
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", choices=["float32", "float64"], default="float64")
args = ap.parse_args()
dtype = np.dtype(args.dtype)

def pinned_like(a):
    t = torch.empty(a.shape, dtype=getattr(torch, args.dtype), pin_memory=True)
    n = t.numpy(); n[...] = a
    return n, t

s = syn.band_structure(10000, 50); rows, cols = s.kkt_pattern()
prm = hipldl.default_params(dtype)
out = {}

def timed(fn, n):
    for _ in range(5):
        fn()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return 1e3 * (time.perf_counter() - t0) / n

for B in (1, 16, 512):
    vh, rh = (np.ascontiguousarray(a, dtype) for a in bench.band_batch(s, B, 3000))
    L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=dtype)
    for kind in ("pageable", "pinned"):
        if kind == "pinned":
            v, _kv = pinned_like(vh); r, _kr = pinned_like(rh); d, _kd = pinned_like(np.zeros((B, s.N), dtype))
        else:
            v, r, d = vh.copy(), rh.copy(), np.zeros((B, s.N), dtype)
        ro = np.zeros(B, dtype)
        n = 30 if B <= 16 else 8
        ms = timed(lambda: hipldl.newton_system_(d, s.nvar, s.nequ, s.ncon, r, v, L, ro, prm), n)
        out[f"B{B}_{kind}"] = {"ms_per_call": ms, "systems_per_s": B / ms * 1e3}
        print(B, kind, "%.3f ms/call" % ms, "%.0f systems/s" % (B / ms * 1e3), flush=True)
    if dtype == np.float32 and B != 16:
        # the two-call sequence on pageable arrays (the copy sequence of these two calls is the handle's pinned block)
        v, r, d = vh.copy(), rh.copy(), np.zeros((B, s.N), dtype)
        # (solve first: behind the newton_system calls above every problem holds a factor, whatever rho it took)
        ms_s = timed(lambda: hipldl.solve_ldl_(r, L.factor, d), n)
        ms_f = timed(lambda: hipldl.try_to_factorize(L, v, s.nvar, s.nequ, s.ncon, prm[0], return_inertia=True), n)
        out[f"B{B}_factorize"] = {"ms_per_call": ms_f}
        out[f"B{B}_solve"] = {"ms_per_call": ms_s}
        print(B, "factorize %.3f ms/call, solve %.3f ms/call" % (ms_f, ms_s), flush=True)
    L.close()
os.makedirs("gpurun_out", exist_ok=True)
json.dump(out, open("gpurun_out/host_call_timing.json", "w"), indent=1)
