"""Float32 general handles on the register-front kernel (tuning float32_register_front, DESIGN sections 9.3 and 9.4): the time of
the WHOLE device-resident newton_system! call (cnl_newton_system_f32_dev / cnl_newton_system_dev) and of the whole solve_ldl! call
(cnl_solve_f32_dev / cnl_solve_dev, behind that factorisation), taken with device events on the stream — cnl_last_kernel_ms
brackets the multifrontal kernel only and misses the condensation passes — for
  * a Float32 handle with float32_general = 1, float32_register_front = 1 and float32_direct_records = 1 (direct records),
  * a Float32 handle with tuning float32_general = 1 and float32_register_front = 1 (the passes around the launch),
  * a Float32 handle with float32_general = 1 and float32_condense = 1 (the general kernel on the condensed system), and
  * the default Float64 handle,
on random_structure(60, 80, 4, 0.1, seed=3), band_structure(1000, 10, hw=3) and dense_structure(40, 70).
Every problem factorises at the first attempt.  The four handles of a pattern take turns call by call (the same process, the same
device); median of 10 calls after 3 warm-up calls each, with min .. max.  A second pass with cnl_set_timing on gives the multifrontal
kernel's own time.
usage: time_f32_register_front.py [B]   (default 4096); prints one JSON line per (pattern, handle) and a table."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cannoles_jl_amd  # noqa: F401,E402
from cannoles_jl_amd import hipldl, synthetic as syn  # noqa: E402

WARMUP, STEPS = 3, 10
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
HANDLES = (("float32 direct", np.float32, dict(float32_general=1, float32_register_front=1, float32_direct_records=1)),
           ("float32 register-front", np.float32, dict(float32_general=1, float32_register_front=1)),
           ("float32 condensed", np.float32, dict(float32_general=1, float32_condense=1)),
           ("float64 default", np.float64, dict()))
PATTERNS = (("random(60,80,4,0.1)", syn.random_structure(60, 80, 4, 0.1, seed=3), syn.random_values, 100),
            ("band(1000,10,hw=3)", syn.band_structure(1000, 10, hw=3), syn.band_values, 4000),
            ("dense(40,70)", syn.dense_structure(40, 70), syn.dense_values, 100))
dev = torch.device("cuda", 0)
table = []
for pname, s, gen, seed0 in PATTERNS:
    rows, cols = s.kkt_pattern()
    base = [gen(s, seed0 + k) for k in range(16)]
    vh, rh = np.stack([v for v, _ in base]), np.stack([r for _, r in base])
    rep = (B + 15) // 16
    runs = []
    for hname, T, opt in HANDLES:
        tt = torch.float32 if T == np.float32 else torch.float64
        r = {"name": hname, "T": T,
             "vals": torch.from_numpy(np.ascontiguousarray(np.tile(vh, (rep, 1))[:B], T)).to(dev),
             "rhs": torch.from_numpy(np.ascontiguousarray(np.tile(rh, (rep, 1))[:B], T)).to(dev),
             "L": hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=T, options=hipldl.Options(**opt)),
             "d": torch.zeros((B, s.N), dtype=tt, device=dev), "ro": torch.zeros(B, dtype=tt, device=dev), "rho": torch.zeros(B, dtype=tt, device=dev),
             "nf": torch.zeros(B, dtype=torch.int32, device=dev), "su": torch.zeros(B, dtype=torch.int32, device=dev),
             "par": hipldl.default_params(T), "call": [], "kernel": [], "solve": []}
        runs.append(r)
    for timing in (False, True):
        for r in runs:
            r["L"].set_timing(timing)
        for k in range(WARMUP + STEPS):
            for r in runs:   # the handles take turns
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hipldl.newton_system_dev(r["L"], r["vals"], r["rhs"], r["d"], r["ro"], r["rho"], r["nf"], r["su"], r["par"], 0)
                e1.record()
                torch.cuda.synchronize()
                if k >= WARMUP:
                    (r["kernel"] if timing else r["call"]).append(r["L"].last_kernel_ms() if timing else e0.elapsed_time(e1))
                if not timing:   # solve_ldl! with the factor the call left (the caller's vals alive and unmodified)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    hipldl.solve_dev(r["L"], r["rhs"], r["d"], 0)
                    e1.record()
                    torch.cuda.synchronize()
                    if k >= WARMUP:
                        r["solve"].append(e0.elapsed_time(e1))
    for r in runs:
        c, info = r["L"].config, r["L"].info
        med, kmed, smed = float(np.median(r["call"])), float(np.median(r["kernel"])), float(np.median(r["solve"]))
        row = {"pattern": pname, "B": B, "handle": r["name"], "kernel": c["kernel"], "ncond": info["ncond"], "fmax": info["fmax"], "wpb": c["wpb"],
               "lds2_bytes": c["lds2_bytes"], "cond_resident": c["cond_resident"], "direct": c["direct"], "v2_solve": c["v2_solve"], "call_ms": med, "call_ms_min": float(min(r["call"])),
               "call_ms_max": float(max(r["call"])), "kernel_ms": kmed, "solve_ms": smed, "solve_ms_min": float(min(r["solve"])),
               "solve_ms_max": float(max(r["solve"])), "systems_per_s": B / (med * 1e-3),
               "success": int(r["su"].sum().item()), "nfact_max": int(r["nf"].max().item())}
        assert row["success"] == B and row["nfact_max"] == 1, row
        print(json.dumps(row), flush=True)
        table.append(row)
        r["L"].close()
    del runs
    torch.cuda.empty_cache()
print()
print("| pattern | handle | kernel | direct | largest front | whole call ms (min .. max) | multifrontal kernel ms | solve_ldl! ms (min .. max) | systems/s |")
print("|---|---|---|---|---|---|---|---|---|")
for r in table:
    print(f"| {r['pattern']} x {r['B']} | {r['handle']} | {r['kernel']} | {'yes' if r['direct'] else 'no'} | {r['fmax']} | "
          f"{r['call_ms']:.3f} ({r['call_ms_min']:.3f} .. {r['call_ms_max']:.3f}) | {r['kernel_ms']:.3f} | "
          f"{r['solve_ms']:.3f} ({r['solve_ms_min']:.3f} .. {r['solve_ms_max']:.3f}) | {r['systems_per_s'] / 1e6:.3f} M |")
