"""The Float32 instantiation of the general multifrontal kernel against its Float64 twin: cnl_last_kernel_ms of the
device-resident newton_system! (cnl_newton_system_f32_dev / cnl_newton_system_dev), median of 10 calls after warm-up, for
  * a Float32 handle with tuning float32_general = 1,
  * a Float64 handle forced onto the general kernel without condensation (the same plan), and
  * the default Float64 handle (what the register-front kernel and its condensation give for the same batch),
on random_structure(60, 80, 4, 0.1, seed=3) and band_structure(1000, 10, hw=3).  One process, one device.
usage: time_f32_general.py [B]   (default 4096); prints one JSON line per (pattern, handle) and a table."""
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
GENERAL64 = dict(plan_kind=1, condense=0, register_front=0, general_dense=0, dense_backend=0, band_kernel=0)
dev = torch.device("cuda", 0)
table = []
for pname, s, gen, seed0 in (("random(60,80,4,0.1)", syn.random_structure(60, 80, 4, 0.1, seed=3), syn.random_values, 100),
                             ("band(1000,10,hw=3)", syn.band_structure(1000, 10, hw=3), syn.band_values, 4000)):
    rows, cols = s.kkt_pattern()
    base = [gen(s, seed0 + k) for k in range(64)]
    vh, rh = np.stack([v for v, _ in base]), np.stack([r for _, r in base])
    rep = (B + 63) // 64
    for hname, T, opt in (("float32 general", np.float32, dict(float32_general=1)), ("float64 general", np.float64, GENERAL64),
                          ("float64 default", np.float64, {})):
        tt = torch.float32 if T == np.float32 else torch.float64
        vals = torch.from_numpy(np.ascontiguousarray(np.tile(vh, (rep, 1))[:B], T)).to(dev)
        rhs = torch.from_numpy(np.ascontiguousarray(np.tile(rh, (rep, 1))[:B], T)).to(dev)
        L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=T, options=hipldl.Options(**opt) if opt else None)
        L.set_timing(True)
        d = torch.zeros((B, s.N), dtype=tt, device=dev)
        ro, rho = torch.zeros(B, dtype=tt, device=dev), torch.zeros(B, dtype=tt, device=dev)
        nf, su = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        par = hipldl.default_params(T)
        ms = []
        for k in range(WARMUP + STEPS):
            hipldl.newton_system_dev(L, vals, rhs, d, ro, rho, nf, su, par, 0)
            torch.cuda.synchronize()
            if k >= WARMUP:
                ms.append(L.last_kernel_ms())
        med = float(np.median(ms))
        c = L.config
        row = {"pattern": pname, "B": B, "handle": hname, "kernel": "band" if c["band"] else c["kernel"], "tpp": c["tpp"], "ppb": c["ppb"],
               "lds_work": c["lds_work"], "lds_bytes": c["lds_bytes"], "ms": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
               "systems_per_s": B / (med * 1e-3), "success": int(su.sum().item()), "nfact_max": int(nf.max().item())}
        print(json.dumps(row), flush=True)
        table.append(row)
        L.close()
        del vals, rhs, d
        torch.cuda.empty_cache()
print()
print("| pattern | handle | kernel | tpp x ppb, work area | ms | systems/s |")
print("|---|---|---|---|---|---|")
for r in table:
    print(f"| {r['pattern']} x {r['B']} | {r['handle']} | {r['kernel']} | {r['tpp']} x {r['ppb']}, {'LDS' if r['lds_work'] else 'global'} | "
          f"{r['ms']:.3f} | {r['systems_per_s'] / 1e6:.3f} M |")
