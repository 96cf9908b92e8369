"""Float32 against Float64 on the band kernels: device-resident newton_system! (cnl_newton_system_f32_dev / cnl_newton_system_dev) on the
headline pattern (band_structure(10000, 50)), both value layouts, per-call device events around the `_dev` call after warm-up.
usage: time_band_f32.py [B ...]   (default 256 8192 16384); prints one JSON line per (B, type, layout) and a table."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cannoles_jl_amd  # noqa: F401,E402
from cannoles_jl_amd import hipldl, synthetic as syn  # noqa: E402
import bench  # noqa: E402

WARMUP, STEPS = 3, 10
s = syn.band_structure(10000, 50)
rows, cols = s.kkt_pattern()
dev = torch.device("cuda", 0)
table = []
for B in [int(a) for a in sys.argv[1:]] or [256, 8192, 16384]:
    vh, rh = bench.band_batch(s, min(B, 256), 3000)
    rep = (B + len(vh) - 1) // len(vh)
    for T, tname in ((np.float64, "float64"), (np.float32, "float32")):
        tt = torch.float64 if T == np.float64 else torch.float32
        vals = torch.from_numpy(np.ascontiguousarray(np.tile(vh, (rep, 1))[:B], T)).to(dev)
        rhs = torch.from_numpy(np.ascontiguousarray(np.tile(rh, (rep, 1))[:B], T)).to(dev)
        par = hipldl.default_params(T)
        for layout in (0, 1):
            opt = hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT, batch_layout=layout)
            L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, options=opt, dtype=T)
            assert L.config["band"] and L.config["float32"] == (T == np.float32)
            vin = vals
            if layout:
                vin = torch.zeros(hipldl.layout_len(L, 0), dtype=tt, device=dev)
                hipldl.interleave_dev(L, 0, vals, vin)
            d = torch.zeros((B, s.N), dtype=tt, device=dev)
            ro, rho = torch.zeros(B, dtype=tt, device=dev), torch.zeros(B, dtype=tt, device=dev)
            nf, su = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            st = torch.cuda.Stream()
            ms = []
            with torch.cuda.stream(st):
                for k in range(WARMUP + STEPS):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    hipldl.newton_system_dev(L, vin, rhs, d, ro, rho, nf, su, par, st.cuda_stream)
                    e1.record(st)
                    e1.synchronize()
                    if k >= WARMUP:
                        ms.append(e0.elapsed_time(e1))
            ok = int(su.sum().item())
            kb = bench.band_kernel_bytes(L, s) * (np.dtype(T).itemsize / 8)   # the same program's streams, 4- or 8-byte elements
            med = float(np.median(ms))
            row = {"B": B, "dtype": tname, "layout": "interleaved" if layout else "problem-major", "band_nl": L.config["band_nl"],
                   "ms_per_step": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)), "systems_per_s": B / (med * 1e-3),
                   "kernel_bytes_per_system": kb, "GBps_on_kernel_bytes": kb * B / (med * 1e-3) / 1e9, "success": ok}
            print(json.dumps(row), flush=True)
            table.append(row)
            L.close()
            del vin, d, ro, rho, nf, su
        del vals, rhs
        torch.cuda.empty_cache()
print()
print(f"| B | type | layout | nl | ms/step | systems/s | GB/s on kernel bytes |")
print("|---|---|---|---|---|---|---|")
for r in table:
    print(f"| {r['B']} | {r['dtype']} | {r['layout']} | {r['band_nl']} | {r['ms_per_step']:.3f} | {r['systems_per_s'] / 1e6:.3f} M | {r['GBps_on_kernel_bytes']:.0f} |")
