"""Float32 against Float64 for the device-resident passes around the Newton system on the headline pattern (band_structure(10000, 50)):
row f2 (prepare, problem-major and interleaved `vals`), row f1 (`_jac`: the model's Jacobian arrays), the trial point, row f4 (CGLS,
latency-bound), and the whole step prepare (interleaved) + newton_system! + trial point + f1 (`_jac`).  Device events around each call
after warm-up, median of 10; GB/s on the bytes each row has to move and the fraction of 8 TB/s.
usage: time_f32_rows.py [B ...]   (default 4096 16384); one JSON line per (B, type, row) and a table."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cannoles_jl_amd  # noqa: F401,E402
from cannoles_jl_amd import hipldl, synthetic as syn  # noqa: E402
import bench  # noqa: E402

WARMUP, STEPS, HBM = 3, 10, 8e12
s = syn.band_structure(10000, 50)
rows, cols = s.kkt_pattern()
off = s.offsets()
dev = torch.device("cuda", 0)
n, m, p, N, nnz = s.nvar, s.nequ, s.ncon, s.N, s.nnzNS
ELEMS = {   # elements each row reads and writes per problem
    "f2_problem_major": s.nnzhF + s.nnzhc + s.nnzjF + s.nnzjc + 1 + (nnz - m),
    "f2_interleaved": s.nnzhF + s.nnzhc + s.nnzjF + s.nnzjc + 1 + (nnz - m),
    "f1_jac": s.nnzjF + s.nnzjc + 2 * m + 2 * p + N + 2,
    "trial_point": (n + m + p + N) + (n + m + 2 * p),
    "cgls_jac": 0,
    "step": 0,
}


def timed(fn, stream):
    ms = []
    with torch.cuda.stream(stream):
        for k in range(WARMUP + STEPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn(stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            if k >= WARMUP:
                ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


table = []
for B in [int(a) for a in sys.argv[1:]] or [4096, 16384]:
    vh, rh = bench.band_batch(s, min(B, 256), 3000)
    rep = (B + len(vh) - 1) // len(vh)
    for T, tname in ((np.float64, "float64"), (np.float32, "float32")):
        tt = torch.float64 if T == np.float64 else torch.float32
        esz = np.dtype(T).itemsize
        vals = torch.from_numpy(np.ascontiguousarray(vh, T)).to(dev).repeat(rep, 1)[:B].contiguous()
        rhs = torch.from_numpy(np.ascontiguousarray(rh, T)).to(dev).repeat(rep, 1)[:B].contiguous()
        seg = lambda a, b: vals[:, off[a]:off[b]].contiguous()   # noqa: E731
        hF, hc, Jx, Jc = seg(0, 1), -seg(1, 2), seg(2, 3), seg(3, 4)
        delta = -vals[:, off[5]].contiguous()
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        mk = lambda k: torch.randn((B, k), dtype=tt, device=dev, generator=g)   # noqa: E731
        x, r, lam, Fx, cx = mk(n), mk(m), mk(p), mk(m), mk(p)
        par = hipldl.default_params(T)
        st = torch.cuda.Stream()
        Ls = {lay: hipldl.HIPLDLStruct(s.N, rows, cols, None, n, m, p, batch=B, dtype=T,
                                       options=hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT, batch_layout=lay)) for lay in (0, 1)}
        vpm = vals.clone()   # (the -I segment, which prepare leaves alone, holds -1)
        vil = torch.zeros(hipldl.layout_len(Ls[1], 0), dtype=tt, device=dev)
        hipldl.interleave_dev(Ls[1], 0, vals, vil)
        d = torch.zeros((B, N), dtype=tt, device=dev)
        d.copy_(rhs * 1e-3)
        out_rhs, nrm = torch.zeros((B, N), dtype=tt, device=dev), torch.zeros((B, 2), dtype=tt, device=dev)
        xt, rt, lt, dl = torch.zeros_like(x), torch.zeros_like(r), torch.zeros_like(lam), torch.zeros_like(lam)
        ro, rho = torch.zeros(B, dtype=tt, device=dev), torch.zeros(B, dtype=tt, device=dev)
        nf, su = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        lam_ls, it = torch.zeros_like(lam), torch.zeros(B, dtype=torch.int32, device=dev)
        L0, L1 = Ls[0], Ls[1]

        def step(sp):
            hipldl.prepare_newton_system_dev(L1, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, hF, hc, Jx, Jc, delta, vil, sp)
            hipldl.newton_system_dev(L1, vil, rhs, d, ro, rho, nf, su, par, sp)
            hipldl.trial_point_dev(L1, x, r, lam, d, 1e4, xt, rt, lt, dl, sp)
            hipldl.residual_vectors_jac_dev(L1, s.nnzjF, s.nnzjc, Jx, Jc, rt, lt, Fx, cx, out_rhs, nrm, sp)

        rows_fn = {
            "f2_problem_major": lambda sp: hipldl.prepare_newton_system_dev(L0, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, hF, hc, Jx, Jc, delta, vpm, sp),
            "f2_interleaved": lambda sp: hipldl.prepare_newton_system_dev(L1, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, hF, hc, Jx, Jc, delta, vil, sp),
            "f1_jac": lambda sp: hipldl.residual_vectors_jac_dev(L0, s.nnzjF, s.nnzjc, Jx, Jc, r, lam, Fx, cx, out_rhs, nrm, sp),
            "trial_point": lambda sp: hipldl.trial_point_dev(L0, x, r, lam, d, 1e4, xt, rt, lt, dl, sp),
            "cgls_jac": lambda sp: hipldl.cgls_multipliers_jac_dev(L0, s.nnzjF, s.nnzjc, Jx, Jc, r, lam_ls, iters_ptr=it, stream=sp),
            "step": step,
        }
        for name, fn in rows_fn.items():
            med, lo, hi = timed(fn, st)
            by = ELEMS[name] * esz
            row = {"B": B, "dtype": tname, "row": name, "ms": med, "ms_min": lo, "ms_max": hi, "bytes_per_system": by}
            if by:
                row["GBps"] = by * B / (med * 1e-3) / 1e9
                row["frac_8TBps"] = by * B / (med * 1e-3) / HBM
            if name == "step":
                row["success"] = int(su.sum().item())
            if name == "cgls_jac":
                row["iters_max"] = int(it.max().item())
            print(json.dumps(row), flush=True)
            table.append(row)
        for L in Ls.values():
            L.close()
        del vals, rhs, hF, hc, Jx, Jc, delta, x, r, lam, Fx, cx, vpm, vil, d, out_rhs, nrm, xt, rt, lt, dl
        torch.cuda.empty_cache()
print()
print("| B | row | Float64 ms | Float32 ms | Float32 / Float64 | Float64 frac of 8 TB/s | Float32 frac of 8 TB/s |")
print("|---|---|---|---|---|---|---|")
by_key = {(t["B"], t["row"], t["dtype"]): t for t in table}
for (B, name, dt), t64 in by_key.items():
    if dt != "float64":
        continue
    t32 = by_key[(B, name, "float32")]
    f = lambda t: f"{t['frac_8TBps']:.2f}" if "frac_8TBps" in t else "-"   # noqa: E731
    print(f"| {B} | {name} | {t64['ms']:.3f} | {t32['ms']:.3f} | {t32['ms'] / t64['ms']:.2f} | {f(t64)} | {f(t32)} |")
