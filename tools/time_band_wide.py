"""The wide band kernels on the pattern a constrained model produces (synthetic.model_band_structure(10000, 50): H_c as wide as H_F),
device-resident newton_system!, per-call device events around the `_dev` call after warm-up.

  one library:   time_band_wide.py run [--pieces 0|15|20] [--dtype float64|float32] [--layout 0|1] [--nl N] B [B ...]
                 one JSON line per batch size: median / min / max of STEPS calls, the kernel that ran, GB/s on the kernel's own bytes
                 (bench.band_kernel_bytes' formula on the wide program's records: every COO value — both copies of the Hessian
                 positions included — and right-hand-side entry once, the records written and read once, the Jacobian / -I entries
                 of the condensed rows again in the backward sweep, d once)
  two libraries: time_band_wide.py ab <other libcannoles_hip.so> [--rounds R] B [B ...]
                 alternates fresh processes on this tree's library and on the other one (a build of the parent commit:
                 tools/ab_lib.py build parent <ref>) with default options — the other library runs what it runs on this pattern
                 (before the wide form: the register-front kernel) — and prints both medians per batch size and round.
Float64 handles take the wide kernel automatically only where this comparison showed it faster (csrc/capi_handle.cpp, band_wide_serves_f64)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS = 3, 10


def model_batch(syn, bench, s, B, seed):
    """bench.band_batch on the band_structure twin, moved into the model-shaped layout (small off-diagonal H_c entries)"""
    twin = syn.band_structure(s.nvar, s.ncon, hw=s.meta["hw"])
    v0, rhs = bench.band_batch(twin, B, seed)
    o0, o1 = twin.offsets(), s.offsets()
    vals = np.zeros((B, s.nnzNS))
    vals[:, o1[0]:o1[1]] = v0[:, o0[0]:o0[1]]
    r, c = np.asarray(s.hc[0]), np.asarray(s.hc[1])
    hcv = np.random.default_rng(seed + 1).uniform(-0.01, 0.01, (B, len(r)))
    hcv[:, r == c] = v0[:, o0[1]:o0[2]]
    vals[:, o1[1]:o1[2]] = hcv
    vals[:, o1[2]:] = v0[:, o0[2]:]
    return vals, rhs


def kernel_bytes(L, s, esz):
    prefix = "bandw" if L.config["band_pieces"] == 20 else "band"
    info = L.plan_array(prefix + "_info")
    lsz = sum(int(L.plan_array(f"{prefix}_part{q}")[3]) * 6 for q in range(int(info[1])))
    fwd = s.nnzNS + s.N + lsz
    bwd = lsz + len(s.jF[0]) + 2 * s.nequ + s.N
    return esz * (fwd + bwd)


def run(args):
    import torch
    sys.path.insert(0, ROOT)
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    import bench
    s = syn.model_band_structure(10000, 50) if hasattr(syn, "model_band_structure") else None
    if s is None:   # a library AND tree of the parent commit: the pattern from the structure's parts
        b = syn.band_structure(10000, 50)
        s = syn.Structure(b.nvar, b.nequ, b.ncon, b.hF, b.hF, b.jF, b.jc, name="band-model", meta=dict(b.meta, hw=2))
    rows, cols = s.kkt_pattern()
    dev = torch.device("cuda", 0)
    T = np.float64 if args.dtype == "float64" else np.float32
    tt = torch.float64 if T == np.float64 else torch.float32
    vh, rh = model_batch(syn, bench, s, 256, 3000)
    for B in args.B:
        rep = (B + 255) // 256
        vals = torch.from_numpy(np.ascontiguousarray(np.tile(vh, (rep, 1))[:B], T)).to(dev)
        rhs = torch.from_numpy(np.ascontiguousarray(np.tile(rh, (rep, 1))[:B], T)).to(dev)
        kw = dict(batch_layout=args.layout)
        if args.pieces:
            kw["band_pieces"] = args.pieces
        if args.nl:
            kw["band_problems_per_group"] = args.nl
        kw = {k: v for k, v in kw.items() if v}
        L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=T, options=hipldl.Options(**kw) if kw else None)
        vin = vals
        if args.layout:
            vin = torch.zeros(hipldl.layout_len(L, 0), dtype=tt, device=dev)
            hipldl.interleave_dev(L, 0, vals, vin)
        d = torch.zeros((B, s.N), dtype=tt, device=dev)
        ro, rho = torch.zeros(B, dtype=tt, device=dev), torch.zeros(B, dtype=tt, device=dev)
        nf, su = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        par = hipldl.default_params(T)
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
        med = float(np.median(ms))
        band = bool(L.config["band"])
        row = {"lib": os.path.relpath(hipldl.LIB_PATH, ROOT), "B": B, "dtype": args.dtype, "layout": "interleaved" if args.layout else "problem-major",
               "kernel": "band" if band else L.config["kernel"], "band_pieces": L.config.get("band_pieces", 15 if band else 0),
               "band_nl": L.config["band_nl"], "ms_per_step": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
               "systems_per_s": B / (med * 1e-3), "success": int(su.sum().item())}
        if band:
            kb = kernel_bytes(L, s, np.dtype(T).itemsize)
            row.update(kernel_bytes_per_system=kb, GBps_on_kernel_bytes=kb * B / (med * 1e-3) / 1e9)
        print(json.dumps(row), flush=True)
        L.close()
        del vals, rhs, vin, d


def ab(args):
    """fresh child processes, this tree's library and the other one alternately; every child under a time limit of its own, and the
    first child that fails ends the comparison"""
    rows = []
    for B in args.B:
        for rnd in range(args.rounds):
            for name, lib in (("this", None), ("other", os.path.abspath(args.other))):
                env = dict(os.environ)
                if lib:
                    env["CANNOLES_HIP_LIB"] = lib
                else:
                    env.pop("CANNOLES_HIP_LIB", None)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "run", str(B)], env=env, capture_output=True, text=True, timeout=240)
                if out.returncode != 0:
                    sys.exit(f"child ({name}, B = {B}) ended with {out.returncode}:\n{out.stderr[-2000:]}")
                r = json.loads(out.stdout.strip().splitlines()[-1])
                r.update(which=name, round=rnd)
                print(json.dumps(r), flush=True)
                rows.append(r)
    print(f"{'B':>6} {'library':>7} {'kernel':>6} {'nl':>3} {'median of medians ms':>21} {'min':>8} {'max':>8}   (medians of {STEPS} calls, {args.rounds} alternated rounds)")
    for B in args.B:
        for name in ("other", "this"):
            m = [r["ms_per_step"] for r in rows if r["B"] == B and r["which"] == name]
            r0 = next(r for r in rows if r["B"] == B and r["which"] == name)
            print(f"{B:6d} {name:>7} {r0['kernel']:>6} {r0['band_nl']:3d} {np.median(m):21.3f} {min(m):8.3f} {max(m):8.3f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("run")
    a.add_argument("--pieces", type=int, default=0)
    a.add_argument("--dtype", default="float64")
    a.add_argument("--layout", type=int, default=0)
    a.add_argument("--nl", type=int, default=0)
    a.add_argument("B", type=int, nargs="+")
    b = sub.add_parser("ab")
    b.add_argument("other")
    b.add_argument("--rounds", type=int, default=3)
    b.add_argument("B", type=int, nargs="+")
    args = ap.parse_args()
    run(args) if args.cmd == "run" else ab(args)
