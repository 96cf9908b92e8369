"""Refined handles (tuning float32_refine): the time of the WHOLE device-resident newton_system! call
(cnl_newton_system_dev / cnl_newton_system_f32_dev) and of the solve_ldl! call behind it, taken with device events on the stream, for
  * the refined handle, k = 1, 2, 3 (a Float64 handle on the inner Float32 handle the configuration's keys select),
  * the default Float64 handle, and
  * the bare inner Float32 handle (the same keys without float32_refine)
at the shapes of CONFIGS.  Every problem factorises at the first attempt.

One configuration = one child process (a fresh device context) under its own time limit; a child that fails or runs out of time ends
the run.  Inside a child every handle is created first, each makes one guarded call — all problems succeed; the refined handles meet
the derived backward bound of tests/support/f32_refine.py on problem 0, in longdouble —, then the handles take turns call by call:
median of ROUNDS calls after WARMUP warm-up calls each, with min .. max.  The child runs its turns twice and prints both medians
(the spread of repeated runs).  Run it from a checkout of the repository with the library built.

--rows: the two instances of the KKT residual kernel (tuning refine_rows = 1: a row per lane, 2: a row per wavefront) through
cnl_kkt_residual_dev on the two patterns the threshold KKT_WAVE_ROW_THRESHOLD (csrc/refine.h) was picked from, alternated.

usage: time_f32_refine.py [--out FILE]      all configurations and the --rows timing; the text goes to stdout and, with --out, to FILE
       time_f32_refine.py --one K            configuration K of CONFIGS (what the driver starts); one JSON line per handle
       time_f32_refine.py --rows             the residual kernel's instances alone"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (generator, its arguments, batch, the keys of the inner handle, time limit of the child in s)
CONFIGS = [("dense", (1000, 2000), 32, dict(float32_dense=1), 400),
           ("dense", (100, 160), 4096, dict(float32_dense=1), 300),
           ("random", (1000, 1500, 10, 0.01, 1), 256, dict(float32_general_dense=1), 400),
           ("random", (129, 150, 0, 0.06, 5), 4096, dict(float32_general_dense=1), 300),
           ("dense", (1000, 2000), 1, dict(float32_dense=1), 400),
           ("band", (1000, 10, 3), 4096, dict(float32_register_front=1), 300)]
ROWS_CASES = [("random", (60, 80, 4, 0.1, 1), 4096), ("dense", (100, 160), 4096)]
WARMUP, ROUNDS = 3, 15


def _setup():
    import torch
    torch.zeros(1, device="cuda")   # torch's HIP runtime first (tests/conftest.py)
    sys.path.insert(0, ROOT)
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    return torch, hipldl, syn


def _structure(syn, gen, args):
    if gen == "dense":
        return syn.dense_structure(*args), syn.dense_values
    if gen == "band":
        return syn.band_structure(args[0], args[1], hw=args[2]), syn.band_values
    return syn.random_structure(*args), syn.random_values


def _inputs(np, s, values, B):
    nbase = min(B, 8)
    base = [values(s, 40 + 5 * j) for j in range(nbase)]
    rep = (B + nbase - 1) // nbase
    return np.tile(np.stack([v for v, _ in base]), (rep, 1))[:B], np.tile(np.stack([r for _, r in base]), (rep, 1))[:B]


def one(k):
    import numpy as np
    torch, hipldl, syn = _setup()
    from tests.support import f32_refine as RF
    gen, args, B, keys, _ = CONFIGS[k]
    s, values = _structure(syn, gen, args)
    rows, cols = s.kkt_pattern()
    vh, rh = _inputs(np, s, values, B)
    dev = torch.device("cuda", 0)
    tag = {"pattern": f"{gen}{tuple(args)}", "B": B, "N": s.N, "nnz": s.nnzNS, "keys": keys}
    kinds = [(f"refined k={kk}", np.float64, dict(keys, float32_general=1, float32_refine=kk)) for kk in (1, 2, 3)]
    kinds += [("float64 default", np.float64, None), ("float32 inner", np.float32, dict(keys, float32_general=1, band_kernel=0))]
    runs = []
    for hname, T, opt in kinds:
        tt = torch.float32 if T == np.float32 else torch.float64
        L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=T, options=hipldl.Options(**opt) if opt else None)
        runs.append({"name": hname, "L": L, "T": T, "vals": torch.from_numpy(np.ascontiguousarray(vh, T)).to(dev),
                     "rhs": torch.from_numpy(np.ascontiguousarray(rh, T)).to(dev), "d": torch.zeros((B, s.N), dtype=tt, device=dev),
                     "ro": torch.zeros(B, dtype=tt, device=dev), "rho": torch.zeros(B, dtype=tt, device=dev),
                     "nf": torch.zeros(B, dtype=torch.int32, device=dev), "su": torch.zeros(B, dtype=torch.int32, device=dev),
                     "par": RF.demoted_params(hipldl)[1] if hname == "float32 inner" else hipldl.default_params(T)})   # (the parameters the refined handles hand their inner handle)
    # every handle exists before the first call of any: no creation (hipMalloc, hipMemset, uploads) falls between timed calls
    for r in runs:
        hipldl.newton_system_dev(r["L"], r["vals"], r["rhs"], r["d"], r["ro"], r["rho"], r["nf"], r["su"], r["par"], 0)
        torch.cuda.synchronize()
        assert int(r["su"].sum().item()) == B and int(r["nf"].max().item()) == 1, r["name"]
        r["guard"] = RF.omega(s, vh[0], rh[0], r["d"][0].cpu().numpy().astype(np.float64))
        if r["L"].config["refine"] >= 2:
            assert r["guard"] <= RF.bwd_bound(s), (r["name"], r["guard"], RF.bwd_bound(s))
    for rep in range(2):
        for r in runs:
            r["ms"], r["solve_ms"] = [], []
        for it in range(WARMUP + ROUNDS):
            for r in runs:   # the handles take turns
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record()
                hipldl.newton_system_dev(r["L"], r["vals"], r["rhs"], r["d"], r["ro"], r["rho"], r["nf"], r["su"], r["par"], 0)
                e1.record()
                hipldl.solve_dev(r["L"], r["rhs"], r["d"], 0)
                e2.record()
                torch.cuda.synchronize()
                if it >= WARMUP:
                    r["ms"].append(e0.elapsed_time(e1))
                    r["solve_ms"].append(e1.elapsed_time(e2))
        for r in runs:
            print(json.dumps(dict(tag, handle=r["name"], run=rep, kernel=r["L"].config["kernel"], call_ms=float(np.median(r["ms"])),
                                  call_ms_min=float(min(r["ms"])), call_ms_max=float(max(r["ms"])), solve_ms=float(np.median(r["solve_ms"])),
                                  solve_ms_min=float(min(r["solve_ms"])), solve_ms_max=float(max(r["solve_ms"])), omega=r["guard"],
                                  omega_bound=RF.bwd_bound(s))), flush=True)
    for r in runs:
        r["L"].close()


def rows_timing():
    import numpy as np
    torch, hipldl, syn = _setup()
    dev = torch.device("cuda", 0)
    for gen, args, B in ROWS_CASES:
        s, _ = _structure(syn, gen, args)
        rows, cols = s.kkt_pattern()
        rng = np.random.default_rng(1)
        tv, tr, td = (torch.from_numpy(rng.normal(size=(B, n))).to(dev) for n in (s.nnzNS, s.N, s.N))
        tg, tn = torch.zeros((B, s.N), dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)
        Ls = {m: hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, options=hipldl.Options(refine_rows=m)) for m in (1, 2)}
        ms = {1: [], 2: []}
        for it in range(WARMUP + ROUNDS):
            for m in (1, 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hipldl.kkt_residual_dev(Ls[m], tv, tr, td, tg, tn, 0)
                e1.record()
                torch.cuda.synchronize()
                if it >= WARMUP:
                    ms[m].append(e0.elapsed_time(e1))
        full = 2 * s.nnzNS - s.N   # (no diagonal is duplicated in these patterns)
        print(json.dumps({"rows_timing": f"{gen}{tuple(args)}", "B": B, "N": s.N, "mean_row": full / s.N,
                          "lane_ms": float(np.median(ms[1])), "lane_ms_min": min(ms[1]), "lane_ms_max": max(ms[1]),
                          "wavefront_ms": float(np.median(ms[2])), "wavefront_ms_min": min(ms[2]), "wavefront_ms_max": max(ms[2])}), flush=True)
        for L in Ls.values():
            L.close()


def _child(args, limit, what):
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"{what}: no result within {limit} s; stopping", flush=True)
        return None
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    if p.returncode != 0:
        print(p.stderr[-4000:])
        print(f"{what}: exit status {p.returncode}; stopping", flush=True)
        return None
    return [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]


def main(argv):
    if argv[:1] == ["--one"]:
        one(int(argv[1]))
        return 0
    if argv[:1] == ["--rows"]:
        rows_timing()
        return 0
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    rows = _child(["--rows"], 300, "rows timing")
    if rows is None:
        return 1
    for k, cfg in enumerate(CONFIGS):
        got = _child(["--one", str(k)], cfg[4], f"{cfg[0]}{cfg[1]} x {cfg[2]}")
        if got is None:
            return 1
        rows += got
    lines = ["| pattern x batch | handle | kernel | newton_system! ms: run 0 / run 1 median (min .. max of run 1) | solve_ldl! ms: run 0 / run 1 | omega(d) of problem 0 (bound) |",
             "|---|---|---|---|---|---|"]
    timed = [r for r in rows if "handle" in r]
    for r1 in (r for r in timed if r["run"] == 1):
        r0 = next(r for r in timed if r["run"] == 0 and (r["pattern"], r["B"], r["handle"]) == (r1["pattern"], r1["B"], r1["handle"]))
        lines.append(f"| {r1['pattern']} x {r1['B']} | {r1['handle']} | {r1['kernel']} | {r0['call_ms']:.3f} / {r1['call_ms']:.3f} ({r1['call_ms_min']:.3f} .. "
                     f"{r1['call_ms_max']:.3f}) | {r0['solve_ms']:.3f} / {r1['solve_ms']:.3f} | {r1['omega']:.2e} ({r1['omega_bound']:.2e}) |")
    lines += ["", "| residual kernel: pattern x batch | mean row | a row per lane, ms (min .. max) | a row per wavefront, ms (min .. max) |", "|---|---|---|---|"]
    for r in (r for r in rows if "rows_timing" in r):
        lines.append(f"| {r['rows_timing']} x {r['B']} | {r['mean_row']:.1f} | {r['lane_ms']:.3f} ({r['lane_ms_min']:.3f} .. {r['lane_ms_max']:.3f}) | "
                     f"{r['wavefront_ms']:.3f} ({r['wavefront_ms_min']:.3f} .. {r['wavefront_ms_max']:.3f}) |")
    text = "\n".join(lines) + "\n"
    print()
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
