"""Float32 handles on the dense backend (tuning float32_dense): the time of the WHOLE device-resident
newton_system! call (cnl_newton_system_f32_dev / cnl_newton_system_dev), taken with device events on the stream, for
  * the Float32 dense handle (float32_general = 1, float32_dense = 1: csrc/dense_f32.hip),
  * the Float32 float32_condense handle ("v1": the general kernel in float on the condensed system) — where its creation fails, the
    error text is recorded instead —, and
  * the default Float64 handle (the dense backend in double)
on dense_structure(1000, 2000) at B = 1, 8, 32 (BASELINE config 2) and dense_structure(100, 160), dense_structure(40, 70) at
B = 4096.  Every problem factorises at the first attempt.

One configuration = one child process (a fresh device context) under its own time limit; a child that fails or runs out of time ends
the run.  Inside a child the handles are created once, each passes a parity guard on problem 0 against the CPU oracle (Float32: the
oracle on the widened float32 inputs with ParamCaNNOLeS(Float32), backward error <= 512 eps32, forward error <= 1e-3; Float64:
forward error <= 1e-9), then they take turns call by call: median of ROUNDS calls after WARMUP warm-up calls each, with min .. max.

usage: time_dense_f32.py [--out FILE]          all configurations; the table goes to stdout and, with --out, to FILE
       time_dense_f32.py --one N M B            one configuration (what the driver starts); one JSON line per handle"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(1000, 2000, 1, 420), (1000, 2000, 8, 420), (1000, 2000, 32, 480), (100, 160, 4096, 300), (40, 70, 4096, 240)]   # n, m, B, time limit (s)
WARMUP, ROUNDS = 3, 10
SLOW_CALL_S = 4.0   # a handle whose first call takes longer is reported with that one call and takes no turns


def one(n, m, B):
    import numpy as np
    import torch
    torch.zeros(1, device="cuda")   # torch's HIP runtime first (tests/conftest.py)
    sys.path.insert(0, ROOT)
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    from oracle import oracle as O
    from tests.support import f32_general as G

    s = syn.dense_structure(n, m)
    rows, cols = s.kkt_pattern()
    nbase = min(B, 16)
    base = [syn.dense_values(s, 100 + k) for k in range(nbase)]
    vh, rh = np.stack([v for v, _ in base]), np.stack([r for _, r in base])
    rep = (B + nbase - 1) // nbase
    dev = torch.device("cuda", 0)
    orc = O.Oracle(s.N, rows, cols, O.canonical_perm(s.nvar, s.nequ, s.ncon))
    handles = (("float32 dense", np.float32, dict(float32_general=1, float32_dense=1), "dense"),
               ("float32 condensed", np.float32, dict(float32_general=1, float32_condense=1), "v1"),
               ("float64 dense", np.float64, dict(), "dense"))
    runs = []
    for hname, T, opt, kernel in handles:
        tt = torch.float32 if T == np.float32 else torch.float64
        try:
            L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=T, options=hipldl.Options(**opt))
        except hipldl.CnlError as e:
            print(json.dumps({"n": n, "m": m, "B": B, "handle": hname, "error": str(e)}), flush=True)
            continue
        assert L.config["kernel"] == kernel and L.config["float32"] == (T == np.float32), L.config
        vals = np.ascontiguousarray(np.tile(vh, (rep, 1))[:B], T)
        rhs = np.ascontiguousarray(np.tile(rh, (rep, 1))[:B], T)
        r = {"name": hname, "L": L, "vals": torch.from_numpy(vals).to(dev), "rhs": torch.from_numpy(rhs).to(dev),
             "d": torch.zeros((B, s.N), dtype=tt, device=dev), "ro": torch.zeros(B, dtype=tt, device=dev), "rho": torch.zeros(B, dtype=tt, device=dev),
             "nf": torch.zeros(B, dtype=torch.int32, device=dev), "su": torch.zeros(B, dtype=torch.int32, device=dev),
             "par": hipldl.default_params(T), "ms": []}
        # parity guard on problem 0 (the call is also timed on the host: see SLOW_CALL_S)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hipldl.newton_system_dev(L, r["vals"], r["rhs"], r["d"], r["ro"], r["rho"], r["nf"], r["su"], r["par"], 0)
        torch.cuda.synchronize()
        r["first_call_s"] = time.perf_counter() - t0
        d0, ok0, _, _, nf0 = O.newton_system(orc, s.nvar, s.nequ, s.ncon, rhs[0].astype(np.float64), vals[0].astype(np.float64), 0.0,
                                             np.asarray(r["par"], np.float64))
        dg = r["d"][0].cpu().numpy().astype(np.float64)
        fe = float(np.abs(dg - d0).max() / np.abs(d0).max())
        be = float(G.backward_error(s, vals[0], rhs[0], dg))
        assert ok0 and nf0 == 1 and int(r["su"][0].item()) == 1 and int(r["nf"][0].item()) == 1, (hname, ok0, nf0)
        assert (be <= G.BWD_TOL and fe <= G.FWD_TOL) if T == np.float32 else fe <= 1e-9, (hname, be, fe)
        r["guard"] = (be, fe)
        if r["first_call_s"] > SLOW_CALL_S:
            # WARMUP + ROUNDS more calls of this handle would not fit the step's time limit: its first (guarded) call is what is reported
            print(json.dumps({"n": n, "m": m, "B": B, "handle": hname, "kernel": L.config["kernel"], "ncond": L.info["ncond"], "single_call_s": r["first_call_s"],
                              "guard_backward": be, "guard_forward": fe}), flush=True)
            L.close()
            continue
        runs.append(r)
    for k in range(WARMUP + ROUNDS):
        for r in runs:   # the handles take turns
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hipldl.newton_system_dev(r["L"], r["vals"], r["rhs"], r["d"], r["ro"], r["rho"], r["nf"], r["su"], r["par"], 0)
            e1.record()
            torch.cuda.synchronize()
            if k >= WARMUP:
                r["ms"].append(e0.elapsed_time(e1))
    for r in runs:
        med = float(np.median(r["ms"]))
        row = {"n": n, "m": m, "B": B, "handle": r["name"], "kernel": r["L"].config["kernel"], "ncond": r["L"].info["ncond"],
               "call_ms": med, "call_ms_min": float(min(r["ms"])), "call_ms_max": float(max(r["ms"])), "systems_per_s": B / (med * 1e-3),
               "guard_backward": r["guard"][0], "guard_forward": r["guard"][1],
               "success": int(r["su"].sum().item()), "nfact_max": int(r["nf"].max().item())}
        assert row["success"] == B and row["nfact_max"] == 1, row
        print(json.dumps(row), flush=True)
        r["L"].close()


def main(argv):
    if len(argv) >= 4 and argv[0] == "--one":
        one(int(argv[1]), int(argv[2]), int(argv[3]))
        return 0
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    rows = []
    for n, m, B, limit in CONFIGS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), str(m), str(B)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"dense({n},{m}) x {B}: no result within {limit} s; stopping", flush=True)
            return 1
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(p.stderr[-4000:])
            print(f"dense({n},{m}) x {B}: exit status {p.returncode}; stopping", flush=True)
            return 1
        rows += [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    lines = ["| pattern | handle | kernel | whole call ms (min .. max) | systems/s | guard: backward / forward error |", "|---|---|---|---|---|---|"]
    for r in rows:
        head = f"| dense({r['n']},{r['m']}) x {r['B']} | {r['handle']} | "
        if "error" in r:
            lines.append(head + f"— | creation failed: {r['error']} | — | — |")
        elif "single_call_s" in r:
            lines.append(head + f"{r['kernel']} | {1e3 * r['single_call_s']:.0f} (one call, host clock; not alternated) | {r['B'] / r['single_call_s']:.1f} | "
                         f"{r['guard_backward']:.2e} / {r['guard_forward']:.2e} |")
        else:
            lines.append(head + f"{r['kernel']} | {r['call_ms']:.3f} ({r['call_ms_min']:.3f} .. {r['call_ms_max']:.3f}) | {r['systems_per_s']:.0f} | "
                         f"{r['guard_backward']:.2e} / {r['guard_forward']:.2e} |")
    text = "\n".join(lines) + "\n"
    print()
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
