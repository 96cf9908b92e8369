"""Float32 general handles on the general form of the dense backend (tuning float32_general_dense): the time of
the WHOLE device-resident newton_system! call (cnl_newton_system_f32_dev / cnl_newton_system_dev) and of the solve_ldl! call behind
it (cnl_solve_f32_dev / cnl_solve_dev), taken with device events on the stream, for
  * the Float32 handle with the key (float32_general = 1, float32_general_dense = 1: csrc/dense_f32.hip, the general form),
  * the Float32 handle without it (float32_general = 1, float32_condense = 1 — "v1": the general kernel in float on the condensed
    system; where its creation fails, the error text is recorded instead), and
  * the default Float64 handle (where its batch rule holds: the general form of the dense backend in double)
on three irregular patterns random_structure(n, m, p, density, seed) — condensed orders 129, 454 and 1010 — at 1, 16, 256 and 4096
problems.  A batch the batch rule of the key's value 1 excludes (3 x 16 384 x ceil(order / 64)^2 x batch > 8e9 bytes) is skipped and
listed as such.  Every problem factorises at the first attempt.

One configuration = one child process (a fresh device context) under its own time limit; a child that fails or runs out of time ends
the run.  Inside a child the handles are created once, each passes a parity guard on problem 0 against the CPU oracle (Float32: the
oracle on the widened float32 inputs with ParamCaNNOLeS(Float32), backward error <= 512 eps32, forward error <= 1e-3; Float64:
forward error <= 1e-9), then they take turns call by call: median of ROUNDS calls after WARMUP warm-up calls each, with min .. max.
The guard ASSERTS: one handle that misses its tolerance ends its child, and with it the whole table run — a table is only written
from results that passed.  Run it from a checkout of the repository: the inputs, the oracle and the error measures are the test
suite's (tests/support/f32_general.py, oracle/), imported from the repository root; the library and the oracle have to be built.
Every handle runs with its default dense_graph = 1: both dense handles replay their call sequence as a graph.

usage: time_f32_general_dense.py [--out FILE]     all configurations; the table goes to stdout and, with --out, to FILE
       time_f32_general_dense.py --one K B         pattern K of PATTERNS at batch B (what the driver starts); one JSON line per handle"""
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = [(129, 150, 0, 0.06, 5), (450, 300, 4, 0.02, 1), (1000, 1500, 10, 0.01, 1)]   # random_structure(n, m, p, density, seed)
BATCHES = [(1, 240), (16, 240), (256, 300), (4096, 420)]   # batch, time limit of the child (s)
WARMUP, ROUNDS = 3, 20
SLOW_CALL_S = 2.0   # a handle whose first call takes longer is reported with that one call and takes no turns


def batch_rule(order, batch):
    """the key's value 1 takes the route at this order and batch (csrc/capi_handle.cpp: create_f32_general_from_plan)"""
    return 96 <= order <= 4096 and (batch <= 16 or batch * 3.0 * 16384.0 * math.ceil(order / 64.0) ** 2 <= 8e9)


def one(k, B):
    import numpy as np
    import torch
    torch.zeros(1, device="cuda")   # torch's HIP runtime first (tests/conftest.py)
    sys.path.insert(0, ROOT)
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    from oracle import oracle as O
    from tests.support import f32_general as G

    n, m, p, dens, seed = PATTERNS[k]
    s = syn.random_structure(n, m, p, dens, seed=seed)
    rows, cols = s.kkt_pattern()
    nbase = min(B, 8)
    base = [syn.random_values(s, 40 + 5 * j) for j in range(nbase)]
    vh, rh = np.stack([v for v, _ in base]), np.stack([r for _, r in base])
    rep = (B + nbase - 1) // nbase
    dev = torch.device("cuda", 0)
    orc = O.Oracle(s.N, rows, cols, O.canonical_perm(s.nvar, s.nequ, s.ncon))
    tag = {"pattern": list(PATTERNS[k]), "order": n + p, "B": B}
    handles = (("float32 general dense", np.float32, dict(float32_general=1, float32_general_dense=1), "dense"),
               ("float32 condensed", np.float32, dict(float32_general=1, float32_condense=1), "v1"),
               ("float64 default", np.float64, dict(), None))
    runs, created = [], []
    for hname, T, opt, kernel in handles:
        tt = torch.float32 if T == np.float32 else torch.float64
        try:
            L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=T, options=hipldl.Options(**opt))
        except hipldl.CnlError as e:
            print(json.dumps(dict(tag, handle=hname, error=str(e))), flush=True)
            continue
        assert (kernel is None or L.config["kernel"] == kernel) and L.config["float32"] == (T == np.float32), L.config
        vals = np.ascontiguousarray(np.tile(vh, (rep, 1))[:B], T)
        rhs = np.ascontiguousarray(np.tile(rh, (rep, 1))[:B], T)
        created.append({"name": hname, "L": L, "T": T, "vals": torch.from_numpy(vals).to(dev), "rhs": torch.from_numpy(rhs).to(dev),
                        "d": torch.zeros((B, s.N), dtype=tt, device=dev), "ro": torch.zeros(B, dtype=tt, device=dev), "rho": torch.zeros(B, dtype=tt, device=dev),
                        "nf": torch.zeros(B, dtype=torch.int32, device=dev), "su": torch.zeros(B, dtype=torch.int32, device=dev),
                        "par": hipldl.default_params(T), "ms": [], "solve_ms": [], "host": (vals, rhs)})
    # every handle exists before the first call of any: no creation (hipMalloc, hipMemset, uploads) falls between timed calls
    for r in created:
        hname, L, T, (vals, rhs) = r["name"], r["L"], r["T"], r["host"]
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
            print(json.dumps(dict(tag, handle=hname, kernel=L.config["kernel"], ncond=L.info["ncond"], single_call_s=r["first_call_s"],
                                  guard_backward=be, guard_forward=fe)), flush=True)
            L.close()
            continue
        runs.append(r)
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
        med, smed = float(np.median(r["ms"])), float(np.median(r["solve_ms"]))
        row = dict(tag, handle=r["name"], kernel=r["L"].config["kernel"], ncond=r["L"].info["ncond"],
                   call_ms=med, call_ms_min=float(min(r["ms"])), call_ms_max=float(max(r["ms"])),
                   solve_ms=smed, solve_ms_min=float(min(r["solve_ms"])), solve_ms_max=float(max(r["solve_ms"])),
                   systems_per_s=B / (med * 1e-3), guard_backward=r["guard"][0], guard_forward=r["guard"][1],
                   success=int(r["su"].sum().item()), nfact_max=int(r["nf"].max().item()))
        assert row["success"] == B and row["nfact_max"] == 1, row
        print(json.dumps(row), flush=True)
        r["L"].close()


def main(argv):
    if len(argv) >= 3 and argv[0] == "--one":
        one(int(argv[1]), int(argv[2]))
        return 0
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    rows, skipped = [], []
    for k, pat in enumerate(PATTERNS):
        order = pat[0] + pat[2]
        for B, limit in BATCHES:
            name = f"random{pat} x {B}"
            if not batch_rule(order, B):
                skipped.append(f"{name}: skipped, the batch rule excludes it with value 1 (order {order})")
                print(skipped[-1], flush=True)
                continue
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(k), str(B)], capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                print(f"{name}: no result within {limit} s; stopping", flush=True)
                return 1
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            if p.returncode != 0:
                print(p.stderr[-4000:])
                print(f"{name}: exit status {p.returncode}; stopping", flush=True)
                return 1
            rows += [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    lines = ["| pattern (condensed order) x batch | handle | kernel | newton_system! ms (min .. max) | solve_ldl! ms (min .. max) | systems/s | guard: backward / forward error |",
             "|---|---|---|---|---|---|---|"]
    for r in rows:
        head = f"| random{tuple(r['pattern'])} ({r['order']}) x {r['B']} | {r['handle']} | "
        if "error" in r:
            lines.append(head + f"— | creation failed: {r['error']} | — | — | — |")
        elif "single_call_s" in r:
            lines.append(head + f"{r['kernel']} | {1e3 * r['single_call_s']:.0f} (one call, host clock; not alternated) | — | {r['B'] / r['single_call_s']:.1f} | "
                         f"{r['guard_backward']:.2e} / {r['guard_forward']:.2e} |")
        else:
            lines.append(head + f"{r['kernel']} | {r['call_ms']:.3f} ({r['call_ms_min']:.3f} .. {r['call_ms_max']:.3f}) | "
                         f"{r['solve_ms']:.3f} ({r['solve_ms_min']:.3f} .. {r['solve_ms_max']:.3f}) | {r['systems_per_s']:.0f} | "
                         f"{r['guard_backward']:.2e} / {r['guard_forward']:.2e} |")
    text = "\n".join(lines) + "\n" + "".join("\n" + ln for ln in skipped) + "\n"
    print()
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
