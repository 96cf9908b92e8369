"""The Float32 latency path (tuning float32_latency), by the method of tools/time_f32_staged.py: the time of the
WHOLE device-resident newton_system! call (cnl_newton_system_f32_dev / cnl_newton_system_dev) and of the whole solve_ldl! call behind
it, taken with device events on the stream, for
  * the Float32 handle with float32_general = 1, float32_latency = 1, band_kernel = 0 (the key),
  * the Float32 handle with float32_staged = 1 in its place (one launch per stage, no lean instance: what the key is built on),
  * the default Float64 handle,
  * the key with lean_kernel = 0, with dataflow = 0 and with device_ladder = 0, one at a time,
on band_structure(1000, 10) x 32 / 256 / 4 096, band_structure(10000, 50) x 1 / 256 and band_structure(1000, 10, hw=3) x 256.  Every
problem factorises at the first attempt.  The handles of a shape take turns call by call (the same process, the same device); median
of 10 calls after 3 warm-up calls each, with min .. max.  Last, one CLIMBING batch — band_structure(1000, 10) x 256 with three problems
in every thirteen under stress="ladder" (nfact = 4) — on all of them and on the Float32 handle without either key: what the ladder
costs on the fused launch, on the sequential launch behind the stages, and without a latency plan.
usage: time_f32_latency.py   prints one JSON line per (shape, batch, handle) and two tables."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cannoles_jl_amd  # noqa: F401,E402
from cannoles_jl_amd import hipldl, synthetic as syn  # noqa: E402

WARMUP, STEPS = 3, 10
KEY = dict(float32_general=1, float32_latency=1, band_kernel=0)
HANDLES = (("float32 latency", np.float32, KEY),
           ("float32 staged", np.float32, dict(float32_general=1, float32_staged=1, band_kernel=0)),
           ("float64 default", np.float64, dict()),
           ("key, lean_kernel=0", np.float32, dict(KEY, lean_kernel=0)),
           ("key, dataflow=0", np.float32, dict(KEY, dataflow=0)),
           ("key, device_ladder=0", np.float32, dict(KEY, device_ladder=0)))
UNKEYED = ("float32 without either key", np.float32, dict(float32_general=1, float32_register_front=1, float32_direct_records=1, band_kernel=0))
SHAPES = (("band(1000,10)", (1000, 10, 2), (32, 256, 4096)), ("band(10000,50)", (10000, 50, 2), (1, 256)), ("band(1000,10,hw=3)", (1000, 10, 3), (256,)))
dev = torch.device("cuda", 0)


def make_runs(s, B, vh, rh, handles):
    rows, cols = s.kkt_pattern()
    rep = (B + len(vh) - 1) // len(vh)
    runs = []
    for hname, T, opt in handles:
        tt = torch.float32 if T == np.float32 else torch.float64
        L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=T, options=hipldl.Options(**opt))
        runs.append({"name": hname, "T": T, "L": L,
                     "vals0": torch.from_numpy(np.ascontiguousarray(np.tile(vh, (rep, 1))[:B], T)).to(dev),
                     "rhs": torch.from_numpy(np.ascontiguousarray(np.tile(rh, (rep, 1))[:B], T)).to(dev),
                     "d": torch.zeros((B, s.N), dtype=tt, device=dev), "ro": torch.zeros(B, dtype=tt, device=dev), "rho": torch.zeros(B, dtype=tt, device=dev),
                     "nf": torch.zeros(B, dtype=torch.int32, device=dev), "su": torch.zeros(B, dtype=torch.int32, device=dev),
                     "par": hipldl.default_params(T), "call": [], "solve": []})
        runs[-1]["vals"] = runs[-1]["vals0"].clone()
    return runs


def time_runs(runs, restore):
    for k in range(WARMUP + STEPS):
        for r in runs:   # the handles take turns
            if restore:   # a climbing call writes the rho slots of vals and rho_old: every call starts from the same inputs
                r["vals"].copy_(r["vals0"])
                r["ro"].zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hipldl.newton_system_dev(r["L"], r["vals"], r["rhs"], r["d"], r["ro"], r["rho"], r["nf"], r["su"], r["par"], 0)
            e1.record()
            torch.cuda.synchronize()
            if k >= WARMUP:
                r["call"].append(e0.elapsed_time(e1))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hipldl.solve_dev(r["L"], r["rhs"], r["d"], 0)
            e1.record()
            torch.cuda.synchronize()
            if k >= WARMUP:
                r["solve"].append(e0.elapsed_time(e1))


def rows_of(pname, B, runs):
    out = []
    for r in runs:
        c, L = r["L"].config, r["L"]
        med, smed = float(np.median(r["call"])), float(np.median(r["solve"]))
        out.append({"pattern": pname, "B": B, "handle": r["name"], "kernel": c["kernel"], "lean": c["lean"], "dataflow": c["dataflow"],
                    "lad_mode": c["lad_mode"], "v2_solve": c["v2_solve"],
                    "tasks": len(L.plan_array("tasks")) // 8, "stages": max(0, len(L.plan_array("stage_ptr")) - 1), "order": L.info["order"],
                    "call_ms": med, "call_ms_min": float(min(r["call"])), "call_ms_max": float(max(r["call"])),
                    "solve_ms": smed, "solve_ms_min": float(min(r["solve"])), "solve_ms_max": float(max(r["solve"])),
                    "systems_per_s": B / (med * 1e-3), "success": int(r["su"].sum().item()), "nfact_max": int(r["nf"].max().item()),
                    "dataflow_timeouts": L.dataflow_timeouts() if c["kernel"] == "v2-staged" else 0})
        print(json.dumps(out[-1]), flush=True)
        L.close()
    return out


def show(table):
    print()
    print("| pattern x batch | handle | kernel, lean / dataflow / ladder | tasks / stages | newton_system! ms (min .. max) | solve_ldl! ms (min .. max) | newton / solve against the key |")
    print("|---|---|---|---|---|---|---|")
    for r in table:
        key = next(x for x in table if (x["pattern"], x["B"]) == (r["pattern"], r["B"]) and x["handle"] == "float32 latency")
        slower = [w for w, f in (("newton_system!", "call_ms"), ("solve_ldl!", "solve_ms")) if r[f] < key[f]]
        rel = "" if r is key else f"{r['call_ms'] / key['call_ms']:.2f} x / {r['solve_ms'] / key['solve_ms']:.2f} x" + \
            (f" (the key is SLOWER: {', '.join(slower)})" if slower else "")
        print(f"| {r['pattern']} x {r['B']} | {r['handle']} | {r['kernel']}, {int(r['lean'])} / {int(r['dataflow'])} / {r['lad_mode']} | {r['tasks']} / {r['stages']} | "
              f"{r['call_ms']:.3f} ({r['call_ms_min']:.3f} .. {r['call_ms_max']:.3f}) | "
              f"{r['solve_ms']:.3f} ({r['solve_ms_min']:.3f} .. {r['solve_ms_max']:.3f}) | {rel} |")


table = []
for pname, (n, p, hw), batches in SHAPES:
    s = syn.band_structure(n, p, hw=hw)
    base = [syn.band_values(s, 4000 + k) for k in range(13)]
    vh, rh = np.stack([v for v, _ in base]), np.stack([r for _, r in base])
    for B in batches:
        runs = make_runs(s, B, vh, rh, HANDLES)
        time_runs(runs, restore=False)
        got = rows_of(pname, B, runs)
        for row in got:
            assert row["success"] == B and row["nfact_max"] == 1 and row["dataflow_timeouts"] == 0, row
        table += got
        del runs
        torch.cuda.empty_cache()
show(table)

# ---- one climbing batch ----
s = syn.band_structure(1000, 10)
base = [syn.band_values(s, 4000 + k) for k in range(13)]
for at, k in ((1, 0), (2, 1), (9, 2)):
    base[at] = syn.band_values(s, 7000 + k, stress="ladder")
vh, rh = np.stack([v for v, _ in base]), np.stack([r for _, r in base])
runs = make_runs(s, 256, vh, rh, HANDLES + (UNKEYED,))
time_runs(runs, restore=True)
climb = rows_of("band(1000,10), 3 of 13 problems climb", 256, runs)
for row in climb:   # (ParamCaNNOLeS(Float32)'s ladder reaches these problems' rung at nfact = 4, ParamCaNNOLeS(Float64)'s at 6)
    assert row["success"] == 256 and row["nfact_max"] == (6 if row["handle"] == "float64 default" else 4) and row["dataflow_timeouts"] == 0, row
show(climb)
