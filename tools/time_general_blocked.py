"""The blocked general kernel (tuning general_blocked): the time of the WHOLE cnl_newton_system_dev call and of
the cnl_factorize_dev call, taken with device events on the stream, for
  * the general-kernel handle with the key off  (Options(general_dense=0)),
  * the same handle with the key on             (Options(general_dense=0, general_blocked=1)), and
  * the handle a default Options() gives (the dense route where it applies) — for context only
at the shapes of SHAPES.  Every problem is healthy: it factorises at the first attempt.

One shape = one child process (a fresh device context) under its own time limit; a child that fails or runs out of time ends the
run.  Inside a child every handle is created first and makes one guarded call (all problems succeed, d of key on within 1e-9 of key
off); then the handles take turns call by call, WARMUP rounds and PAIRS measured rounds: medians, and each side's spread (min .. max)
over the rounds.  A difference between key off and key on counts only beyond the larger of the two spreads.

--dtype float32: the same measurement for tuning float32_blocked on Float32 general handles — key off is
Options(float32_general=1, float32_condense=1), key on adds float32_blocked=1, the context handle adds float32_general_dense=1 (the
dense route in float where it applies) — at the shapes of SHAPES_F32, through cnl_newton_system_f32_dev / cnl_factorize_f32_dev; d of
key on within 1e-3 (the Float32 forward tolerance) of key off.

usage: time_general_blocked.py [--dtype float32] [--out FILE]   all shapes; the table goes to stdout and, with --out, to FILE
       time_general_blocked.py --only K,K,...  those shapes of SHAPES alone
       time_general_blocked.py --one K         shape K of SHAPES (what the driver starts); one JSON line per handle"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (generator, its arguments, batch, time limit of the child in s)
SHAPES = [("random", (800, 900, 0, 0.05, 1), 7, 240),
          ("random", (800, 900, 0, 0.05, 1), 256, 400),
          ("random", (1000, 1500, 10, 0.01, 1), 1, 240),
          ("random", (1000, 1500, 10, 0.01, 1), 256, 400),
          ("random", (450, 300, 4, 0.02, 1), 256, 240),
          ("random", (450, 300, 4, 0.02, 1), 4096, 400),
          ("grid", (48,), 256, 300),
          ("grid", (70,), 1, 300),
          ("grid", (70,), 256, 400),
          # two more, at the LDS limit: the work area in LDS with and without the key (135 KB with it), and one the W panel pushes
          # out of LDS (153.6 KB without the key, 169 KB with it: global scratch)
          ("random", (129, 150, 0, 0.06, 5), 256, 240),
          ("random", (136, 157, 0, 0.06, 5), 256, 240)]
# Float32 (--dtype float32); the last one is the shape the W panel pushes out of LDS in float (154.5 KB without the key, 165.5 KB with
# it: global scratch)
SHAPES_F32 = [("random", (129, 150, 0, 0.06, 5), 256, 240),
              ("random", (450, 300, 4, 0.02, 1), 256, 240),
              ("random", (450, 300, 4, 0.02, 1), 4096, 400),
              ("random", (1000, 1500, 10, 0.01, 1), 1, 300),
              ("random", (1000, 1500, 10, 0.01, 1), 256, 500),
              ("grid", (48,), 256, 300),
              ("random", (194, 215, 0, 0.06, 5), 256, 240)]
WARMUP, PAIRS = 2, 8
HANDLES = [("key off", dict(general_dense=0)), ("key on", dict(general_dense=0, general_blocked=1)), ("default", None)]
_F32 = dict(float32_general=1, float32_condense=1)
HANDLES_F32 = [("key off", _F32), ("key on", dict(_F32, float32_blocked=1)), ("default", dict(_F32, float32_general_dense=1))]


def one(k, f32=False):
    import numpy as np
    import torch
    torch.zeros(1, device="cuda")   # torch's HIP runtime first (tests/conftest.py)
    sys.path.insert(0, ROOT)
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    gen, args, B, _ = (SHAPES_F32 if f32 else SHAPES)[k]
    key, np_t, agree_tol = ("float32_blocked", np.float32, 1e-3) if f32 else ("general_blocked", np.float64, 1e-9)
    s = syn.grid_structure(*args) if gen == "grid" else syn.random_structure(*args)
    rows, cols = s.kkt_pattern()
    nbase = min(B, 8)
    base = [syn.random_values(s, 40 + 5 * j) for j in range(nbase)]
    rep = (B + nbase - 1) // nbase
    vh = np.ascontiguousarray(np.tile(np.stack([v for v, _ in base]), (rep, 1))[:B], np_t)
    rh = np.ascontiguousarray(np.tile(np.stack([r for _, r in base]), (rep, 1))[:B], np_t)
    dev = torch.device("cuda", 0)
    p = hipldl.default_params(np_t)
    f64, i32 = dict(dtype=torch.float32 if f32 else torch.float64, device=dev), dict(dtype=torch.int32, device=dev)   # (f64: the element type)
    runs = []
    for name, opt in HANDLES_F32 if f32 else HANDLES:
        L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np_t, options=hipldl.Options(**opt) if opt else None)
        runs.append(dict(name=name, L=L, vals=torch.from_numpy(vh).to(dev), rhs=torch.from_numpy(rh).to(dev), d=torch.zeros((B, s.N), **f64),
                         ro=torch.zeros(B, **f64), rho=torch.zeros(B, **f64), nf=torch.zeros(B, **i32), su=torch.zeros(B, **i32)))

    def newton(r):
        hipldl.newton_system_dev(r["L"], r["vals"].data_ptr(), r["rhs"].data_ptr(), r["d"].data_ptr(), r["ro"].data_ptr(), r["rho"].data_ptr(),
                                 r["nf"].data_ptr(), r["su"].data_ptr(), p, 0)

    def factorize(r):
        hipldl.factorize_dev(r["L"], r["vals"].data_ptr(), float(p[0]), r["su"].data_ptr(), stream=0)

    for r in runs:   # every handle exists before the first call of any; one guarded call each
        newton(r)
        torch.cuda.synchronize()
        assert int(r["su"].sum().item()) == B and int(r["nf"].max().item()) == 1, r["name"]
    off, on = runs[0], runs[1]
    assert on["L"].config["kernel"] == off["L"].config["kernel"] == "v1" and not off["L"].config[key]
    agree = float(((on["d"] - off["d"]).abs().amax(1) / off["d"].abs().amax(1)).max().item())
    assert agree <= agree_tol, agree
    for r in runs:
        r["newton"], r["factor"] = [], []
    for it in range(WARMUP + PAIRS):
        for r in runs:   # the handles take turns
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            newton(r)
            e1.record()
            factorize(r)
            e2.record()
            torch.cuda.synchronize()
            if it >= WARMUP:
                r["newton"].append(e0.elapsed_time(e1))
                r["factor"].append(e1.elapsed_time(e2))
    for r in runs:
        c = r["L"].config
        print(json.dumps(dict(pattern=f"{gen}{tuple(args)}", B=B, N=s.N, fmax=r["L"].info["fmax"], handle=r["name"], kernel=c["kernel"],
                              blocked=c[key], tpp=c["tpp"], lds_work=c["lds_work"], agree=agree,
                              newton=[float(np.median(r["newton"])), min(r["newton"]), max(r["newton"])],
                              factor=[float(np.median(r["factor"])), min(r["factor"]), max(r["factor"])])), flush=True)
    for r in runs:
        r["L"].close()


def verdict(off, on):
    """key on against key off: the ratio of the medians, and whether the difference exceeds the larger spread"""
    spread = max(off[2] - off[1], on[2] - on[1])
    diff = on[0] - off[0]
    word = "same" if abs(diff) <= spread else ("FASTER" if diff < 0 else "SLOWER")
    return f"{off[0] / on[0]:6.2f}x {word}"


def main(argv):
    f32 = "--dtype" in argv and argv[argv.index("--dtype") + 1] == "float32"
    if "--one" in argv:
        return one(int(argv[argv.index("--one") + 1]), f32)
    shapes = SHAPES_F32 if f32 else SHAPES
    lines = [f"{'float32_blocked' if f32 else 'general_blocked'}: whole-call device time in ms, median [min .. max] of {PAIRS} alternated rounds after {WARMUP} warm-up rounds",
             "pattern, batch, fmax | call | key off | key on | off/on, beyond the larger spread? | " + ("float32_general_dense=1 (context)" if f32 else "default Options() (context)")]
    only = [int(x) for x in argv[argv.index("--only") + 1].split(",")] if "--only" in argv else list(range(len(shapes)))
    for k, (gen, args, B, limit) in enumerate(shapes):
        if k not in only:
            continue
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--one", str(k)] + (["--dtype", "float32"] if f32 else []), cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            lines.append(f"{gen}{args} x {B}: child exited with {r.returncode}; the run ends here\n{r.stderr[-2000:]}")
            break
        rec = {j["handle"]: j for j in (json.loads(l) for l in r.stdout.splitlines() if l.startswith("{"))}
        off, on, dflt = rec["key off"], rec["key on"], rec["default"]
        fmt = lambda t: f"{t[0]:9.3f} [{t[1]:9.3f} .. {t[2]:9.3f}]"
        for call in ("newton", "factor"):
            lines.append(f"{off['pattern']} x {B}, fmax {off['fmax']}, tpp {on['tpp']}, lds_work {off['lds_work']}/{on['lds_work']} | {call:6s} | {fmt(off[call])} | "
                         f"{fmt(on[call])} | {verdict(off[call], on[call])} | {dflt['kernel']}: {fmt(dflt[call])}")
        print("\n".join(lines[-2:]), flush=True)
    text = "\n".join(lines) + "\n"
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as f:
            f.write(text)
    return 0 if len(lines) == 2 + 2 * len(only) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
