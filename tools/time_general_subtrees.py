"""The general kernel's subtree execution (tuning general_subtrees): whole-call device time of
cnl_newton_system_dev, cnl_factorize_dev and cnl_solve_dev, taken with device events on the stream, for the SAME handle options with
the key off and on.

One process.  Per case both handles are created first and make one guarded call (key on agrees with key off in success, nfact and,
within 1e-9, d); then they take turns call by call, WARMUP rounds and ROUNDS measured rounds: medians, and each side's spread
(min .. max).  A case counts as FASTER or SLOWER only when the medians differ by more than the larger of the two spreads; otherwise
it is level.  The baseline is always the key-off handle of the same process.

Cases (CASES): grid_structure(48) and (70) at batch 1, 16 and 256 with general_blocked 0 and 1; task_cap 4, 8, 16, 32 on
grid_structure(70) x 1 and x 256; the two chain-like trees; the seven-kind mix (tests/support/dense_general_cases.py) repeated to 256
problems on grid_structure(48), which pays the climbers' repeated first attempt.  Healthy problems everywhere else.

--dtype float32: the same measurement for tuning float32_subtrees on Float32 general handles — the
float32_condense handle with float32_blocked = 1 on both sides, Float32 data and parameters, CASES_F32: grid_structure(48) and (70) at
batch 1, 16 and 256, the two chain-like trees, and the Float32 five-kind mix (tests/support/f32_general_dense.py) repeated to 256
problems on grid_structure(48); d of the two handles is compared within the Float32 forward bar (1e-3).

--ladder R,R,...: the staged rho ladder (tuning subtree_ladder).  newton_system alone, LADDER_CASES, and per case
the sides "subtree key off" (the classic kernel), "key on, R = 0" (the sequence without the ladder key) and "key on, subtree_ladder = R"
for every R given, general_blocked / float32_blocked = 1 on all sides, all in one process and taking turns call by call.  Every side
must agree with the key-off side in success, nfact and rho, and every R > 0 bit for bit with R = 0 in every output.  The cases: the
mix x 256 on grid_structure(48); grid_structure(70) x 1 with the one problem of kind 2 (nfact 6, in float 5) and of kind 3 (nfact 4);
grid_structure(70) x 16 with one kind-2 climber among healthy problems; the healthy grid_structure(70) x 1 and x 256 and
grid_structure(48) x 256, where a rung is S + 1 empty launches.

--wide: the per-stage launch shapes (tuning subtree_wide = W and subtree_lds_panels = M).  newton_system_dev and
factorize_dev, WIDE_CASES in both element types (one table, Float64 first), the subtree key and the blocked key on on every side.  Sides, all
in one process and taking turns call by call: both keys off; W = 1, 96, 128, 160; M = 4096 alone; every W with M = 4096 (the row of the
W with the lowest newton_system median is marked "best W + M").  Every side must agree with the keys-off side bit for bit in success,
nfact, rho, rho_old, d and vals.  The last case is grid_structure(70) x 1 with subtree_ladder = 5 on every side and the one problem of
kind 2 climbing.  Each row also gives the table of cnl_subtree_stage_shape as threads per stage and LPAN stages.

--solve-panels: the solve sweeps in panels of 16 pivots (tuning subtree_solve_panels = P).  newton_system_dev and
solve_dev (on the factor the newton_system call before it left), WIDE_CASES in both element types, the subtree key and the blocked key on on
every side.  Sides, all in one process and taking turns call by call: P = 0, 1, 2, 3; then P = 0 and 3 again with subtree_wide = 1 and
subtree_lds_panels = 4096.  Every side is checked against the P = 0 side of the same launch shapes: success, nfact, rho, rho_old and vals bit
for bit, d of both calls bit for bit for P = 2 and within the forward bar (1e-9; float: FWD_TOL of tests/support/f32_general.py) for
P = 1 and 3, the launch counts equal.

usage: time_general_subtrees.py [--dtype float32] [--only K,K,...] [--out FILE]
       time_general_subtrees.py --wide [--only K,K,...] [--out FILE]
       time_general_subtrees.py --solve-panels [--only K,K,...] [--out FILE]
       time_general_subtrees.py --trace-wide W,M[,P] [--with-solve]   grid_structure(70) x 1, general_blocked = 1, the keys as given
                                             (P: subtree_solve_panels): three newton_system calls, with --with-solve three solve calls behind them
       time_general_subtrees.py --ladder 3,5,19 [--dtype float32] [--only K,K,...] [--out FILE]
       time_general_subtrees.py --trace      grid_structure(70) x 1, key on, general_blocked = 1: three newton_system calls and nothing
                                             else, for a kernel trace taken from outside (profiles/general_subtrees_trace.txt)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, ROUNDS = 2, 8
BASE = dict(general_dense=0, register_front=0, dense_backend=0)
# (generator, its arguments, batch, extra options, values: "healthy" or "mix")
CASES = ([("grid", (G,), B, dict(general_blocked=blk), "healthy") for G in (48, 70) for B in (1, 16, 256) for blk in (0, 1)] +
         [("grid", (70,), B, dict(general_blocked=1, task_cap=cap), "healthy") for B in (1, 256) for cap in (4, 8, 16, 32)] +
         [("random", (450, 300, 4, 0.02, 1), 256, dict(general_blocked=1), "healthy"),
          ("random", (1000, 1500, 10, 0.01, 1), 1, dict(general_blocked=1), "healthy"),
          ("grid", (48,), 256, dict(general_blocked=1), "mix")])
BASE_F32 = dict(float32_general=1, float32_condense=1)
CASES_F32 = ([("grid", (G,), B, dict(float32_blocked=1), "healthy") for G in (48, 70) for B in (1, 16, 256)] +
             [("random", (450, 300, 4, 0.02, 1), 256, dict(float32_blocked=1), "healthy"),
              ("random", (1000, 1500, 10, 0.01, 1), 1, dict(float32_blocked=1), "healthy"),
              ("grid", (48,), 256, dict(float32_blocked=1), "mix")])
# --ladder: (generator, its arguments, batch, values) — "mix", "healthy", "kind2" / "kind3" (every problem of that kind of the mix),
# "one-climber" (problem 0 of kind 2, the others healthy)
LADDER_CASES = [("grid", (48,), 256, "mix"), ("grid", (70,), 1, "kind2"), ("grid", (70,), 1, "kind3"), ("grid", (70,), 16, "one-climber"),
                ("grid", (70,), 1, "healthy"), ("grid", (70,), 256, "healthy"), ("grid", (48,), 256, "healthy")]
# --wide: (generator, its arguments, batch, values, subtree_ladder)
WIDE_CASES = ([("grid", (70,), B, "healthy", 0) for B in (1, 16, 256)] + [("grid", (48,), B, "healthy", 0) for B in (1, 256)] +
              [("random", (1000, 1500, 10, 0.01, 1), 1, "healthy", 0), ("grid", (70,), 1, "kind2", 5)])
WIDE_W, WIDE_M = (1, 96, 128, 160), 4096
F32 = False      # --dtype float32


def setup():
    import torch
    torch.zeros(1, device="cuda")   # torch's HIP runtime first (tests/conftest.py)
    sys.path.insert(0, ROOT)
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    return torch, hipldl, syn


def inputs(syn, s, B, kind):
    import numpy as np
    if kind == "mix":
        if F32:
            from tests.support import f32_general_dense as GC
        else:
            from tests.support import dense_general_cases as GC
        v, r, ro = GC.values(s, GC.MIX)
        rep = (B + GC.MIX - 1) // GC.MIX
        return (np.ascontiguousarray(np.tile(v, (rep, 1))[:B]), np.ascontiguousarray(np.tile(r, (rep, 1))[:B]), np.ascontiguousarray(np.tile(ro, rep)[:B]))
    if kind in ("kind2", "kind3", "one-climber"):      # the mix's rule for an indefinite Hessian block (kind 3: from rho_old = 2)
        from tests.support import dense_general_cases as GC
        v, r, ro = inputs(syn, s, B, "healthy")
        for b in range(B if kind != "one-climber" else 1):
            ro[b] = GC.apply_kind(s, v[b], 3 if kind == "kind3" else 2)
        return v, r, ro
    nbase = min(B, 8)
    base = [syn.random_values(s, 40 + 5 * j) for j in range(nbase)]
    rep = (B + nbase - 1) // nbase
    return (np.ascontiguousarray(np.tile(np.stack([v for v, _ in base]), (rep, 1))[:B]),
            np.ascontiguousarray(np.tile(np.stack([r for _, r in base]), (rep, 1))[:B]), np.zeros(B))


def make_runs(torch, hipldl, syn, case, keys=(0, 1)):
    """keys: the sides — 0 / 1 the subtree key, (1, R) the subtree key with subtree_ladder = R, or a dict of further options beside the
    subtree key (--wide)"""
    import numpy as np
    gen, args, B, extra, kind = case
    s = syn.grid_structure(*args) if gen == "grid" else syn.random_structure(*args)
    rows, cols = s.kkt_pattern()
    vh, rh, roh = (np.ascontiguousarray(a, np.float32 if F32 else np.float64) for a in inputs(syn, s, B, kind))
    dev = torch.device("cuda", 0)
    f64, i32 = dict(dtype=torch.float32 if F32 else torch.float64, device=dev), dict(dtype=torch.int32, device=dev)   # (the run's element type)
    runs = []
    for key in keys:
        more = key if isinstance(key, dict) else {}
        key, rungs = key if isinstance(key, tuple) else (1 if isinstance(key, dict) else key, None)
        opt = dict(BASE_F32, float32_subtrees=key, **extra, **more) if F32 else dict(BASE, general_subtrees=key, **extra, **more)
        if rungs is not None:
            opt["subtree_ladder"] = rungs
        if gen == "grid" and not F32:
            opt["plan_kind"] = hipldl.PLAN_THROUGHPUT
        L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, options=hipldl.Options(**opt), **(dict(dtype=np.float32) if F32 else {}))
        runs.append(dict(key=key, rungs=rungs, more=more, L=L, vh=torch.from_numpy(vh).to(dev), vals=torch.from_numpy(vh).to(dev), rhs=torch.from_numpy(rh).to(dev), roh=torch.from_numpy(roh).to(dev),
                         d=torch.zeros((B, s.N), **f64), ro=torch.zeros(B, **f64), rho=torch.zeros(B, **f64), nf=torch.zeros(B, **i32), su=torch.zeros(B, **i32)))
    return s, runs


def one(torch, hipldl, syn, case):
    import numpy as np
    gen, args, B, extra, kind = case
    p = hipldl.default_params(np.float32) if F32 else hipldl.default_params()
    KEY, BLK = ("float32_subtrees", "float32_blocked") if F32 else ("general_subtrees", "general_blocked")
    s, runs = make_runs(torch, hipldl, syn, case)

    def reset(r):      # (the ladder writes the rho slots of vals and rho_old: every call starts from the same inputs)
        r["vals"].copy_(r["vh"])
        r["ro"].copy_(r["roh"])

    def newton(r):
        hipldl.newton_system_dev(r["L"], r["vals"].data_ptr(), r["rhs"].data_ptr(), r["d"].data_ptr(), r["ro"].data_ptr(), r["rho"].data_ptr(),
                                 r["nf"].data_ptr(), r["su"].data_ptr(), p, 0)

    def factorize(r):
        hipldl.factorize_dev(r["L"], r["vals"].data_ptr(), float(p[0]), r["su"].data_ptr(), stream=0)

    def solve(r):
        hipldl.solve_dev(r["L"], r["rhs"].data_ptr(), r["d"].data_ptr(), stream=0)

    for r in runs:
        reset(r)
        r["d"].fill_(7.0)
        newton(r)
        torch.cuda.synchronize()
    off, on = runs
    assert off["L"].config["kernel"] == on["L"].config["kernel"] == "v1" and not off["L"].config[KEY], (off["L"].config, on["L"].config)
    assert off["L"].config["float32"] == on["L"].config["float32"] == F32 and off["L"].config[BLK] == on["L"].config[BLK]
    assert torch.equal(on["su"], off["su"]) and torch.equal(on["nf"], off["nf"]) and torch.equal(on["rho"], off["rho"])
    ok = off["su"] == 1
    if kind == "healthy":
        assert bool(ok.all()) and int(off["nf"].max().item()) == 1
    agree = float(((on["d"][ok] - off["d"][ok]).abs().amax(1) / off["d"][ok].abs().amax(1)).max().item())
    assert agree <= (1e-3 if F32 else 1e-9), agree
    bit_equal = bool(torch.equal(on["d"][ok], off["d"][ok]))
    for r in runs:
        r["t"] = dict(newton=[], factor=[], solve=[])
    for it in range(WARMUP + ROUNDS):
        for r in runs:   # the handles take turns; each call between events of its own (solve on the factor of the call before it)
            for name, fn in (("newton", newton), ("factor", factorize), ("solve", solve)):
                if name != "solve":
                    reset(r)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(r)
                e1.record()
                torch.cuda.synchronize()
                if it >= WARMUP:
                    r["t"][name].append(e0.elapsed_time(e1))
    out = []
    for r in runs:
        c = r["L"].config
        gi = r["L"].plan_array("ginfo").tolist()
        out.append(dict(pattern=f"{gen}{tuple(args)}", B=B, N=s.N, fmax=r["L"].info["fmax"], key=r["key"], subtrees=c[KEY], blocked=c[BLK],
                        tpp=c["tpp"], lds_work=c["lds_work"], extra=extra, values=kind, ginfo=gi, bit_equal=bit_equal, agree=agree,
                        **{k: [float(np.median(v)), min(v), max(v)] for k, v in r["t"].items()}))
    for r in runs:
        r["L"].close()
    return out


def ladder_one(torch, hipldl, syn, case, Rs):
    """one case of --ladder: sides key off, (key on, R = 0), (key on, R) for R in Rs; newton_system only"""
    import numpy as np
    gen, args, B, kind = case
    p = hipldl.default_params(np.float32) if F32 else hipldl.default_params()
    KEY, BLK = ("float32_subtrees", "float32_blocked") if F32 else ("general_subtrees", "general_blocked")
    extra = {BLK: 1}
    s, runs = make_runs(torch, hipldl, syn, (gen, args, B, extra, kind), keys=[0, (1, 0)] + [(1, R) for R in Rs])

    def newton(r):
        r["vals"].copy_(r["vh"])
        r["ro"].copy_(r["roh"])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hipldl.newton_system_dev(r["L"], r["vals"].data_ptr(), r["rhs"].data_ptr(), r["d"].data_ptr(), r["ro"].data_ptr(), r["rho"].data_ptr(),
                                 r["nf"].data_ptr(), r["su"].data_ptr(), p, 0)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for r in runs:
        r["d"].fill_(7.0)
        before = hipldl.launch_counts()["general"]
        newton(r)
        r["launches"] = hipldl.launch_counts()["general"] - before
    off, r0 = runs[0], runs[1]
    assert not off["L"].config[KEY] and off["L"].config["subtree_ladder"] == 0, off["L"].config
    for r in runs[1:]:
        c = r["L"].config
        assert c[KEY] and c["subtree_ladder"] == r["rungs"] and c[BLK] == off["L"].config[BLK] and c["kernel"] == "v1", c
        for k in ("su", "nf", "rho", "ro"):
            assert torch.equal(r[k], off[k]), (r["rungs"], k)
        for k in ("su", "nf", "rho", "ro", "d", "vals"):      # bit for bit the sequence without the ladder key (NaN inputs compare as bits)
            a, b = r[k], r0[k]
            assert torch.equal(a.view(torch.int32 if a.element_size() == 4 else torch.int64), b.view(torch.int32 if b.element_size() == 4 else torch.int64)), (r["rungs"], k)
    if kind == "healthy":
        assert bool((off["su"] == 1).all()) and int(off["nf"].max().item()) == 1
    nf = off["nf"].cpu().numpy()
    for r in runs:
        r["t"] = []
    for it in range(WARMUP + ROUNDS):
        for r in runs:
            t = newton(r)
            if it >= WARMUP:
                r["t"].append(t)
    gi = r0["L"].plan_array("ginfo").tolist()
    out = dict(pattern=f"{gen}{tuple(args)}", B=B, N=s.N, values=kind, ginfo=gi, tpp=r0["L"].config["tpp"], nfact=sorted(set(int(x) for x in nf)),
               sides=[dict(key=r["key"], rungs=r["rungs"], launches=r["launches"], t=[float(np.median(r["t"])), min(r["t"]), max(r["t"])]) for r in runs])
    for r in runs:
        r["L"].close()
    return out


def ladder(argv):
    torch, hipldl, syn = setup()
    Rs = [int(x) for x in argv[argv.index("--ladder") + 1].split(",")]
    only = [int(x) for x in argv[argv.index("--only") + 1].split(",")] if "--only" in argv else list(range(len(LADDER_CASES)))
    key = "float32_subtrees" if F32 else "general_subtrees"
    lines = [f"subtree_ladder with {key} ({'float32_blocked' if F32 else 'general_blocked'} = 1 on all sides): whole-call device time of newton_system_dev in ms, "
             f"median [min .. max] of {ROUNDS} alternated rounds after {WARMUP} warm-up rounds, one process; every side agrees with the key-off side in success, nfact, rho, rho_old "
             f"and every R > 0 with R = 0 bit for bit in every output",
             "pattern x batch, values (nfact present), tasks / stages, tpp | side | launches | time | against key off | against R = 0 (beyond the larger spread?)"]
    fmt = lambda t: f"{t[0]:9.3f} [{t[1]:9.3f} .. {t[2]:9.3f}]"
    for k in only:
        t0 = time.time()
        o = ladder_one(torch, hipldl, syn, LADDER_CASES[k], Rs)
        head = f"{o['pattern']} x {o['B']}, {o['values']} (nfact {o['nfact']}), {o['ginfo'][1]} / {o['ginfo'][2]}, tpp {o['tpp']}"
        off, r0 = o["sides"][0]["t"], o["sides"][1]["t"]
        n0 = len(lines)
        for sd in o["sides"]:
            name = "key off" if not sd["key"] else f"key on, R = {sd['rungs']}"
            lines.append(f"[{k}] {head} | {name:16s} | {sd['launches']:4d} | {fmt(sd['t'])} | {verdict(off, sd['t']) if sd['key'] else '':>16s} | "
                         f"{verdict(r0, sd['t']) if sd['key'] and sd['rungs'] else ''}")
        print("\n".join(lines[n0:]) + f"\n    ({time.time() - t0:.1f} s)", flush=True)
        print(json.dumps(o), file=sys.stderr, flush=True)
        if "--out" in argv:      # (written case by case: what was measured is kept if a later case is not reached)
            with open(argv[argv.index("--out") + 1], "w") as f:
                f.write("\n".join(lines) + "\n")
    return 0


def wide_one(torch, hipldl, syn, case):
    """one case of --wide in the element type F32 says: the sides of the module docstring, newton_system and factorize"""
    import numpy as np
    gen, args, B, kind, R = case
    p = hipldl.default_params(np.float32) if F32 else hipldl.default_params()
    KEY, BLK = ("float32_subtrees", "float32_blocked") if F32 else ("general_subtrees", "general_blocked")
    extra = {BLK: 1}
    if R:
        extra["subtree_ladder"] = R
    sides = [{}] + [dict(subtree_wide=W) for W in WIDE_W] + [dict(subtree_lds_panels=WIDE_M)] + [dict(subtree_wide=W, subtree_lds_panels=WIDE_M) for W in WIDE_W]
    s, runs = make_runs(torch, hipldl, syn, (gen, args, B, extra, kind), keys=sides)

    def timed(r, call):
        r["vals"].copy_(r["vh"])
        r["ro"].copy_(r["roh"])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if call == "newton":
            hipldl.newton_system_dev(r["L"], r["vals"].data_ptr(), r["rhs"].data_ptr(), r["d"].data_ptr(), r["ro"].data_ptr(), r["rho"].data_ptr(),
                                     r["nf"].data_ptr(), r["su"].data_ptr(), p, 0)
        else:
            hipldl.factorize_dev(r["L"], r["vals"].data_ptr(), float(p[0]), r["su"].data_ptr(), stream=0)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    off = runs[0]
    for r in runs:
        r["d"].fill_(7.0)
        before = hipldl.launch_counts()["general"]
        timed(r, "newton")
        r["launches"] = hipldl.launch_counts()["general"] - before
        c = r["L"].config
        assert c[KEY] and c[BLK] and c["kernel"] == "v1" and c["subtree_ladder"] == R and r["launches"] == off["launches"], (c, r["launches"])
        tpp, lds = hipldl.subtree_stage_shape(r["L"])
        r["tpp"], r["lpan"] = tpp.tolist(), (lds > 16 * (4 if F32 else 8)).astype(int).tolist()
        assert c["subtree_wide"] == (max(r["tpp"]) > c["tpp"]) and c["subtree_lds_panels"] == bool(max(r["lpan"]))
        for k in ("su", "nf", "rho", "ro", "d", "vals"):      # bit for bit the keys-off side (NaN compares as bits)
            a, b = r[k], off[k]
            assert torch.equal(a.view(torch.int32 if a.element_size() == 4 else torch.int64), b.view(torch.int32 if b.element_size() == 4 else torch.int64)), (r["more"], k)
    assert off["tpp"] == [off["L"].config["tpp"]] * len(off["tpp"]) and not max(off["lpan"])
    if kind == "healthy":
        assert bool((off["su"] == 1).all()) and int(off["nf"].max().item()) == 1
    for r in runs:
        r["t"] = dict(newton=[], factor=[])
    for it in range(WARMUP + ROUNDS):
        for r in runs:
            for call in ("newton", "factor"):
                t = timed(r, call)
                if it >= WARMUP:
                    r["t"][call].append(t)
    gi = off["L"].plan_array("ginfo").tolist()
    F = [int(max(t[7] for t in off["L"].plan_array("gtasks").reshape(-1, 8) if t[0] == st)) for st in range(gi[2])]
    out = dict(pattern=f"{gen}{tuple(args)}", B=B, N=s.N, values=kind, rungs=R, ginfo=gi, tpp=off["L"].config["tpp"], nfact=sorted(set(int(x) for x in off["nf"].cpu().numpy())),
               F=F, stage_tasks=np.diff(off["L"].plan_array("gstage_ptr")).tolist(), launches=off["launches"],
               sides=[dict(keys=r["more"], tpp=r["tpp"], lpan=r["lpan"], **{k: [float(np.median(v)), min(v), max(v)] for k, v in r["t"].items()}) for r in runs])
    for r in runs:
        r["L"].close()
    return out


def wide(argv):
    global F32
    torch, hipldl, syn = setup()
    only = [int(x) for x in argv[argv.index("--only") + 1].split(",")] if "--only" in argv else list(range(len(WIDE_CASES)))
    lines = [f"subtree_wide = W / subtree_lds_panels = M on subtree handles, blocked key on on every side: whole-call device time in ms, median [min .. max] of {ROUNDS} "
             f"alternated rounds after {WARMUP} warm-up rounds, one process; every side agrees with the keys-off side bit for bit in success, nfact, rho, rho_old, d and vals",
             "against keys off: off / side, FASTER or SLOWER only beyond the larger of the two spreads; ** ** marks what is slower",
             "[case] pattern x batch, element type, values, F_s per stage, tasks per stage | side: stages at 1024 threads, LPAN stages | newton_system | against keys off | factorize | against keys off"]
    fmt = lambda t: f"{t[0]:9.3f} [{t[1]:9.3f} .. {t[2]:9.3f}]"

    def mark(v):
        return f"**{v.strip()}**" if v.endswith("SLOWER") else v.strip()
    for k in only:
        for f32 in (False, True):
            F32 = f32
            t0 = time.time()
            o = wide_one(torch, hipldl, syn, WIDE_CASES[k])
            head = (f"[{k}] {o['pattern']} x {o['B']}, {'Float32' if f32 else 'Float64'}, {o['values']}{', subtree_ladder = %d (nfact %s)' % (o['rungs'], o['nfact']) if o['rungs'] else ''}, "
                    f"F_s {o['F']}, tasks {o['stage_tasks']}, {o['launches']} launches per newton_system")
            lines.append(head)
            off = o["sides"][0]
            ws = [sd for sd in o["sides"] if set(sd["keys"]) == {"subtree_wide"}]
            best = min(ws, key=lambda sd: sd["newton"][0])["keys"]["subtree_wide"]
            n0 = len(lines) - 1
            for sd in o["sides"]:
                name = ", ".join(f"{'W' if a == 'subtree_wide' else 'M'} = {b}" for a, b in sd["keys"].items()) or "keys off"
                if sd["keys"] == dict(subtree_wide=best, subtree_lds_panels=WIDE_M):
                    name += " (best W + M)"
                shape = f"{sum(1 for t in sd['tpp'] if t == 1024)} wide {''.join('w' if t == 1024 else '.' for t in sd['tpp'])}, {sum(sd['lpan'])} LPAN {''.join('l' if x else '.' for x in sd['lpan'])}"
                cmp_ = ["", ""] if not sd["keys"] else [mark(verdict(off[c], sd[c])) for c in ("newton", "factor")]
                lines.append(f"    {name:34s} | {shape} | {fmt(sd['newton'])} | {cmp_[0]:>18s} | {fmt(sd['factor'])} | {cmp_[1]:>18s}")
            print("\n".join(lines[n0:]) + f"\n    ({time.time() - t0:.1f} s)", flush=True)
            print(json.dumps(o), file=sys.stderr, flush=True)
            if "--out" in argv:      # (written case by case: what was measured is kept if a later case is not reached)
                with open(argv[argv.index("--out") + 1], "w") as f:
                    f.write("\n".join(lines) + "\n")
    return 0


SOLVE_SIDES = [dict(subtree_solve_panels=P) if P else {} for P in (0, 1, 2, 3)] + [dict(subtree_wide=1, subtree_lds_panels=WIDE_M),
                                                                                   dict(subtree_wide=1, subtree_lds_panels=WIDE_M, subtree_solve_panels=3)]


def solve_one(torch, hipldl, syn, case):
    """one case of --solve-panels in the element type F32 says: newton_system and solve (on the factor newton_system left), the sides
    SOLVE_SIDES; every side with P > 0 is checked against the P = 0 side of the same launch shapes"""
    import numpy as np
    gen, args, B, kind, R = case
    p = hipldl.default_params(np.float32) if F32 else hipldl.default_params()
    KEY, BLK = ("float32_subtrees", "float32_blocked") if F32 else ("general_subtrees", "general_blocked")
    if F32:
        from tests.support.f32_general import FWD_TOL
    else:
        FWD_TOL = 1e-9
    extra = {BLK: 1}
    if R:
        extra["subtree_ladder"] = R
    s, runs = make_runs(torch, hipldl, syn, (gen, args, B, extra, kind), keys=SOLVE_SIDES)
    bits = lambda a: a.view(torch.int32 if a.element_size() == 4 else torch.int64)

    def timed(r, call):
        if call == "newton":
            r["vals"].copy_(r["vh"])
            r["ro"].copy_(r["roh"])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if call == "newton":
            hipldl.newton_system_dev(r["L"], r["vals"].data_ptr(), r["rhs"].data_ptr(), r["d"].data_ptr(), r["ro"].data_ptr(), r["rho"].data_ptr(),
                                     r["nf"].data_ptr(), r["su"].data_ptr(), p, 0)
        else:
            hipldl.solve_dev(r["L"], r["rhs"].data_ptr(), r["d2"].data_ptr(), stream=0)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for r in runs:
        r["d"].fill_(7.0)
        r["d2"] = torch.full_like(r["d"], 7.0)
        r["P"] = r["more"].get("subtree_solve_panels", 0)
        n0 = hipldl.launch_counts()["general"]
        timed(r, "newton")
        n1 = hipldl.launch_counts()["general"]
        timed(r, "solve")
        r["launches"] = (n1 - n0, hipldl.launch_counts()["general"] - n1)
        c = r["L"].config
        assert c[KEY] and c[BLK] and c["kernel"] == "v1" and c["subtree_ladder"] == R and c["subtree_solve_panels"] == r["P"], c
        base = next(q for q in runs if q["P"] == 0 and q["more"].get("subtree_wide", 0) == r["more"].get("subtree_wide", 0))
        assert r["launches"] == base["launches"], (r["more"], r["launches"])
        ok = base["su"] == 1
        r["agree"] = 0.0
        for k in ("su", "nf", "rho", "ro", "vals"):      # the decisions and the rho slots: bit for bit
            assert torch.equal(bits(r[k]), bits(base[k])), (r["more"], k)
        for k in ("d", "d2"):
            if r["P"] in (0, 2):                          # the forward substitution in panels: d bit for bit
                assert torch.equal(bits(r[k]), bits(base[k])), (r["more"], k)
                continue
            assert bool((r[k][~ok] == 7.0).all())
            if bool(ok.any()):
                r["agree"] = max(r["agree"], float(((r[k][ok] - base[k][ok]).abs().amax(1) / base[k][ok].abs().amax(1)).max().item()))
        assert r["agree"] <= FWD_TOL, (r["more"], r["agree"])
    if kind == "healthy":
        assert bool((runs[0]["su"] == 1).all()) and int(runs[0]["nf"].max().item()) == 1
    for r in runs:
        r["t"] = dict(newton=[], solve=[])
    for it in range(WARMUP + ROUNDS):
        for r in runs:
            for call in ("newton", "solve"):
                t = timed(r, call)
                if it >= WARMUP:
                    r["t"][call].append(t)
    off = runs[0]
    gi = off["L"].plan_array("ginfo").tolist()
    F = [int(max(t[7] for t in off["L"].plan_array("gtasks").reshape(-1, 8) if t[0] == st)) for st in range(gi[2])]
    out = dict(pattern=f"{gen}{tuple(args)}", B=B, N=s.N, values=kind, rungs=R, ginfo=gi, tpp=off["L"].config["tpp"], nfact=sorted(set(int(x) for x in off["nf"].cpu().numpy())),
               F=F, stage_tasks=np.diff(off["L"].plan_array("gstage_ptr")).tolist(), launches=off["launches"],
               sides=[dict(keys=r["more"], agree=r["agree"], **{k: [float(np.median(v)), min(v), max(v)] for k, v in r["t"].items()}) for r in runs])
    for r in runs:
        r["L"].close()
    return out


def solve_panels(argv):
    global F32
    torch, hipldl, syn = setup()
    only = [int(x) for x in argv[argv.index("--only") + 1].split(",")] if "--only" in argv else list(range(len(WIDE_CASES)))
    lines = [f"subtree_solve_panels = P on subtree handles, blocked key on on every side: whole-call device time in ms, median [min .. max] of {ROUNDS} alternated rounds after "
             f"{WARMUP} warm-up rounds, one process; every side agrees with the P = 0 side of the same launch shapes bit for bit in success, nfact, rho, rho_old and vals, P = 2 also in d of "
             f"both calls, P = 1 and 3 in d within the forward bar (the largest relative difference is printed)",
             "against P = 0 of the same launch shapes: off / side, FASTER or SLOWER only beyond the larger of the two spreads; ** ** marks what is slower",
             "[case] pattern x batch, element type, values, F_s per stage, tasks per stage | side | newton_system | against P = 0 | solve | against P = 0 | d against P = 0"]
    fmt = lambda t: f"{t[0]:9.3f} [{t[1]:9.3f} .. {t[2]:9.3f}]"

    def mark(v):
        return f"**{v.strip()}**" if v.endswith("SLOWER") else v.strip()
    for k in only:
        for f32 in (False, True):
            F32 = f32
            t0 = time.time()
            o = solve_one(torch, hipldl, syn, WIDE_CASES[k])
            head = (f"[{k}] {o['pattern']} x {o['B']}, {'Float32' if f32 else 'Float64'}, {o['values']}{', subtree_ladder = %d (nfact %s)' % (o['rungs'], o['nfact']) if o['rungs'] else ''}, "
                    f"F_s {o['F']}, tasks {o['stage_tasks']}, {o['launches'][0]} launches per newton_system, {o['launches'][1]} per solve")
            lines.append(head)
            n0 = len(lines) - 1
            for sd in o["sides"]:
                P = sd["keys"].get("subtree_solve_panels", 0)
                wide_side = "subtree_wide" in sd["keys"]
                name = f"P = {P}" + (", W = 1, M = 4096" if wide_side else "")
                base = next(q for q in o["sides"] if "subtree_solve_panels" not in q["keys"] and ("subtree_wide" in q["keys"]) == wide_side)
                cmp_ = ["", ""] if not P else [mark(verdict(base[c], sd[c])) for c in ("newton", "solve")]
                lines.append(f"    {name:26s} | {fmt(sd['newton'])} | {cmp_[0]:>18s} | {fmt(sd['solve'])} | {cmp_[1]:>18s} | {sd['agree']:.2e}")
            print("\n".join(lines[n0:]) + f"\n    ({time.time() - t0:.1f} s)", flush=True)
            print(json.dumps(o), file=sys.stderr, flush=True)
            if "--out" in argv:      # (written case by case: what was measured is kept if a later case is not reached)
                with open(argv[argv.index("--out") + 1], "w") as f:
                    f.write("\n".join(lines) + "\n")
    return 0


def verdict(off, on):
    spread = max(off[2] - off[1], on[2] - on[1])
    diff = on[0] - off[0]
    word = "level" if abs(diff) <= spread else ("FASTER" if diff < 0 else "SLOWER")
    return f"{off[0] / on[0]:6.2f}x {word}"


def trace():
    torch, hipldl, syn = setup()
    case = ("grid", (70,), 1, dict(general_blocked=1), "healthy")
    s, runs = make_runs(torch, hipldl, syn, case, keys=(1,))
    r = runs[0]
    assert r["L"].config["general_subtrees"] and r["L"].config["general_blocked"], r["L"].config
    p = hipldl.default_params()
    for _ in range(3):
        hipldl.newton_system_dev(r["L"], r["vals"].data_ptr(), r["rhs"].data_ptr(), r["d"].data_ptr(), r["ro"].data_ptr(), r["rho"].data_ptr(),
                                 r["nf"].data_ptr(), r["su"].data_ptr(), p, 0)
        torch.cuda.synchronize()
    assert int(r["su"].item()) == 1
    print("stage_ptr", r["L"].plan_array("gstage_ptr").tolist(), "ginfo", r["L"].plan_array("ginfo").tolist())
    r["L"].close()
    return 0


def trace_wide(argv):
    W, M, P = (tuple(int(x) for x in argv[argv.index("--trace-wide") + 1].split(",")) + (0,))[:3]
    torch, hipldl, syn = setup()
    case = ("grid", (70,), 1, dict(general_blocked=1), "healthy")
    s, runs = make_runs(torch, hipldl, syn, case, keys=[{k: v for k, v in (("subtree_wide", W), ("subtree_lds_panels", M), ("subtree_solve_panels", P)) if v}])
    r = runs[0]
    assert r["L"].config["general_subtrees"] and r["L"].config["general_blocked"], r["L"].config
    p = hipldl.default_params()
    for _ in range(3):
        hipldl.newton_system_dev(r["L"], r["vals"].data_ptr(), r["rhs"].data_ptr(), r["d"].data_ptr(), r["ro"].data_ptr(), r["rho"].data_ptr(),
                                 r["nf"].data_ptr(), r["su"].data_ptr(), p, 0)
        torch.cuda.synchronize()
    assert int(r["su"].item()) == 1
    if "--with-solve" in argv:      # (three solve_ldl! calls on that factor behind them: 2 S stage launches each)
        for _ in range(3):
            hipldl.solve_dev(r["L"], r["rhs"].data_ptr(), r["d"].data_ptr(), stream=0)
            torch.cuda.synchronize()
    tpp, lds = hipldl.subtree_stage_shape(r["L"])
    print("W", W, "M", M, "P", r["L"].config["subtree_solve_panels"], "stage_ptr", r["L"].plan_array("gstage_ptr").tolist(), "tpp", tpp.tolist(), "lds_bytes", lds.tolist())
    r["L"].close()
    return 0


def main(argv):
    global F32
    if "--trace" in argv:
        return trace()
    if "--trace-wide" in argv:
        return trace_wide(argv)
    if "--wide" in argv:
        return wide(argv)
    if "--solve-panels" in argv:
        return solve_panels(argv)
    if "--dtype" in argv:
        F32 = {"float32": True, "float64": False}[argv[argv.index("--dtype") + 1]]
    if "--ladder" in argv:
        return ladder(argv)
    cases = CASES_F32 if F32 else CASES
    torch, hipldl, syn = setup()
    only = [int(x) for x in argv[argv.index("--only") + 1].split(",")] if "--only" in argv else list(range(len(cases)))
    lines = [f"{'float32_subtrees' if F32 else 'general_subtrees'}: whole-call device time in ms, median [min .. max] of {ROUNDS} alternated rounds after {WARMUP} warm-up rounds, one process",
             "pattern x batch, options, tasks / stages (cap), tpp | call | key off | key on | off/on, beyond the larger spread? | d bit-equal"]
    fmt = lambda t: f"{t[0]:9.3f} [{t[1]:9.3f} .. {t[2]:9.3f}]"
    for k in only:
        t0 = time.time()
        off, on = one(torch, hipldl, syn, cases[k])
        gi = on["ginfo"]
        head = (f"{off['pattern']} x {off['B']}, {'mix, ' if off['values'] == 'mix' else ''}{' '.join(f'{a}={b}' for a, b in off['extra'].items())}, "
                f"{gi[1]} / {gi[2]} ({gi[4]}), tpp {on['tpp']}, on the route: {on['subtrees']}")
        for call in ("newton", "factor", "solve"):
            lines.append(f"[{k}] {head} | {call:6s} | {fmt(off[call])} | {fmt(on[call])} | {verdict(off[call], on[call])} | {on['bit_equal']}")
        print("\n".join(lines[-3:]) + f"\n    ({time.time() - t0:.1f} s)", flush=True)
        print(json.dumps(dict(off=off, on=on)), file=sys.stderr, flush=True)
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
