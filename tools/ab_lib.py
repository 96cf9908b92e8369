#!/usr/bin/env python3
"""A/B of whole-library builds on ONE box (boxes of the pool differ by +-4 %, so only same-box pairs mean anything).
  build (CPU):  python tools/ab_lib.py build <name> <git-ref>|WORK [extra compiler flags]   -> build_abl/ab_<name>/libcannoles_hip.so
  run (GPU):    python tools/ab_lib.py run <B> <name> [<name> ...]    interleaved rounds, kernel ms of the headline step (cfg3 pattern)
  outputs (GPU): python tools/ab_lib.py outputs <name> <name> [...]   one small case per route of the C ABI driver, the three calls of the
                plugin surface each; results saved to build_abl/outputs_<name>.npz and compared bit for bit (exit status 1: they differ)
WORK = the working tree as it is.  The libraries are loaded through CANNOLES_HIP_LIB."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTD = os.path.join(ROOT, "build_abl")


def build(name, ref, flags):
    d = os.path.join(OUTD, "ab_" + name)
    src = os.path.join(d, "src")
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(src)
    if ref == "WORK":
        shutil.copytree(os.path.join(ROOT, "cannoles.jl_amd", "csrc"), os.path.join(src, "cannoles.jl_amd", "csrc"), ignore=shutil.ignore_patterns("build"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(src, "include"))
    else:
        tar = subprocess.run(["git", "-C", ROOT, "archive", ref, "cannoles.jl_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", src], input=tar, check=True)
    csrc = os.path.join(src, "cannoles.jl_amd", "csrc")
    srcs = [f for f in os.listdir(csrc) if f.endswith((".cpp", ".hip"))]
    objs = []
    procs = []
    for f in srcs:
        o = os.path.join(d, f + ".o")
        objs.append(o)
        procs.append(subprocess.Popen(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", *flags, "-c", "-o", o, f], cwd=csrc))
    assert all(p.wait() == 0 for p in procs)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-o", os.path.join(d, "libcannoles_hip.so"), *objs])
    shutil.rmtree(src)
    for o in objs:
        os.remove(o)
    print("built", os.path.join(d, "libcannoles_hip.so"))


RUN = r'''
import sys; sys.path.insert(0, %(root)r)
import numpy as np, torch
import cannoles_jl_amd
from cannoles_jl_amd import hipldl, synthetic as syn
import bench
s = syn.band_structure(%(n)d, %(p)d); rows, cols = s.kkt_pattern()
B = %(B)d
vh, rh = bench.band_batch(s, min(B, 512), 3000)
dev = torch.device("cuda", 0)
rep = max(1, B // 512)
vals = torch.from_numpy(np.tile(vh, (rep, 1))[:B]).to(dev); rhs = torch.from_numpy(np.tile(rh, (rep, 1))[:B]).to(dev)
d = torch.zeros((B, s.N), dtype=torch.float64, device=dev); ro = torch.zeros(B, dtype=torch.float64, device=dev); rho = torch.zeros_like(ro)
nf = torch.zeros(B, dtype=torch.int32, device=dev); su = torch.zeros_like(nf)
L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B)
p = hipldl.default_params()
st = torch.cuda.Stream()
def step():
    hipldl.newton_system_dev(L, vals.data_ptr(), rhs.data_ptr(), d.data_ptr(), ro.data_ptr(), rho.data_ptr(), nf.data_ptr(), su.data_ptr(), p, st.cuda_stream)
with torch.cuda.stream(st):
    for _ in range(3): step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(%(reps)d): step()
    e1.record(st); torch.cuda.synchronize()
print("RESULT %%.5f %%d" %% (e0.elapsed_time(e1) / %(reps)d, int((su == 1).all())))
'''


def run(B, names, n=10000, p=50, rounds=3):
    res = {k: [] for k in names}
    reps = 20 if B >= 1024 else 100
    for r in range(rounds):
        for k in names:
            lib = os.path.join(OUTD, "ab_" + k, "libcannoles_hip.so")
            env = dict(os.environ, CANNOLES_HIP_LIB=lib)
            out = subprocess.run([sys.executable, "-c", RUN % {"root": ROOT, "B": B, "n": n, "p": p, "reps": reps}], env=env, capture_output=True, text=True)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
            if not line:
                # nothing more is started on a device a child may have faulted
                raise SystemExit(f"{k} FAILED (exit status {out.returncode}): {out.stderr[-500:]}")
            ms, ok = line[0].split()[1:]
            res[k].append(float(ms))
            print(f"round {r} {k:12s} B={B} {float(ms):.4f} ms/step  {B / float(ms):.1f} k systems/s ok={ok}", flush=True)
    for k in names:
        if res[k]:
            print(f"{k:12s} min {min(res[k]):.4f} median {sorted(res[k])[len(res[k]) // 2]:.4f} ms")


# The child of `outputs`: the three calls of the plugin surface — try_to_factorize(A), newton_system!(B), solve_ldl!(rhs of A) — on one
# small case per route of the C ABI driver (csrc/call_shape.h, csrc/capi_run.cpp), everything a caller can observe saved to one .npz.
OUT = r'''
import sys; sys.path.insert(0, %(root)r)
import numpy as np, torch
import cannoles_jl_amd
from cannoles_jl_amd import hipldl, synthetic as syn
T, IL = hipldl.PLAN_THROUGHPUT, hipldl.LAYOUT_INTERLEAVED
res = {}

def values(s, B, dtype, ladder, gen):
    if gen is None:
        vA, rA = syn.batch_values(s, B, cfg=4); vB, rB = syn.batch_values(s, B, cfg=3)
        for b in ladder:
            vB[b], rB[b] = syn.band_values(s, 5000 + b, stress="ladder")
    else:
        (vA, rA), (vB, rB) = ([np.stack(x) for x in zip(*[gen(s, 100 * k + b) for b in range(B)])] for k in (1, 2))
        off = s.offsets()
        for b in ladder:
            vB[b, off[0]:off[1]] *= -20.0   # indefinite top-left block
    return [np.ascontiguousarray(x, dtype=dtype) for x in (vA, rA, vB, rB)]

def case(name, s, B, opts=None, dtype=np.float64, ladder=(1,), gen=None, expect=None, dev=False):
    rows, cols = s.kkt_pattern()
    L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=dtype, options=hipldl.Options(**(opts or {})))
    cfg = L.config
    kind = cfg["kernel"] + ("+band" if cfg["band"] else "") + ("+tail" if cfg["tail"] else "") + ("+lean" if cfg["lean"] else "")
    assert expect is None or kind.startswith(expect), (name, kind)
    kind += " " + L.info["order"]
    vA, rA, vB, rB = values(s, B, dtype, ladder, gen)
    p = hipldl.default_params(dtype)
    ro = np.zeros(B, dtype); ro[0] = 1e-3
    c0 = hipldl.launch_counts()
    out = {}
    if dev:   # device entry points (the only ones an interleaved handle has): vals interleaved, everything else problem-major
        g = torch.device("cuda", 0)
        t = lambda a: torch.from_numpy(a).to(g)
        def vin(v):
            tv = t(v)
            if not cfg["batch_layout"]: return tv, tv
            ti = torch.zeros(hipldl.layout_len(L, 0), dtype=tv.dtype, device=g)
            hipldl.interleave_dev(L, 0, tv.data_ptr(), ti.data_ptr(), 0)
            return tv, ti
        (tvA, tinA), (tvB, tinB) = vin(vA), vin(vB)
        su0, su, nf = (torch.zeros(B, dtype=torch.int32, device=g) for _ in range(3))
        d, d2 = (torch.full((B, s.N), 7.0, dtype=tvA.dtype, device=g) for _ in range(2))
        tro, rho, trA, trB = t(ro), t(np.zeros(B, dtype)), t(rA), t(rB)
        hipldl.factorize_dev(L, tinA.data_ptr(), p[0], su0.data_ptr(), 0)
        hipldl.newton_system_dev(L, tinB.data_ptr(), trB.data_ptr(), d.data_ptr(), tro.data_ptr(), rho.data_ptr(), nf.data_ptr(), su.data_ptr(), p, 0)
        hipldl.solve_dev(L, trA.data_ptr(), d2.data_ptr(), 0)
        if cfg["batch_layout"]: hipldl.deinterleave_dev(L, 0, tinB.data_ptr(), tvB.data_ptr(), 0)
        torch.cuda.synchronize()
        out.update(factor_success=su0, d=d, rho_tail=tvB[:, s.nnzNS - s.nvar:], rho=rho, rho_old=tro, nfact=nf, success=su, d_solve=d2)
        out = {k: v.cpu().numpy() for k, v in out.items()}
    else:
        ok0, npos, nzero = hipldl.try_to_factorize(L, vA, s.nvar, s.nequ, s.ncon, p[0], return_inertia=True)
        d, d2 = np.full((B, s.N), 7.0, dtype), np.full((B, s.N), 7.0, dtype)
        _, ok, rho, ro_out, nf = hipldl.newton_system_(d, s.nvar, s.nequ, s.ncon, rB, vB, L, ro, p)
        hipldl.solve_ldl_(rA, L.factor, d2)
        out.update(factor_success=ok0, npos=npos, nzero=nzero, d=d, rho_tail=vB[:, s.nnzNS - s.nvar:], rho=rho, rho_old=ro_out, nfact=nf, success=ok, d_solve=d2)
    c1 = hipldl.launch_counts()
    out["launches"] = np.array([c1[k] - c0[k] for k in sorted(c0)])
    L.close()
    for k, v in out.items():
        res[name + "/" + k] = np.atleast_1d(np.asarray(v))
    print("CASE %%-28s %%-30s nfact max %%d, %%d of %%d succeed, launches %%s" %% (name, kind, int(np.max(out["nfact"])), int(np.sum(out["success"])), B, out["launches"].tolist()), flush=True)

band, small, chain = syn.band_structure(800, 8), syn.band_structure(300, 4), syn.band_structure(300, 4, hw=2)
irr, irr2 = syn.random_structure(200, 260, 0, 0.04, seed=2), syn.random_structure(100, 130, 6, 0.03, 1)
f32g = dict(float32_general=1, band_kernel=0)
case("band_f64", band, 20, dict(plan_kind=T), expect="v2+band")
case("band_f64_interleaved", band, 37, dict(plan_kind=T, batch_layout=IL), expect="v2+band", dev=True)
case("band_f32", band, 20, dict(plan_kind=T), dtype=np.float32, expect="band")
case("f32_general", small, 6, f32g, dtype=np.float32, expect="v1")
case("f32_condense", small, 6, dict(f32g, float32_condense=1), dtype=np.float32, expect="v1")
case("f32_register_front", syn.dense_structure(24, 40), 6, dict(f32g, float32_register_front=1), dtype=np.float32, gen=syn.dense_values, ladder=(), expect="v2")
case("direct_throughput", small, 8, dict(plan_kind=T, band_kernel=0), expect="v2")
case("direct_throughput_dev", small, 8, dict(plan_kind=T, band_kernel=0), expect="v2", dev=True)
case("direct_post_pass", small, 8, dict(plan_kind=T, band_kernel=0, rows_in_backward=0), expect="v2")
case("staged_dataflow", syn.band_structure(2000, 10), 4, None, expect="v2-staged")
case("staged_no_dataflow", syn.band_structure(2000, 10), 4, dict(dataflow=0), expect="v2-staged")
# a batch just above a small staged_max_batch: the chain part + a remainder handle, or two halves (the concurrent form of run_split
# needs more than 4096 problems whatever the tuning: the suite's test_split_* cases hold it)
case("split_tail", chain, 73, dict(staged_max_batch=64, band_kernel=0), ladder=(1, 70), expect="v2-staged+tail")
case("split_halves", chain, 73, dict(staged_max_batch=64, band_kernel=0, split_tail=0), ladder=(1, 70), expect="v2-staged")
case("dense", syn.dense_structure(96, 200), 3, None, gen=syn.dense_values, ladder=(), expect="dense")
case("general_dense", irr, 3, None, gen=syn.random_values, expect="dense")
case("condensed", irr2, 5, dict(general_dense=0), gen=syn.random_values, expect="v1")
case("host_ladder", syn.band_structure(2000, 10), 4, dict(host_ladder=1, device_ladder=0), expect="v2-staged")
case("device_ladder_sequential", syn.band_structure(2000, 10), 4, dict(host_ladder=0, device_ladder=0), expect="v2-staged")
case("device_ladder_fused", syn.band_structure(2000, 10), 4, dict(device_ladder_fused=1), expect="v2-staged")
np.savez(%(out)r, **res)
print("SAVED %%d arrays" %% len(res))
'''


def outputs(names):
    """Every named library in a fresh child process (never two libraries in one process) under a time limit of its own; the first
    failure stops the rest.  Then, on the CPU: every array of every case bit-equal, every count equal, first library against each other."""
    import numpy as np
    for k in names:
        env = dict(os.environ, CANNOLES_HIP_LIB=os.path.join(OUTD, "ab_" + k, "libcannoles_hip.so"))
        out = os.path.join(OUTD, "outputs_" + k + ".npz")
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", OUT % {"root": ROOT, "out": out}], env=env)
        if r.returncode != 0:
            raise SystemExit(f"{k} FAILED (exit status {r.returncode}): nothing more is started")
    ref = np.load(os.path.join(OUTD, "outputs_" + names[0] + ".npz"))
    bad = 0
    for k in names[1:]:
        got = np.load(os.path.join(OUTD, "outputs_" + k + ".npz"))
        assert sorted(ref.files) == sorted(got.files)
        diff = [f for f in ref.files if ref[f].dtype != got[f].dtype or ref[f].tobytes() != got[f].tobytes()]
        bad += len(diff)
        print(f"{names[0]} against {k}: {len(ref.files)} arrays of {len(set(f.split('/')[0] for f in ref.files))} cases, {len(diff)} differ {diff}")
    raise SystemExit(1 if bad else 0)


if __name__ == "__main__":
    if sys.argv[1] == "build":
        build(sys.argv[2], sys.argv[3], sys.argv[4:])
    elif sys.argv[1] == "outputs":
        outputs(sys.argv[2:])
    else:
        a = sys.argv[2:]
        n, p = 10000, 50
        if "--cfg4" in a:
            a.remove("--cfg4"); n, p = 1000, 10
        run(int(a[0]), a[1:], n=n, p=p)
