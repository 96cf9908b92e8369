"""What the tests of the Float32 general-form dense route share (tuning float32_general = 1, float32_general_dense = 1: an irregular
condensed system as ONE dense matrix on the float kernels of csrc/dense_f32.hip) — tests/test_float32_general_dense_cpu.py and
tests/test_float32_general_dense_gpu.py: numpy only.

Inputs: syn.random_structure(n, m, p, density, seed); problem b takes syn.random_values(s, 40 + b) rounded to float32, and a
five-problem mix goes by b % 5 — 0 and 4 healthy, 1 hopeless (H_F = NaN), 2 and 3 indefinite (the H_F segment times -20) climbing the
ladder from rho_old = 0 resp. 2.  The shapes are the smallest at each edge of the kernels the general form runs: order 96 is the
smallest the route takes (two tiles, the second half empty), 128 / 129 the edge of the second tile, 454 the ladder's second pass over
the row tiles and three workgroups of dnf_panel.

Reference, tolerances and the per-call bar are those of tests/support/f32_dense.py (the fp64 oracle on the widened float32 data
with ParamCaNNOLeS(Float32) widened; check_outputs; eig_margins, which is written for any pattern); the CPU test vouches for every
decision of every rung by eigenvalues, so no GPU test skips or reclassifies a problem.

Run as a script (python -m tests.support.f32_general_dense) it runs the two smallest shapes on the device entry and prints one line
of hexadecimal digests per shape: the test of what earlier kernels left behind runs it in child processes and compares the lines."""
import hashlib

import numpy as np

from tests.support import f32_dense as FD
from tests.support import f32_general as G

EPS32, BWD_TOL, FWD_TOL, bits, EIG_MARGIN = G.EPS32, G.BWD_TOL, G.FWD_TOL, G.bits, FD.EIG_MARGIN
check_outputs, eig_margins = FD.check_outputs, FD.eig_margins
MIX = 5
BASE = dict(float32_general=1, float32_condense=1)          # the handle without the key (the key implies float32_condense)
OPTIONS = dict(float32_general=1, float32_general_dense=1)

# (n, m, p, density, seed): (condensed order, largest front of the condensed throughput plan) — what the shape is there for
SHAPES = {
    (96, 120, 0, 0.06, 1): (96, 96),      # smallest order the route takes; T = 2, half-empty last tile
    (92, 110, 4, 0.08, 2): (96, 97),      # the same with constraint pivots in the last tile
    (128, 150, 0, 0.06, 3): (128, 128),   # two full tiles
    (125, 140, 4, 0.06, 4): (129, 126),   # one real row in the third tile, and it is a -delta pivot
    (129, 150, 0, 0.06, 5): (129, 130),   # one real variable row in the third tile
    (450, 300, 4, 0.02, 1): (454, 375),   # (= dense_cases.GENERAL) T = 8: second pass of the ladder, three dnf_panel workgroups
}
SMALLEST = (96, 120, 0, 0.06, 1)
NOT_TAKEN = (60, 80, 4, 0.1, 1)           # condensed order 64, largest front 63
WANT_OK = [True, False, True, True, True]
WANT_NF = [1, 10, 5, 4, 1]
# the plan cnl_create_f32_ex builds for such a handle, as Plan options (the library forces the same switches internally)
COND_PLAN = dict(plan_kind=1, condense=1, register_front=0, dense_backend=0, general_dense=0, staged=0, band_kernel=0)


def shape_id(shape):
    return "n%d-m%d-p%d-d%g-s%d" % shape


def structure(shape):
    from cannoles_jl_amd import synthetic as syn
    n, m, p, dens, seed = shape
    return syn.random_structure(n, m, p, dens, seed=seed)


def values(s, B):
    """(vals, rhs, rho_old) of B problems, float32"""
    from cannoles_jl_amd import synthetic as syn
    off = s.offsets()
    vals, rhs, ro = np.zeros((B, s.nnzNS)), np.zeros((B, s.N)), np.zeros(B)
    for b in range(B):
        vals[b], rhs[b] = syn.random_values(s, 40 + b)
        kind = b % 5
        if kind == 1:
            vals[b, off[0]:off[1]] = np.nan
        elif kind in (2, 3):
            vals[b, off[0]:off[1]] *= -20.0
            if kind == 3:
                ro[b] = 2.0
    return tuple(np.ascontiguousarray(a, np.float32) for a in (vals, rhs, ro))


_cache = {}


def case(shape, B=MIX):
    """The float32 case and what the fp64 oracle makes of it, computed once per session and shared (read-only): the dict of
    tests/support/f32_dense.py: case."""
    key = (shape, B)
    if key not in _cache:
        from oracle import oracle as O
        s = structure(shape)
        rows, cols = s.kkt_pattern()
        vals, rhs, ro = values(s, B)
        p32 = FD.params32()
        orc = O.Oracle(s.N, rows, cols, O.canonical_perm(s.nvar, s.nequ, s.ncon))
        va = vals.astype(np.float64)
        d, ok, rho, rold, nf = O.newton_system_batch(orc, B, s.nvar, s.nequ, s.ncon, rhs.astype(np.float64), va, ro.astype(np.float64),
                                                     p32.astype(np.float64))
        c = dict(s=s, rows=rows, cols=cols, vals=vals, rhs=rhs, rho_old=ro, p32=p32, d=d, ok=np.asarray(ok, bool), rho=rho, ro=rold,
                 nf=np.asarray(nf, np.int64), vals_after=va)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def handle(hipldl, c, B, options=OPTIONS, **opt):
    s = c["s"]
    return hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32,
                               options=hipldl.Options(**options, **opt))


def on_the_route(L):
    return L.config["kernel"] == "dense" and L.config["float32"] and not L.config["band"] and L.info["ncond"] > 0


class Args:
    """one argument set of cnl_newton_system_f32_dev on the device"""

    def __init__(self, s, B):
        import torch
        dev = torch.device("cuda:0")
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self.vals, self.rhs, self.d = torch.zeros((B, s.nnzNS), **f32), torch.zeros((B, s.N), **f32), torch.zeros((B, s.N), **f32)
        self.ro, self.rho = torch.zeros(B, **f32), torch.zeros(B, **f32)
        self.nf, self.ok = torch.zeros(B, **i32), torch.zeros(B, **i32)

    def fill(self, vals, rhs, ro):
        import torch
        self.vals.copy_(torch.from_numpy(np.array(vals)))   # (copies: the shared cases are read-only)
        self.rhs.copy_(torch.from_numpy(np.array(rhs)))
        self.ro.copy_(torch.from_numpy(np.array(ro)))
        self.d.fill_(7.0)
        self.rho.fill_(-1.0)
        self.nf.fill_(-1)
        self.ok.fill_(-1)
        torch.cuda.synchronize()

    def call(self, hipldl, L, p):
        import torch
        hipldl.newton_system_dev(L, self.vals, self.rhs, self.d, self.ro, self.rho, self.nf, self.ok, p,
                                 stream=torch.cuda.current_stream().cuda_stream)

    def read(self):
        import torch
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("vals", "d", "ro", "rho", "nf", "ok")}


def main():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl
    for shape in ((96, 120, 0, 0.06, 1), (92, 110, 4, 0.08, 2)):
        s = structure(shape)
        rows, cols = s.kkt_pattern()
        vals, rhs, ro = values(s, MIX)
        L = handle(hipldl, dict(s=s, rows=rows, cols=cols), MIX)
        assert on_the_route(L), L.config
        A = Args(s, MIX)
        A.fill(vals, rhs, ro)
        A.call(hipldl, L, FD.params32())
        out = A.read()
        L.close()
        print(shape_id(shape), " ".join(hashlib.sha256(np.ascontiguousarray(out[k]).tobytes()).hexdigest()[:16] for k in sorted(out)))
    print("done")


if __name__ == "__main__":
    main()
