"""What the tests of the general kernel's subtree execution in float share (tuning float32_subtrees: csrc/kernels.hip — newton_subtrees
instantiated for float —, csrc/capi_handle.cpp — setup_subtrees) — tests/test_float32_subtrees_cpu.py and
tests/test_float32_subtrees_gpu.py: numpy only.

Nothing is invented here.  Shapes: those of tests/support/general_subtrees_cases.py (GS: GRID12, GRID16, GRID32, FOREST3, FOREST4,
CHAIN).  Values and reference: the Float32 five-kind mix of tests/support/f32_general_dense.py and the fp64 oracle on the widened float
data with ParamCaNNOLeS(Float32) widened, as tests/support/f32_blocked_cases.py builds it (`case`); `oracle_on` is the same oracle on
the plan's own elimination order.  Bars: BWD_TOL, FWD_TOL and MARGIN of tests/support/f32_general.py.

The forced analysis of a Float32 general handle is the throughput analysis with the switches of GD.COND_PLAN (float32_condense) or
G.GENERAL_PLAN (uncondensed); with float32_subtrees it also asks for the cut, and with float32_blocked on top for 16 staging rows per
task region.  `plan_options` spells that as Plan options (general_subtrees, general_blocked), so that the CPU tests see the plan the
creator builds; the GPU tests compare the handle's own ginfo with it.

SubtreeSimF32 is GS.SubtreeSim with every store rounded to float32, between the float condensation passes of
tests/support/plan_sim_f32_cond.py where the plan is condensed."""
import numpy as np

from tests.support import f32_blocked_cases as FB
from tests.support import f32_general as G
from tests.support import f32_general_dense as GD
from tests.support import general_subtrees_cases as GS
from tests.support.plan_sim_f32 import PlanSimF32
from tests.support.plan_sim_f32_cond import PlanSimF32Cond

F32 = np.float32
EPS32, BWD_TOL, FWD_TOL, MARGIN, bits = G.EPS32, G.BWD_TOL, G.FWD_TOL, G.MARGIN, G.bits
check_outputs, eig_margins, MIX = GD.check_outputs, GD.eig_margins, GD.MIX
WANT_OK, WANT_NF = GD.WANT_OK, GD.WANT_NF
GRID12, GRID16, GRID32, FOREST3, FOREST4, CHAIN = GS.GRID12, GS.GRID16, GS.GRID32, GS.FOREST3, GS.FOREST4, GS.CHAIN
SHAPES = (GRID12, GRID16, GRID32, FOREST3, FOREST4, CHAIN)
shape_id, structure, case, handle = GS.shape_id, GS.structure, FB.case, FB.handle

KEY = dict(float32_subtrees=1)
COND, UNCOND, FORCED = FB.COND, FB.UNCOND, FB.FORCED      # the two handles the key acts on; v1_tpp = 256, v1_ppb = 1
MEMORY_BOUND = 8e9      # bytes of task regions of the whole batch
ESZ = 4

# the cut of the forced float plans: (shape, condensed, cap) -> (tasks, stages, tasks of the first stage)
CUT = {
    (GRID12, True, 4): (12, 4, 7), (GRID12, True, 8): (6, 3, 4), (GRID12, False, 4): (24, 6, 13), (GRID12, False, 8): (16, 5, 9),
    (GRID16, True, 4): (24, 6, 13), (GRID16, True, 8): (14, 5, 8), (GRID16, False, 4): (43, 8, 23), (GRID16, False, 8): (26, 6, 14),
    (FOREST3, True, 4): (7, 2, 6), (FOREST3, True, 8): (3, 1, 3), (FOREST3, False, 4): (12, 3, 10), (FOREST3, False, 8): (7, 2, 6),
    (FOREST4, True, 4): (14, 4, 11), (FOREST4, True, 8): (12, 3, 10), (FOREST4, False, 8): (21, 4, 17),
    (GRID32, True, 8): (50, 6, 26), (GRID32, False, 8): (97, 7, 54),
    (CHAIN, True, 8): (31, 9, 18),
}
# largest front of those plans (condensed, uncondensed); CHAIN alone is above order 96: 256 threads per problem by itself
FMAX = {GRID12: (34, 34), GRID16: (52, 52), FOREST3: (23, 28), FOREST4: (40, 58), GRID32: (95, 95), CHAIN: (375, None)}


def plan_options(cond, cap, blocked=0, subtrees=1):
    """the forced analysis of the Float32 general handle (float32_condense or not) with float32_subtrees / float32_blocked, as Plan options"""
    return dict(GD.COND_PLAN if cond else G.GENERAL_PLAN, general_subtrees=subtrees, task_cap=cap, general_blocked=1 if blocked and subtrees else 0)


def make_plan(shape, cond, cap, blocked=0, subtrees=1, B=MIX):
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl
    s = structure(shape)
    rows, cols = s.kkt_pattern()
    return s, hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=B, options=hipldl.Options(**plan_options(cond, cap, blocked, subtrees)))


def ginfo(plan_or_handle):
    a = plan_or_handle.plan_array("ginfo") if hasattr(plan_or_handle, "plan_array") else plan_or_handle.array("ginfo")
    return [int(x) for x in a]


def takes_the_route(plan, batch, tpp, ppb=1, general_kernel=True):
    """the rule of DESIGN section 9.11 on the host, for a Float32 general handle: (a) the launch is the general kernel in float,
    (b) one problem per workgroup of 256 threads, (c) two tasks or more in the first stage, (d) batch x gwork x 4 <= 8e9 bytes"""
    gi = plan.array("ginfo")
    if len(gi) == 0:
        return False
    gwork, ntasks, nstages, first = (int(x) for x in gi[:4])
    return bool(general_kernel) and ppb == 1 and tpp == 256 and first >= 2 and batch * gwork * ESZ <= MEMORY_BOUND


_own = {}


def oracle_on(perm, c):
    """the case with the oracle's results on the elimination order `perm` (the handle's) in place of those on the canonical order"""
    from oracle import oracle as O
    s = c["s"]
    perm = np.asarray(perm, np.int64)
    if np.array_equal(perm, O.canonical_perm(s.nvar, s.nequ, s.ncon)):
        return c
    key = (id(c), perm.tobytes())
    if key not in _own:
        B = len(c["vals"])
        orc = O.Oracle(s.N, c["rows"], c["cols"], perm)
        va = c["vals"].astype(np.float64)
        d, ok, rho, rold, nf = O.newton_system_batch(orc, B, s.nvar, s.nequ, s.ncon, c["rhs"].astype(np.float64), va, c["rho_old"].astype(np.float64),
                                                     c["p32"].astype(np.float64))
        _own[key] = dict(c, d=d, ok=np.asarray(ok, bool), rho=rho, ro=rold, nf=np.asarray(nf, np.int64), vals_after=va)
    return _own[key]


class SubtreeSimF32(GS.SubtreeSim):
    """GS.SubtreeSim in numpy.float32: the work area (NaN until written), the factor panels, the solution stack and d are float32
    arrays, so every product, quotient and sum of _forward_front is a float32 operation; the backward sweep is PlanSimF32's, task by
    task.  newton_system is PlanSimF32's ladder on an uncondensed plan and PlanSimF32Cond's — float condense, cond_inertia, expand
    around it — on a condensed one."""

    def __init__(self, plan, reverse=False, rows=2, check_writes=True):
        super().__init__(plan, reverse=reverse, rows=rows, check_writes=check_writes)
        if self.ncond:
            self.nslot = len(self.c_ptr) - 1
            self.c_len = np.diff(self.c_ptr)

    condense, cond_inertia, expand = PlanSimF32Cond.condense, PlanSimF32Cond.cond_inertia, PlanSimF32Cond.expand

    def factor(self, vals, rhs, nvar, eig_tol, rho=None):
        t = self.tasks
        eig_tol = F32(eig_tol)
        W = np.full(self.gwork, np.nan, F32)
        L = np.full(self.info["lsize"], np.nan, F32)
        src_all = np.concatenate([np.asarray(vals, F32), np.zeros(self.N, F32) if rhs is None else np.asarray(rhs, F32)])
        if rho is not None:
            src_all[self.nnz - nvar:self.nnz] = F32(rho)
        slots = np.zeros((self.ntasks, 2), np.int64)
        self.trace = []
        for k in self.order():
            lo, hi = self.region(k)
            assert hi <= self.gwork and np.isnan(W[lo:hi]).all(), f"task {k}: its region was written before it ran"
            before = W.copy() if self.check_writes else None
            for s in range(t["f0"][k], t["f1"][k]):
                slots[k] += self._forward_front(s, W, L, src_all, eig_tol)
            if self.check_writes:
                same = (before == W) | (np.isnan(before) & np.isnan(W))
                same[lo:hi] = True
                assert same.all(), f"task {k} wrote outside its region at {np.flatnonzero(~same)[:4]}"
            self.trace.append(k)
        assert W.dtype == F32 and L.dtype == F32
        self.W = W
        return L, int(slots[:, 0].sum()), int(slots[:, 1].sum())

    def backward(self, L):
        f, t = self.fr, self.tasks
        assert L.dtype == F32
        X = np.full(self.gwork, np.nan, F32)
        d = np.zeros(self.N, F32)
        for k in self.order(backward=True):
            for s in range(t["f1"][k] - 1, t["f0"][k] - 1, -1):
                nupd, npiv = f["nupd"][s], f["npiv"][s]
                fs = 1 + nupd + npiv
                tu = GS.tri(1 + nupd)
                panel = L[self.lptr[s]:self.lptr[s] + GS.tri(fs) - tu]
                xo = f["xoff"][s]
                if f["parent"][s] >= 0:
                    rel = self.rel_idx[f["rel_begin"][s]:f["rel_begin"][s] + 1 + nupd]
                    xp = f["xoff"][f["parent"][s]]
                    X[xo + 1:xo + 1 + nupd] = X[xp + rel[1:]].copy()
                for i in range(nupd + 1, fs):
                    row = panel[GS.tri(i) - tu:GS.tri(i) - tu + i + 1]
                    acc = F32(0)
                    for j in range(1, i):   # float32 products and sums, one after the other (PlanSimF32.backward)
                        acc = F32(acc + F32(row[j] * X[xo + j]))
                    xi = F32(row[0] - acc)
                    X[xo + i] = xi
                    d[self.perm[f["first_piv"][s] + (fs - 1 - i)]] = -xi
        return d

    def newton_system(self, vals, rhs, nvar, nequ, ncon, rho_old, params):
        if self.ncond:
            return PlanSimF32Cond.newton_system(self, vals, rhs, nvar, nequ, ncon, rho_old, params)
        return PlanSimF32.newton_system(self, vals, rhs, nvar, nequ, ncon, rho_old, params)


def classic_sim(plan):
    """PlanSim in float32 on the classic table of the same plan"""
    from tests.support.plan_sim import PlanSim
    probe = PlanSim(plan)
    return PlanSimF32Cond(plan) if probe.ncond else PlanSimF32(plan)
