"""What the tests of the general kernel's subtree execution share (tuning general_subtrees: csrc/analysis.cpp — the cut and the task
regions —, csrc/kernels.hip — newton_subtrees) — tests/test_general_subtrees_cpu.py and tests/test_general_subtrees_gpu.py: numpy only.

Shapes, the smallest that still have the structure: grid_structure(12), (16) and (32) on the large-batch plan (general_blocked_cases:
GRID_BATCH), and two forests — random_structure(120, 130, 0, 0.01, 1) with four roots, (40, 50, 0, 0.03, 2) with three.  CHAIN is
the chain-like tree of the measurements.  OPTS are the options every case runs under: no dense route, no register-front kernel, no
dense backend, so that the general kernel serves the handle; the thread count and the cap come with the case.

Values and reference: the seven-kind mix of tests/support/dense_general_cases.py and the CPU oracle, as in general_blocked_cases.

SubtreeSim is PlanSim on the plan's SECOND front table, run TASK BY TASK as the device runs it: the tasks of a stage one after the
other (forwards or reversed — they are independent), every stage behind the one before; the work area is one array of gwork
elements that starts as NaN everywhere, so that a task that reads what no earlier task wrote — a region of a task that has not
run, or a stale piece of its own — poisons its result; a task that writes outside its own region is caught at once."""
import numpy as np

from tests.support import dense_general_cases as GC
from tests.support import general_blocked_cases as GB
from tests.support.plan_sim import HDR, PlanSim, tri

OPTS = dict(general_subtrees=1, general_dense=0, register_front=0, dense_backend=0)
GRID12, GRID16, GRID32 = ("grid", 12), ("grid", 16), ("grid", 32)
FOREST4 = (120, 130, 0, 0.01, 1)
FOREST3 = (40, 50, 0, 0.03, 2)
CHAIN = (450, 300, 4, 0.02, 1)
SHAPES = (GRID12, GRID16, GRID32, FOREST4, FOREST3)
GTASK = ["stage", "f0", "f1", "parent", "base", "pb_off", "wv_off", "fmax"]      # csrc/plan.h: struct GTask
MOVED = ("foff", "ubase", "xoff")                                                # what gfronts may differ from fronts in
# the issue's table of the cut at cap 8: shape -> (tasks, stages)
CUT_CAP8 = {GRID12: (6, 3), GRID16: (14, 5), GRID32: (50, 6)}
MEMORY_BOUND = 8e9      # bytes of task regions of the whole batch (the bound of the dense batch rule)

shape_id, structure = GB.shape_id, GB.structure


def options(**extra):
    return dict(OPTS, **extra)


def make_plan(shape, B=GC.MIX, **extra):
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl
    s = structure(shape)
    rows, cols = s.kkt_pattern()
    if shape[0] == "grid":
        extra = dict(dict(plan_kind=hipldl.PLAN_THROUGHPUT), **extra)
    return s, hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=GB.plan_batch(shape, B), options=hipldl.Options(**options(**extra)))


def cut_of(plan):
    """(tasks as a dict of int64 columns, stage_ptr, gfronts as a dict of columns, ginfo)"""
    t = plan.array("gtasks").reshape(-1, 8)
    g = plan.array("gfronts").reshape(-1, 16)
    return ({k: t[:, i].astype(np.int64) for i, k in enumerate(GTASK)}, plan.array("gstage_ptr").astype(np.int64),
            {k: g[:, i].astype(np.int64) for i, k in enumerate(HDR)}, plan.array("ginfo").astype(np.int64))


def case(shape, B=GC.MIX, kinds=None):
    """the mix on a shape and the oracle's results on the canonical order (general_blocked_cases.case: shared, read-only)"""
    return GB.case(shape, B=B, kinds=kinds)


def takes_the_route(plan, batch, tpp, ppb=1):
    """the documented rule on the host, for a Float64 handle whose launch is the general kernel"""
    gi = plan.array("ginfo")
    if len(gi) == 0:
        return False
    gwork, ntasks, nstages, first = (int(x) for x in gi[:4])
    return ppb == 1 and tpp in (256, 1024) and first >= 2 and batch * gwork * 8 <= MEMORY_BOUND


class SubtreeSim(PlanSim):
    """PlanSim.factor / .backward over gfronts, task by task.  reverse: the tasks of every stage in reversed order.  rows: staging
    rows of a region (2, or 16 under general_blocked).  factor() checks, per task, that nothing outside the task's region changed."""

    def __init__(self, plan, reverse=False, rows=2, check_writes=True):
        super().__init__(plan)
        self.tasks, self.stage_ptr, self.fr, gi = cut_of(plan)
        self.gwork = int(gi[0])
        self.reverse, self.rows, self.check_writes = reverse, rows, check_writes
        self.lptr = self.fr["lptr_lo"] | (self.fr["lptr_hi"] << 31)
        self.ntasks = len(self.tasks["f0"])
        self.trace = []      # the tasks in the order they ran (forward passes)

    def region(self, k):
        t = self.tasks
        return int(t["base"][k]), int(t["wv_off"][k] + self.rows * t["fmax"][k])

    def order(self, backward=False):
        nst = len(self.stage_ptr) - 1
        for st in (range(nst - 1, -1, -1) if backward else range(nst)):
            ks = list(range(self.stage_ptr[st], self.stage_ptr[st + 1]))
            for k in (ks[::-1] if self.reverse else ks):
                yield k

    def _forward_front(self, s, W, L, src_all, eig_tol):
        """PlanSim.factor's loop body, operation for operation"""
        f = self.fr
        nupd, npiv = f["nupd"][s], f["npiv"][s]
        fs = 1 + nupd + npiv
        tf, tu = tri(fs), tri(1 + nupd)
        F = W[f["foff"][s]:f["foff"][s] + tf]
        F[:] = 0.0
        for r in range(f["seg_begin"][s], f["seg_end"][s]):
            e0, e1 = self.seg_ptr[r], self.seg_ptr[r + 1]
            F[self.asm_pos[e0:e1]] += src_all[self.asm_src[e0:e1]]
        for c in self.child_idx[f["child_begin"][s]:f["child_end"][s]]:
            nu = f["nupd"][c]
            tuc = tri(1 + nu)
            U = W[f["ubase"][c]:f["ubase"][c] + tuc]
            rel = self.rel_idx[f["rel_begin"][c]:f["rel_begin"][c] + 1 + nu]
            F[tri(rel[self.ti[:tuc]]) + rel[self.tj[:tuc]]] += U
        idep = fs - f["indep"][s]
        npos = nzer = 0
        for i in range(fs - 1, nupd, -1):
            ulim = idep if i >= idep else i
            row = F[tri(i):tri(i) + i + 1]
            dp = row[i]
            npos += dp > eig_tol
            nzer += abs(dp) <= eig_tol
            w = row[:ulim].copy()
            with np.errstate(all="ignore"):
                l = w / dp
            row[:ulim] = l
            tul = tri(ulim)
            with np.errstate(all="ignore"):
                F[:tul] -= l[self.ti[:tul]] * w[self.tj[:tul]]
        L[self.lptr[s]:self.lptr[s] + tf - tu] = F[tu:tf]
        if f["ubase"][s] != f["foff"][s]:
            W[f["ubase"][s]:f["ubase"][s] + tu] = F[:tu].copy()
        return int(npos), int(nzer)

    def factor(self, vals, rhs, nvar, eig_tol, rho=None):
        t = self.tasks
        W = np.full(self.gwork, np.nan)
        L = np.full(self.info["lsize"], np.nan)
        src_all = np.concatenate([np.asarray(vals, float), np.zeros(self.N) if rhs is None else np.asarray(rhs, float)])
        if rho is not None:
            src_all[self.nnz - nvar:self.nnz] = rho
        slots = np.zeros((self.ntasks, 2), np.int64)      # a slot per task, summed behind the last stage (the decide kernel)
        self.trace = []
        for k in self.order():
            lo, hi = self.region(k)
            assert np.isnan(W[lo:hi]).all(), f"task {k}: its region was written before it ran"
            before = W.copy() if self.check_writes else None
            for s in range(t["f0"][k], t["f1"][k]):
                slots[k] += self._forward_front(s, W, L, src_all, eig_tol)
            if self.check_writes:
                same = (before == W) | (np.isnan(before) & np.isnan(W))
                same[lo:hi] = True
                assert same.all(), f"task {k} wrote outside its region at {np.flatnonzero(~same)[:4]}"
            self.trace.append(k)
        self.W = W
        return L, int(slots[:, 0].sum()), int(slots[:, 1].sum())

    def backward(self, L):
        f, t = self.fr, self.tasks
        X = np.full(self.gwork, np.nan)
        d = np.zeros(self.N)
        for k in self.order(backward=True):
            for s in range(t["f1"][k] - 1, t["f0"][k] - 1, -1):
                nupd, npiv = f["nupd"][s], f["npiv"][s]
                fs = 1 + nupd + npiv
                tu = tri(1 + nupd)
                panel = L[self.lptr[s]:self.lptr[s] + tri(fs) - tu]
                xo = f["xoff"][s]
                if f["parent"][s] >= 0:
                    rel = self.rel_idx[f["rel_begin"][s]:f["rel_begin"][s] + 1 + nupd]
                    xp = f["xoff"][f["parent"][s]]
                    X[xo + 1:xo + 1 + nupd] = X[xp + rel[1:]].copy()
                for i in range(nupd + 1, fs):
                    row = panel[tri(i) - tu:tri(i) - tu + i + 1]
                    xi = row[0] - np.dot(row[1:i], X[xo + 1:xo + i])
                    X[xo + i] = xi
                    d[self.perm[f["first_piv"][s] + (fs - 1 - i)]] = -xi
        return d
