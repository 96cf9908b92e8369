"""What the tests of the blocked general kernel share (tuning general_blocked: csrc/kernels.hip, eliminate_blocked and
panel_trailing_update) — tests/test_general_blocked_cpu.py and tests/test_general_blocked_gpu.py: numpy only.

Shapes.  A shape is a random_structure tuple (n, m, p, density, seed) or ("grid", G) for synthetic.grid_structure(G); OPTS are the
options every case runs under (no dense route, no register-front kernel, no dense backend: the general kernel serves the handle).
RANDOM_N: one front of n pivots each, n = 16 k - 1, 16 k, 16 k + 1 around one, two and three panels.  COND0: the uncondensed
handle of (33, 40, 4), whose last front has 60 pivots of which the leading 23 are independent (the J'WJ product).  GRID: fronts with
update rows, of which the uncondensed plan adds some with independent pivots.  F130, G125, G450, BIG: the LDS / global scratch and the
256 / 1024 thread instances at their default configuration.

Values and reference: the seven-kind mix of tests/support/dense_general_cases.py and the CPU oracle, as there.

The algorithm: `eliminate_blocked` restates the kernel's blocked elimination of one packed front in numpy, `eliminate_rank1` is
the loop of tests/support/plan_sim.py; BlockedSim walks a plan as PlanSim.factor does, with either."""
import numpy as np

from tests.support import dense_general_cases as GC
from tests.support.plan_sim import PlanSim, tri

PANEL = 16
OPTS = dict(general_blocked=1, general_dense=0, register_front=0, dense_backend=0)
RANDOM_N = (16, 17, 31, 32, 33, 47, 48, 49)
COND0 = (33, 40, 4, 0.3, 1)
GRID = ("grid", 32)
GRID48 = ("grid", 48)
GRID_BATCH = 8192          # the batch the grid plans are made for (the large-batch analysis)
F130 = (129, 150, 0, 0.06, 5)
G125 = (125, 140, 4, 0.06, 4)
G450 = (450, 300, 4, 0.02, 1)


def random_shape(n):
    return (n, n + 10, 0, 0.3, 1)


def shape_id(shape):
    return f"grid{shape[1]}" if shape[0] == "grid" else "n%d-m%d-p%d-s%d" % (shape[0], shape[1], shape[2], shape[4])


def structure(shape):
    from cannoles_jl_amd import synthetic as syn
    if shape[0] == "grid":
        return syn.grid_structure(shape[1])
    return GC.structure(shape)


def plan_batch(shape, B):
    return GRID_BATCH if shape[0] == "grid" else B


# the fronts (npiv, nupd, indep) the GPU tests rely on: shape, extra options -> fronts that must be in the plan
FRONT_TABLE = [(random_shape(n), {}, [(n, 0, None)]) for n in RANDOM_N] + [
    (COND0, dict(condense=0), [(60, 0, 23)]),
    (GRID, {}, [(21, 62, 0), (31, 63, 0), (93, 0, 0)]),
    (GRID, dict(condense=0), [(21, 62, 0), (31, 63, 0), (93, 0, 0), (16, 13, 11), (15, 27, 9)]),
    (G450, {}, [(19, 355, 0), (356, 0, 0)]),
]


def make_plan(shape, B=GC.MIX, **extra):
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl
    s = structure(shape)
    rows, cols = s.kkt_pattern()
    return s, hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=plan_batch(shape, B), options=hipldl.Options(**dict(OPTS, **extra)))


def fronts_of(plan):
    fr = plan.array("fronts").reshape(-1, 16)
    return [(int(f[0]), int(f[1]), int(f[14])) for f in fr]


_cache = {}


def case(shape, B=GC.MIX, kinds=None):
    """the mix (or the problems of `kinds`) on a shape and the oracle's results on the canonical order, shared and read-only"""
    kinds = tuple(range(B)) if kinds is None else tuple(kinds)
    key = ("blocked", shape, kinds)
    if key not in _cache:
        from cannoles_jl_amd import synthetic as syn
        from oracle import oracle as O
        s = structure(shape)
        n = len(kinds)
        vals, rhs, ro = np.zeros((n, s.nnzNS)), np.zeros((n, s.N)), np.zeros(n)
        for k, b in enumerate(kinds):
            vals[k], rhs[k] = syn.random_values(s, 40 + b)
            ro[k] = GC.apply_kind(s, vals[k], b % GC.MIX)
        _cache[key] = GC._oracle_case(key, s, vals, rhs, ro, O.default_params(), np.array(kinds) % GC.MIX)
    return _cache[key]


# ---- the algorithm ----
def eliminate_rank1(F, f, nupd, indep, eig_tol):
    """the pivot-by-pivot loop of PlanSim.factor on one packed front, in place; returns (npos, nzer)"""
    ti, tj = np.tril_indices(f)
    idep = f - indep
    npos = nzer = 0
    for i in range(f - 1, nupd, -1):
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
            F[:tul] -= l[ti[:tul]] * w[tj[:tul]]
    return int(npos), int(nzer)


def eliminate_blocked(F, f, nupd, indep, eig_tol, panel=PANEL):
    """The blocked elimination: panels of `panel` pivots from the highest local index down.  The leading `indep` pivots form panels
    of their own (no step inside the panel, trailing triangle up to idep); a dependent panel [p0, p1) runs its pivots one by one —
    pivot read, counted, row kept unscaled in W and scaled in place, rank-1 update of the rows p0 .. i - 1 only — and then
    F[a][b] -= sum_k L[k][a] W[k][b] for b <= a < p0.  The last panel of either kind is as narrow as it comes."""
    idep = f - indep
    npos = nzer = 0
    p1 = f
    with np.errstate(all="ignore"):
        while p1 > nupd + 1:
            ind = p1 > idep
            floor = idep if ind else nupd + 1
            p0 = max(p1 - panel, floor)
            kp = p1 - p0
            lim = idep if ind else p0
            W, Lk = np.zeros((kp, lim)), np.zeros((kp, lim))
            for k in (range(kp) if ind else range(kp - 1, -1, -1)):
                i = p0 + k
                row = F[tri(i):tri(i) + i + 1]
                dp = row[i]
                npos += dp > eig_tol
                nzer += abs(dp) <= eig_tol
                n = lim if ind else i
                w = row[:n].copy()
                l = w / dp
                row[:n] = l
                W[k], Lk[k] = w[:lim], l[:lim]
                if not ind:
                    for a in range(p0, i):
                        F[tri(a):tri(a) + a + 1] -= l[a] * w[:a + 1]
            ti, tj = np.tril_indices(lim)
            F[:tri(lim)] -= (Lk.T @ W)[ti, tj]
            p1 = p0
    return int(npos), int(nzer)


class BlockedSim(PlanSim):
    """PlanSim whose factor() eliminates fronts of at least PANEL pivots with eliminate_blocked (blocked=True), or every front with
    eliminate_rank1; `on_front(s, F_before, F_after, counts)` sees every front."""

    def factor_with(self, vals, rhs, nvar, eig_tol, rho=None, blocked=True, on_front=None):
        f = self.fr
        W = np.full(self.info["fwd_peak"] + 8, np.nan)
        L = np.full(self.info["lsize"], np.nan)
        src_all = np.concatenate([np.asarray(vals, float), np.zeros(self.N) if rhs is None else np.asarray(rhs, float)])
        if rho is not None:
            src_all[self.nnz - nvar:self.nnz] = rho
        npos = nzer = 0
        for s in range(self.ns):
            nupd, npiv = int(f["nupd"][s]), int(f["npiv"][s])
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
                rel = self.rel_idx[f["rel_begin"][c]:f["rel_begin"][c] + 1 + nu]
                F[tri(rel[self.ti[:tuc]]) + rel[self.tj[:tuc]]] += W[f["ubase"][c]:f["ubase"][c] + tuc]
            before = F.copy() if on_front else None
            elim = eliminate_blocked if blocked and npiv >= PANEL else eliminate_rank1
            cnt = elim(F, fs, nupd, int(f["indep"][s]), eig_tol)
            if on_front:
                on_front(s, before, F, cnt)
            npos += cnt[0]
            nzer += cnt[1]
            L[self.lptr[s]:self.lptr[s] + tf - tu] = F[tu:tf]
            if f["ubase"][s] != f["foff"][s]:
                W[f["ubase"][s]:f["ubase"][s] + tu] = F[:tu].copy()
        return L, int(npos), int(nzer)

    def inner_inputs(self, vals, rhs):
        """(vals, rhs) of the system the fronts work on: the condensed buffer's two parts where the plan condenses"""
        if not self.ncond:
            return np.asarray(vals, float), np.asarray(rhs, float)
        cb = self.condense(vals, rhs)
        nmat = len(cb) - self.N
        return cb[:nmat].copy(), cb[nmat:]
