"""What the tests of the blocked general kernel in float share (tuning float32_blocked: csrc/kernels.hip, eliminate_blocked and
panel_trailing_update instantiated for float) — tests/test_float32_blocked_cpu.py and tests/test_float32_blocked_gpu.py: numpy only.

Nothing is invented here.  Shapes: those of tests/support/general_blocked_cases.py (GB: RANDOM_N, COND0, GRID, F130, G450) and the two
order-96 shapes of tests/support/f32_general_dense.py (GD).  Values and reference: the Float32 five-kind mix of GD (`values`, the fp64
oracle on the widened float data with ParamCaNNOLeS(Float32) widened, `check_outputs`, `eig_margins`); tolerances BWD_TOL, FWD_TOL
and MARGIN of tests/support/f32_general.py.  `case` is GD.case for any shape GB.structure knows (GD.case itself takes
random_structure tuples only, and the grid is none).

SEEDS: the structure seed of every shape, the one the shape tables name — every (shape, problem, rung) of them has the project's
margin in float (tests/test_float32_blocked_cpu.py: test_pivot_margins), so none had to move to the next seed.

The algorithm: `eliminate_blocked_f32` restates the kernel's blocked elimination of one packed front in numpy.float32 with the
trailing update done as the kernel does it — tile by tile, 64 lanes, operands and accumulator placed by the lane maps of
v_mfma_f32_16x16x4_f32, the instruction itself emulated by `mfma_f32_16x16x4` with the hardware's maps."""
import numpy as np

from tests.support import f32_dense as FD
from tests.support import f32_general as G
from tests.support import f32_general_dense as GD
from tests.support import general_blocked_cases as GB
from tests.support.plan_sim import tri

EPS32, BWD_TOL, FWD_TOL, MARGIN, bits = G.EPS32, G.BWD_TOL, G.FWD_TOL, G.MARGIN, G.bits
check_outputs, eig_margins, MIX = GD.check_outputs, GD.eig_margins, GD.MIX
PANEL = GB.PANEL
WANT_OK, WANT_NF = GD.WANT_OK, GD.WANT_NF

KEY = dict(float32_blocked=1)
COND = dict(float32_general=1, float32_condense=1)       # the float32_condense handle
UNCOND = dict(float32_general=1)                          # the uncondensed Float32 general handle
FORCED = dict(v1_tpp=256, v1_ppb=1)                      # the configuration with a blocked instance, where the default is 64 threads

RANDOM_N, COND0, GRID, F130, G450 = GB.RANDOM_N, GB.COND0, GB.GRID, GB.F130, GB.G450
F97 = (92, 110, 4, 0.08, 2)          # GD: condensed order 96, largest front 97
F96 = GD.SMALLEST                    # (96, 120, 0, 0.06, 1): largest front 96 -> 64 threads per problem, no blocked instance
random_shape, shape_id, structure = GB.random_shape, GB.shape_id, GB.structure
# the structure seed in use, by shape (see the module docstring): the tables' own
SEEDS = {shape_id(sh): sh[-1] for sh in [random_shape(n) for n in RANDOM_N] + [COND0, F130, G450, F97, F96]}
SEEDS[shape_id(GRID)] = None         # (the grid has no seed)

# (shape, handle options, plan options of that handle): every handle the GPU tests make under the key
GPU_CASES = [(random_shape(n), COND, GD.COND_PLAN) for n in RANDOM_N] + [
    (COND0, UNCOND, G.GENERAL_PLAN), (GRID, COND, GD.COND_PLAN), (GRID, UNCOND, G.GENERAL_PLAN),
    (F97, COND, GD.COND_PLAN), (F130, COND, GD.COND_PLAN), (G450, COND, GD.COND_PLAN), (F96, COND, GD.COND_PLAN),
    (random_shape(33), UNCOND, G.GENERAL_PLAN)]
# largest front of the Float32 plan, and the threads per problem choose_config takes from it (fmax <= 96: 64)
FMAX = {(shape_id(random_shape(n)), True): n + 1 for n in RANDOM_N}
FMAX.update({(shape_id(COND0), False): 61, (shape_id(GRID), True): 95, (shape_id(GRID), False): 95, (shape_id(F97), True): 97,
             (shape_id(F130), True): 130, (shape_id(G450), True): 375, (shape_id(F96), True): 96, (shape_id(random_shape(33)), False): 64})


def make_plan(shape, plan_opts, B=MIX):
    """the plan cnl_create_f32_ex builds for a Float32 general handle on `shape` (plan_opts: GD.COND_PLAN or G.GENERAL_PLAN)"""
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl
    s = structure(shape)
    rows, cols = s.kkt_pattern()
    return s, hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=B, options=hipldl.Options(**plan_opts))


_cache = {}


def case(shape, B=MIX):
    """GD.case on any shape of GB.structure: the float32 mix (problem b of kind b % 5) and what the fp64 oracle makes of the widened
    data, computed once per session and shared read-only"""
    key = (shape, B)
    if key not in _cache:
        from oracle import oracle as O
        s = structure(shape)
        rows, cols = s.kkt_pattern()
        vals, rhs, ro = GD.values(s, B)
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


def handle(hipldl, c, B, **opt):
    s = c["s"]
    return hipldl.HIPLDLStruct(s.N, c["rows"], c["cols"], None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32, options=hipldl.Options(**opt))


# ---- the algorithm ----
LANES = np.arange(64)
LI, LG = LANES & 15, LANES >> 4


def row_f32(lg, r):
    """result register r of a lane of group lg = l >> 4 holds row 4 lg + r (column l & 15): v_mfma_f32_16x16x4_f32"""
    return 4 * lg + r


def row_f64(lg, r):
    """... row lg + 4 r: v_mfma_f64_16x16x4_f64 — the WRONG map for the float instruction"""
    return lg + 4 * r


def mfma_f32_16x16x4(a, b, c):
    """D = C + A B as v_mfma_f32_16x16x4_f32 lays it out over 64 lanes: a[l] = A[l & 15][l >> 4], b[l] = B[l >> 4][l & 15], c[r][l] and
    the result d[r][l] = element (4 (l >> 4) + r, l & 15).  float32, the four products added one after the other."""
    A = np.zeros((16, 4), np.float32)
    Bm = np.zeros((4, 16), np.float32)
    A[LI, LG] = a
    Bm[LG, LI] = b
    d = np.array(c, np.float32)
    for r in range(4):
        rows = row_f32(LG, r)
        acc = d[r]
        for k in range(4):
            acc = (acc + A[rows, k] * Bm[k, LI]).astype(np.float32)
        d[r] = acc
    return d


def panel_trailing_update_f32(F, W, p0, kp, lim, row=row_f32):
    """panel_trailing_update of csrc/kernels.hip on one wavefront: every 16 x 16 tile of the packed triangle below lim, operands and
    zeros selected lane by lane, the accumulator loaded from F and stored back through `row`, four instructions on two chains"""
    nt = (lim + PANEL - 1) // PANEL
    zero = np.float32(0)
    for ta in range(nt):
        for tb in range(ta + 1):
            ar, bc = PANEL * ta + LI, PANEL * tb + LI
            aop, bop = [], []
            for s in range(4):
                k = 4 * s + LG
                ka = np.minimum(k, kp - 1)
                va, vb = (k < kp) & (ar < lim), (k < kp) & (bc < lim)
                aop.append(np.where(va, -F[tri(p0 + ka) + np.minimum(ar, lim - 1)], zero).astype(np.float32))
                bop.append(np.where(vb, W[ka, np.minimum(bc, lim - 1)], zero).astype(np.float32))
            acc = np.zeros((4, 64), np.float32)
            keep = np.zeros((4, 64), bool)
            pos = np.zeros((4, 64), np.int64)
            for r in range(4):
                a = PANEL * ta + row(LG, r)
                keep[r] = (a < lim) & (bc <= a)
                pos[r] = np.where(keep[r], tri(np.minimum(a, lim - 1)) + np.minimum(bc, a), 0)
                acc[r] = np.where(keep[r], F[pos[r]], zero)
            acc2 = np.zeros((4, 64), np.float32)
            acc = mfma_f32_16x16x4(aop[0], bop[0], acc)
            acc2 = mfma_f32_16x16x4(aop[1], bop[1], acc2)
            acc = mfma_f32_16x16x4(aop[2], bop[2], acc)
            acc2 = mfma_f32_16x16x4(aop[3], bop[3], acc2)
            out = (acc + acc2).astype(np.float32)
            F[pos[keep]] = out[keep]


def eliminate_blocked_f32(F, f, nupd, indep, eig_tol, row=row_f32):
    """GB.eliminate_blocked in numpy.float32 on a packed front (float32 array, changed in place and returned with the counts), the
    trailing update of every panel by panel_trailing_update_f32; `row`: the result map the load and the store of the accumulator use
    (row_f32 is the kernel's; row_f64 shows what copying the double code would compute)"""
    assert F.dtype == np.float32
    eig_tol = np.float32(eig_tol)
    idep = f - indep
    npos = nzer = 0
    p1 = f
    with np.errstate(all="ignore"):
        while p1 > nupd + 1:
            ind = p1 > idep
            floor = idep if ind else nupd + 1
            p0 = max(p1 - PANEL, floor)
            kp = p1 - p0
            lim = idep if ind else p0
            W = np.zeros((kp, max(lim, 1)), np.float32)
            for k in (range(kp) if ind else range(kp - 1, -1, -1)):
                i = p0 + k
                rowi = F[tri(i):tri(i) + i + 1]
                dp = rowi[i]
                npos += dp > eig_tol
                nzer += abs(dp) <= eig_tol
                n = lim if ind else i
                w = rowi[:n].copy()
                l = (w / dp).astype(np.float32)
                rowi[:n] = l
                W[k, :lim] = w[:lim]
                if not ind:
                    for a in range(p0, i):
                        F[tri(a):tri(a) + a + 1] -= (l[a] * w[:a + 1]).astype(np.float32)
            panel_trailing_update_f32(F, W, p0, kp, lim, row)
            p1 = p0
    return F, int(npos), int(nzer)
