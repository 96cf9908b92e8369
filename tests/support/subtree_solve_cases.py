"""What the tests of the panelled solve sweeps of subtree handles share (tuning subtree_solve_panels = P, DESIGN section 3.5:
csrc/kernels.hip — subtree_solve_kernel, front_backward_panels, front_forward_solve_panels —, csrc/capi_handle.cpp — setup_subtrees —,
csrc/capi_run.cpp — launch_subtrees) — tests/test_subtree_solve_cpu.py and tests/test_subtree_solve_gpu.py: numpy only.

Nothing is invented here.  Shapes, mixes, oracles and bars are those of tests/support/general_subtrees_cases.py (GS),
tests/support/f32_subtrees_cases.py (FS) and tests/support/subtree_wide_cases.py (SW).  Restated from the plan's arrays alone:
    the panel cut    panels of PANEL_W = 16 consecutive pivot rows of a front with rows 0 (right-hand side), 1 .. nupd (update rows),
                     nupd + 1 .. f - 1 (pivots): ASCENDING from nupd + 1 in the backward sweep, DESCENDING from f in the forward
                     substitution, the last panel of either as short as it comes
    the LDS need     of a panelled launch of stage s, in elements of the handle's type, with F_s the largest GTask.fmax of the stage:
                       [ vec: round4(F_s) | tri: 16 rows of stride 17 = 272 | pv: 16 ]   need_s = round4(F_s) + 288
                     vec holds the front's X (backward) or F (forward): rows 0 .. f - 1; tri the panel's triangle, element (k, r) at
                     17 k + r for r <= k < 16; pv the panel's 16 values (t_r backward, w_k forward).  Every carve offset is a
                     multiple of 4 elements: 16 bytes in float, 32 in double.  A stage runs panelled where
                     need_s x sizeof(T) <= min(the device's LDS per workgroup, 160 KB)."""
import numpy as np

from tests.support import f32_subtrees_cases as FS
from tests.support import general_subtrees_cases as GS
from tests.support import subtree_wide_cases as SW

PANEL_W = SW.PANEL_W
TRI_LD = PANEL_W + 1
TRI = PANEL_W * TRI_LD
LDS_CAP = SW.LDS_CAP
GPU_SHAPES = SW.GPU_SHAPES
CHAIN = GS.CHAIN
CPU_SHAPES = SW.CPU_SHAPES
CAP = {GS.GRID12: 4, GS.FOREST3: 4}      # task_cap by shape (8 elsewhere): the cuts of the existing subtree tests
MASKS = (0, 1, 2, 3)


def key_options(P=0):
    return {"subtree_solve_panels": P} if P else {}


def vec_elems(F):
    return (np.asarray(F, np.int64) + 3) & ~np.int64(3)


def carve(F):
    """element offsets (vec, tri, pv, end) of the dynamic LDS of a panelled launch of a stage with largest task fmax F"""
    v = int(vec_elems(F))
    return 0, v, v + TRI, v + TRI + PANEL_W


def need_bytes(F, esz):
    return (vec_elems(F) + TRI + PANEL_W) * esz


def stage_lds(table, esz, P, lds_cap=LDS_CAP):
    """dynamic LDS bytes of the panelled launches per stage (0: the stage keeps the unpanelled launch), for a handle with mask P"""
    F, tasks, has = table
    need = need_bytes(F, esz)
    return np.where((P > 0) & (need <= min(lds_cap, LDS_CAP)), need, 0).astype(np.int64)


def backward_panels(npiv, nupd):
    """[p0, p1) in the order the backward sweep runs them"""
    f = 1 + nupd + npiv
    return [(p0, min(p0 + PANEL_W, f)) for p0 in range(nupd + 1, f, PANEL_W)]


def forward_panels(npiv, nupd):
    """[p0, p1) in the order the forward substitution runs them"""
    out, p1 = [], 1 + nupd + npiv
    while p1 > nupd + 1:
        p0 = max(p1 - PANEL_W, nupd + 1)
        out.append((p0, p1))
        p1 = p0
    return out


def fronts_by_stage(src):
    """per stage the fronts of its tasks as (npiv, nupd, indep, fmax of the task)"""
    get = src.plan_array if hasattr(src, "plan_array") else src.array
    t = get("gtasks").reshape(-1, 8).astype(np.int64)
    g = get("gfronts").reshape(-1, 16).astype(np.int64)
    S = int(t[:, 0].max()) + 1
    out = [[] for _ in range(S)]
    for stage, f0, f1, fmax in zip(t[:, 0], t[:, 1], t[:, 2], t[:, 7]):
        out[stage] += [(int(a), int(b), int(c), int(fmax)) for a, b, c in zip(g[f0:f1, 0], g[f0:f1, 1], g[f0:f1, 14])]
    return out


def touched(npiv, nupd):
    """the largest element index each area of the LDS is touched at by the sweeps of one front: (vec, tri, pv)"""
    f = 1 + nupd + npiv
    tri = pv = -1
    for cut in (backward_panels(npiv, nupd), forward_panels(npiv, nupd)):
        for p0, p1 in cut:
            kp = p1 - p0
            tri = max(tri, (kp - 1) * TRI_LD + (kp - 1))      # (the forward triangle keeps its diagonal)
            pv = max(pv, kp - 1)
    return f - 1, tri, pv


# ---- the two sweeps of one front in numpy, unpanelled (front_forward with WITH_K = false, front_backward) and in panels ----
def forward_unpanelled(L, z, nupd, indep):
    """L: f x f lower triangle (row i, columns 0 .. i; column 0 unused), z: the front's vector F; returns (F, the z_i stored)"""
    F, f = z.copy(), len(z)
    idep = f - indep
    out = np.zeros(f, z.dtype)
    for i in range(f - 1, nupd, -1):
        ulim = idep if i >= idep else i
        w = F[i]
        for j in range(1, ulim):
            F[j] = F[j] - L[i, j] * w
        out[i] = w / L[i, i]
    return F, out


def forward_panelled(L, z, nupd, indep):
    F, f = z.copy(), len(z)
    idep = f - indep
    out = np.zeros(f, z.dtype)
    for p0, p1 in forward_panels(f - 1 - nupd, nupd):
        v = F[p0:p1].copy()
        w = np.zeros(p1 - p0, z.dtype)
        for k in range(p1 - p0 - 1, -1, -1):      # inner part: the panel's pivots on F[p0 .. p1)
            i = p0 + k
            ulim = idep if i >= idep else i
            w[k] = v[k]
            for r in range(k):
                if p0 + r < ulim:
                    v[r] = v[r] - L[i, p0 + r] * w[k]
            out[i] = w[k] / L[i, i]
        for j in range(1, p0):                     # outer part: every element below the panel, the panel's pivots descending
            for k in range(p1 - p0 - 1, -1, -1):
                i = p0 + k
                if j < (idep if i >= idep else i):
                    F[j] = F[j] - L[i, j] * w[k]
    return F, out


def backward_unpanelled(L, x, nupd):
    """x: rows 1 .. nupd hold the parent's entries; returns X"""
    X, f = x.copy(), len(x)
    for i in range(nupd + 1, f):
        X[i] = L[i, 0] - sum(L[i, j] * X[j] for j in range(1, i))
    return X


def backward_panelled(L, x, nupd, lanes=16):
    X, f = x.copy(), len(x)
    for p0, p1 in backward_panels(f - 1 - nupd, nupd):
        t = np.zeros(p1 - p0, x.dtype)
        for r in range(p1 - p0):                   # outer part: lanes stride over j, then the butterfly of the lane group
            part = np.zeros(lanes, x.dtype)
            for j in range(1, p0):
                part[(j - 1) % lanes] += L[p0 + r, j] * X[j]
            o = lanes // 2
            while o:
                part = part + part[np.arange(lanes) ^ o]
                o //= 2
            t[r] = L[p0 + r, 0] - part[0]
        for k in range(p1 - p0):                   # inner part
            for r in range(k + 1, p1 - p0):
                t[r] = t[r] - L[p0 + r, p0 + k] * t[k]
        X[p0:p1] = t
    return X
