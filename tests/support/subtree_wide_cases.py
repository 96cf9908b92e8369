"""What the tests of the per-stage launch shapes of subtree handles share (tuning subtree_wide = W and subtree_lds_panels = M, DESIGN
section 3.4: csrc/capi_handle.cpp — setup_subtrees, subtree_stage_shape —, csrc/capi_run.cpp — launch_subtrees —, csrc/kernels.hip — the
LPAN instances of eliminate_blocked) — tests/test_subtree_wide_cpu.py and tests/test_subtree_wide_gpu.py: numpy only.

Nothing is invented here.  Shapes, mixes, oracles and bars are those of tests/support/general_subtrees_cases.py (GS) and
tests/support/f32_subtrees_cases.py (FS).  The stage rule is restated from the plan's arrays alone ("gtasks", "gstage_ptr", "gfronts"):
    F_s        the largest GTask.fmax (word 7 of a task record) of the tasks of stage s
    wide       the handle has 256 threads per workgroup, W > 0, F_s >= W and tasks_s x batch <= 2 x CUs
    LPAN       the handle is blocked, M > 0, F_s <= M, the stage has a front with at least PANEL_W pivots, and
               need_s = (16 + 32 F_s) x sizeof(T) <= min(the device's LDS per workgroup, 160 KB)
`dependent_panels` walks the panels of one front as eliminate_blocked cuts them and yields the dependent ones."""
import numpy as np

from tests.support import f32_subtrees_cases as FS
from tests.support import general_subtrees_cases as GS
from tests.support.plan_sim import tri

PANEL_W = 16
LDS_CAP = 160 * 1024
GRID48, GRID70 = ("grid", 48), ("grid", 70)
GPU_SHAPES = (GS.GRID12, GS.GRID16, GS.GRID32, GS.FOREST4, GS.FOREST3)
CPU_SHAPES = GPU_SHAPES + (GRID48, GRID70)


def stage_table(src):
    """(F_s, tasks_s, has_panel_s), one entry per stage, from a Plan or a handle"""
    get = src.plan_array if hasattr(src, "plan_array") else src.array
    t = get("gtasks").reshape(-1, 8).astype(np.int64)
    sp = get("gstage_ptr").astype(np.int64)
    g = get("gfronts").reshape(-1, 16).astype(np.int64)
    S = len(sp) - 1
    F, has = np.zeros(S, np.int64), np.zeros(S, bool)
    for stage, f0, f1, fmax in zip(t[:, 0], t[:, 1], t[:, 2], t[:, 7]):
        F[stage] = max(F[stage], fmax)
        has[stage] |= bool((g[f0:f1, 0] >= PANEL_W).any())
    assert all((t[sp[s]:sp[s + 1], 0] == s).all() for s in range(S))
    return F, np.diff(sp), has


def need_bytes(F, esz):
    return (16 + 32 * np.asarray(F, np.int64)) * esz


def stage_rule(table, tpp, blocked, esz, W, M, batch, cus, lds_cap=LDS_CAP):
    """(threads per workgroup, dynamic LDS bytes) of the factorising forward launch of every stage"""
    F, tasks, has = table
    wide = (tpp == 256) & (W > 0) & (F >= W) & (tasks * batch <= 2 * cus)
    need = need_bytes(F, esz)
    lpan = bool(blocked) & (M > 0) & (F <= M) & has & (need <= min(lds_cap, LDS_CAP))
    return np.where(wide, 1024, tpp).astype(np.int32), np.where(lpan, need, 16 * esz).astype(np.int32)


def dependent_panels(npiv, nupd, indep):
    """the dependent panels [p0, p1) of a front with at least PANEL_W pivots, in the order eliminate_blocked runs them"""
    f = 1 + nupd + npiv
    idep = f - indep
    p1 = f
    while p1 > nupd + 1:
        ind = p1 > idep
        floor = idep if ind else nupd + 1
        p0 = max(p1 - PANEL_W, floor)
        if not ind:
            yield p0, p1
        p1 = p0


def panel_bounds(src):
    """per stage: the largest LDS piece tri(p1) - tri(p0) of a dependent panel, and the largest staging stride ws of a task with one"""
    get = src.plan_array if hasattr(src, "plan_array") else src.array
    t = get("gtasks").reshape(-1, 8).astype(np.int64)
    g = get("gfronts").reshape(-1, 16).astype(np.int64)
    S = int(t[:, 0].max()) + 1
    piece, ws, ws_task = np.zeros(S, np.int64), np.zeros(S, np.int64), []
    for stage, f0, f1, fmax in zip(t[:, 0], t[:, 1], t[:, 2], t[:, 7]):
        for npiv, nupd, indep in zip(g[f0:f1, 0], g[f0:f1, 1], g[f0:f1, 14]):
            assert 1 + nupd + npiv <= fmax
            if npiv < PANEL_W:
                continue
            for p0, p1 in dependent_panels(int(npiv), int(nupd), int(indep)):
                assert 0 < p1 - p0 <= PANEL_W and p1 <= fmax
                piece[stage] = max(piece[stage], tri(p1) - tri(p0))
                ws[stage] = max(ws[stage], fmax)
                ws_task.append((tri(p1) - tri(p0), int(fmax)))
    return piece, ws, ws_task


def key_options(W=0, M=0):
    return {k: v for k, v in (("subtree_wide", W), ("subtree_lds_panels", M)) if v}
