"""The per-stage launch shapes of subtree handles (tuning subtree_wide = W, subtree_lds_panels = M), without a GPU:
the keys' rules at the four creators, the ABI, the stage rule restated in numpy from the plan's arrays, the bounds that keep the LDS
areas of the LPAN instances from being overrun — on every shape the GPU tests run and on grid_structure(48) and (70) —, and that the
keys change no plan."""
import os
import re

import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl
from tests.support import subtree_wide_cases as SW

GS, FS = SW.GS, SW.FS
CNL_ERR_ARG = 1
f32, f64 = np.float32, np.float64
ARRAYS = ("fronts", "inner_perm", "perm", "seg_ptr", "asm_pos", "asm_src", "child_idx", "rel_idx", "gtasks", "gstage_ptr", "gfronts", "ginfo")
F64_ON = dict(general_subtrees=1, general_blocked=1)
F32_ON = dict(float32_general=1, float32_subtrees=1, float32_blocked=1)


def _rc(make):
    try:
        obj = make()
    except hipldl.CnlError as e:
        return e.code, str(e)
    if hasattr(obj, "close"):
        obj.close()
    return 0, ""


def _creators(s):
    """the four creators as functions of (options) -> (code, message); `f32` says which element type's keys the creator reads"""
    rows, cols = s.kkt_pattern()
    args = (s.N, rows, cols)
    return {
        "cnl_create_ex": (False, lambda **o: _rc(lambda: hipldl.HIPLDLStruct(*args, None, s.nvar, s.nequ, s.ncon, batch=7, dtype=f64, options=hipldl.Options(**o)))),
        "cnl_create_f32_ex": (True, lambda **o: _rc(lambda: hipldl.HIPLDLStruct(*args, None, s.nvar, s.nequ, s.ncon, batch=7, dtype=f32, options=hipldl.Options(**o)))),
        "cnl_plan_create_ex": (False, lambda **o: _rc(lambda: hipldl.Plan(*args, s.nvar, s.nequ, s.ncon, batch=7, options=hipldl.Options(**o)))),
        "cnl_multi_create_ex": (False, lambda **o: _rc(lambda: hipldl.MultiHIPLDLStruct(*args, s.nvar, s.nequ, s.ncon, 7, [0], options=hipldl.Options(**o)))),
    }


# ---- 1. the keys' rules, decided before a device is looked for ----
def test_version_and_symbol(built):
    assert hipldl.lib().cnl_version() >= 509
    assert "cnl_subtree_stage_shape" in hipldl.ABI_SYMBOLS
    assert hasattr(hipldl.lib(), "cnl_subtree_stage_shape")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cannoles_hip.h")).read()
    assert re.search(r"\bint\s+cnl_subtree_stage_shape\s*\(\s*const\s+cnl_handle\s*\*\s*h\s*,\s*int32_t\s*\*\s*tpp\s*,\s*int32_t\s*\*\s*lds_bytes\s*,\s*int64_t\s*\*\s*nstages\s*\)\s*;", header)


@pytest.mark.parametrize("creator", ("cnl_create_ex", "cnl_create_f32_ex", "cnl_plan_create_ex", "cnl_multi_create_ex"))
def test_key_rules_without_a_device(built, creator):
    s = GS.structure(GS.FOREST3)
    is32, make = _creators(s)[creator]
    on = F32_ON if is32 else F64_ON
    sub = "float32_subtrees" if is32 else "general_subtrees"
    blk = "float32_blocked" if is32 else "general_blocked"
    # accepted: every value of the range's ends, alone and together (a machine without a device gets as far as looking for one)
    for keys in (dict(subtree_wide=0, subtree_lds_panels=0), dict(subtree_wide=1), dict(subtree_wide=4096), dict(subtree_lds_panels=16),
                 dict(subtree_lds_panels=4096), dict(subtree_wide=96, subtree_lds_panels=128)):
        rc, msg = make(**dict(on, **keys))
        assert rc != CNL_ERR_ARG and (rc == 0 or "no HIP device" in msg), (keys, rc, msg)
    rc, msg = make(**{k: v for k, v in dict(on, subtree_wide=5).items() if k != blk})      # W needs no blocked key
    assert rc != CNL_ERR_ARG, (rc, msg)
    # out of range
    for keys in (dict(subtree_wide=-1), dict(subtree_wide=4097), dict(subtree_lds_panels=-1), dict(subtree_lds_panels=1), dict(subtree_lds_panels=15),
                 dict(subtree_lds_panels=4097)):
        rc, msg = make(**dict(on, **keys))
        assert rc == CNL_ERR_ARG and list(keys)[0] in msg, (keys, rc, msg)
    # the creator's own subtree key off: absent, written out as 0
    for keys in (dict(subtree_wide=1), dict(subtree_lds_panels=64)):
        for off in ({k: v for k, v in on.items() if k != sub}, dict(on, **{sub: 0})):
            rc, msg = make(**dict(off, **keys))
            assert rc == CNL_ERR_ARG and "subtree" in msg, (keys, off, rc, msg)
    # subtree_lds_panels without the creator's blocked key
    for off in ({k: v for k, v in on.items() if k != blk}, dict(on, **{blk: 0})):
        rc, msg = make(**dict(off, subtree_lds_panels=64))
        assert rc == CNL_ERR_ARG and "subtree_lds_panels" in msg and "blocked" in msg, (off, rc, msg)
    # together with float32_refine
    for keys in (dict(subtree_wide=1), dict(subtree_lds_panels=64)):
        for base in (dict(float32_general=1, float32_subtrees=1, float32_blocked=1), dict(float32_general=1, general_subtrees=1, general_blocked=1)):
            rc, msg = make(**dict(base, float32_refine=1, **keys))
            assert rc == CNL_ERR_ARG, (keys, base, rc, msg)


def test_the_other_element_types_keys_do_not_count(built):
    """a Float64 creator with the Float32 subtree / blocked keys alone, and the reverse"""
    s = GS.structure(GS.FOREST3)
    c = _creators(s)
    for name in ("cnl_create_ex", "cnl_multi_create_ex"):
        for keys in (dict(subtree_wide=1), dict(subtree_lds_panels=64)):
            rc, msg = c[name][1](**dict(F32_ON, **keys))
            assert rc == CNL_ERR_ARG and "general_subtrees" in msg, (name, rc, msg)
        rc, msg = c[name][1](general_subtrees=1, float32_general=1, float32_blocked=1, subtree_lds_panels=64)
        assert rc == CNL_ERR_ARG and "general_blocked" in msg, (name, rc, msg)
    rc, msg = c["cnl_create_f32_ex"][1](float32_general=1, float32_subtrees=1, subtree_lds_panels=64)
    assert rc == CNL_ERR_ARG and "float32_blocked" in msg, (rc, msg)


# ---- 2. the stage rule and the LDS bounds ----
def _plans():
    for shape in SW.CPU_SHAPES:
        caps = (4, 8) if shape in (GS.GRID12, GS.FOREST3) else (8,)
        for cap in caps:
            yield shape, dict(task_cap=cap, general_blocked=1), GS.make_plan(shape, task_cap=cap, general_blocked=1)[1]
    yield GS.GRID32, dict(condense=0, general_blocked=1), GS.make_plan(GS.GRID32, condense=0, general_blocked=1)[1]
    for shape, cond in ((GS.GRID12, True), (GS.GRID32, False), (GS.FOREST4, False)):
        yield shape, dict(float32=True, cond=cond), FS.make_plan(shape, cond, 8, blocked=1)[1]


@pytest.fixture(scope="module")
def plans(built):
    return list(_plans())


def test_lds_areas_cannot_be_overrun(plans):
    """For every front of every stage, every dependent panel's piece of the packed triangle fits 16 F_s elements — and 16 times the
    staging stride of its own task, which is where the kernel puts the second area —, ws <= F_s, and need_s is what the formula says."""
    seen = 0
    for shape, opt, plan in plans:
        F, tasks, has = SW.stage_table(plan)
        piece, ws, per_panel = SW.panel_bounds(plan)
        assert (piece <= SW.PANEL_W * F).all() and (ws <= F).all(), (shape, opt)
        assert all(p <= SW.PANEL_W * w for p, w in per_panel), (shape, opt)
        assert (has >= (piece > 0)).all()      # (a stage with a dependent panel has a front of 16 pivots; not the reverse: independent pivots)
        for esz in (4, 8):
            need = SW.need_bytes(F, esz)
            assert np.array_equal(need, (16 + 32 * F) * esz)
            # [red 16 | rows 16 ws | unscaled rows 16 ws] ends inside need_s for every task of the stage
            assert ((16 + 2 * SW.PANEL_W * ws) * esz <= need).all()
        seen += len(per_panel)
    assert seen > 100


def test_grid70_is_the_issues_table(built):
    """the eight fronts of the last three stages of grid_structure(70) at task_cap 8 on the throughput plan"""
    s, plan = GS.make_plan(SW.GRID70, task_cap=8)
    t, sp, g, gi = GS.cut_of(plan)
    S = len(sp) - 1
    fronts = lambda st: sorted((int(g["npiv"][f]), int(g["nupd"][f])) for k in range(sp[st], sp[st + 1]) for f in range(t["f0"][k], t["f1"][k]))
    assert fronts(S - 1) == [(207, 0)]
    assert fronts(S - 2) == sorted([(69, 139), (47, 139), (47, 138)])
    assert fronts(S - 3) == sorted([(49, 140), (47, 139), (20, 139), (33, 96)])
    F, tasks, has = SW.stage_table(plan)
    assert F[-1] == 208 and has[-3:].all() and tasks[-3:].tolist() == [4, 3, 1]


def test_stage_rule_in_numpy(plans):
    """the rule on hand-made tables, and its monotonicity on the plans: W = 1 widens every stage a small batch allows, a W above every F_s
    none, M = 4096 gives LPAN to every stage with a panel that fits, an M below every F_s to none, and the batch bound is per stage"""
    table = (np.array([10, 64, 208]), np.array([101, 3, 1]), np.array([False, True, True]))
    tpp, lds = SW.stage_rule(table, 256, True, 8, W=64, M=100, batch=1, cus=256)
    assert tpp.tolist() == [256, 1024, 1024] and lds.tolist() == [128, (16 + 32 * 64) * 8, 128]
    tpp, lds = SW.stage_rule(table, 256, True, 8, W=1, M=4096, batch=6, cus=256)        # 101 x 6 > 512 >= 3 x 6
    assert tpp.tolist() == [256, 1024, 1024] and lds.tolist() == [128, (16 + 32 * 64) * 8, (16 + 32 * 208) * 8]
    tpp, lds = SW.stage_rule(table, 256, True, 8, W=1, M=4096, batch=5, cus=256)        # 101 x 5 <= 512
    assert tpp.tolist() == [1024, 1024, 1024]
    tpp, lds = SW.stage_rule(table, 1024, False, 4, W=1, M=4096, batch=1, cus=256)      # neither key acts
    assert tpp.tolist() == [1024] * 3 and lds.tolist() == [64] * 3
    big = (np.array([700]), np.array([1]), np.array([True]))
    assert SW.stage_rule(big, 256, True, 8, W=0, M=4096, batch=1, cus=256)[1].tolist() == [128]       # 179 KB: no LPAN
    assert SW.stage_rule(big, 256, True, 4, W=0, M=4096, batch=1, cus=256)[1].tolist() == [(16 + 32 * 700) * 4]
    assert SW.stage_rule(big, 256, True, 4, W=0, M=4096, batch=1, cus=256, lds_cap=65536)[1].tolist() == [64]
    for shape, opt, plan in plans:
        tb = SW.stage_table(plan)
        F, tasks, has = tb
        esz = 4 if opt.get("float32") else 8
        tpp, lds = SW.stage_rule(tb, 256, True, esz, W=1, M=4096, batch=1, cus=256)
        assert (tpp == np.where(tasks <= 512, 1024, 256)).all() and ((lds > 16 * esz) == (has & (SW.need_bytes(F, esz) <= SW.LDS_CAP))).all()
        tpp, lds = SW.stage_rule(tb, 256, True, esz, W=int(F.max()) + 1, M=16, batch=1, cus=256)
        assert (tpp == 256).all() and (lds == 16 * esz).all() and F[has].min() > 16      # (a front of 16 pivots and its rhs row: F_s >= 18)
        tpp, _ = SW.stage_rule(tb, 256, True, esz, W=int(F[-1]), M=0, batch=1, cus=256)
        assert tpp[-1] == 1024 and (tpp == np.where(F >= F[-1], 1024, 256)).all()


# ---- 3. the keys change no plan ----
@pytest.mark.parametrize("shape,opt", [(GS.GRID12, dict(task_cap=4, general_blocked=1)), (GS.GRID32, dict(condense=0, general_blocked=1)),
                                       (GS.FOREST3, dict(general_blocked=1))], ids=("grid12-cap4", "grid32-uncondensed", "forest3"))
def test_the_keys_change_no_plan(built, shape, opt):
    s, off = GS.make_plan(shape, **opt)
    for keys in (dict(subtree_wide=1), dict(subtree_lds_panels=4096), dict(subtree_wide=64, subtree_lds_panels=64)):
        s, on = GS.make_plan(shape, **dict(opt, **keys))
        assert on.info == off.info
        for name in ARRAYS:
            assert np.array_equal(on.array(name), off.array(name)), (keys, name)
    assert len(off.array("gtasks")) > 0
