"""The panelled solve sweeps of subtree handles (tuning subtree_solve_panels = P, a bit mask 0 .. 3), without a
GPU: the key's rules at the four creators, the ABI version, that the key changes no plan, the panel cut restated in numpy, the
per-stage LDS formula on the plans of every shape the GPU tests run and on grid_structure(48) and (70), and the two sweeps of a front
in numpy — the panelled forward substitution is the unpanelled one operation for operation, the panelled backward sweep another order
of the same sums.  Every test needs a library that knows the key (the `key_known` fixture)."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl
from tests.support import subtree_solve_cases as SP

GS, FS, SW = SP.GS, SP.FS, SP.SW
CNL_ERR_ARG = 1
f32, f64 = np.float32, np.float64
ARRAYS = ("fronts", "inner_perm", "perm", "seg_ptr", "asm_pos", "asm_src", "child_idx", "rel_idx", "gtasks", "gstage_ptr", "gfronts", "ginfo")
F64_ON = dict(general_subtrees=1)
F32_ON = dict(float32_general=1, float32_subtrees=1)
CREATORS = ("cnl_create_ex", "cnl_create_f32_ex", "cnl_plan_create_ex", "cnl_multi_create_ex")


@pytest.fixture(scope="module", autouse=True)
def key_known(built):
    """the library parses the key: on a library without it every test of this file fails here"""
    s = GS.structure(GS.FOREST3)
    rows, cols = s.kkt_pattern()
    hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=7, options=hipldl.Options(general_subtrees=1, subtree_solve_panels=0))


def _rc(make):
    try:
        obj = make()
    except hipldl.CnlError as e:
        return e.code, str(e)
    if hasattr(obj, "close"):
        obj.close()
    return 0, ""


def _creators(s):
    """the four creators as functions of (options) -> (code, message); the flag says which element type's keys the creator reads"""
    rows, cols = s.kkt_pattern()
    args = (s.N, rows, cols)
    return {
        "cnl_create_ex": (False, lambda **o: _rc(lambda: hipldl.HIPLDLStruct(*args, None, s.nvar, s.nequ, s.ncon, batch=7, dtype=f64, options=hipldl.Options(**o)))),
        "cnl_create_f32_ex": (True, lambda **o: _rc(lambda: hipldl.HIPLDLStruct(*args, None, s.nvar, s.nequ, s.ncon, batch=7, dtype=f32, options=hipldl.Options(**o)))),
        "cnl_plan_create_ex": (False, lambda **o: _rc(lambda: hipldl.Plan(*args, s.nvar, s.nequ, s.ncon, batch=7, options=hipldl.Options(**o)))),
        "cnl_multi_create_ex": (False, lambda **o: _rc(lambda: hipldl.MultiHIPLDLStruct(*args, s.nvar, s.nequ, s.ncon, 7, [0], options=hipldl.Options(**o)))),
    }


# ---- 1. the key's rules, decided before a device is looked for ----
def test_version():
    assert hipldl.lib().cnl_version() >= 510


@pytest.mark.parametrize("creator", CREATORS)
def test_key_rules_without_a_device(creator):
    s = GS.structure(GS.FOREST3)
    is32, make = _creators(s)[creator]
    on = F32_ON if is32 else F64_ON
    sub = "float32_subtrees" if is32 else "general_subtrees"
    blk = "float32_blocked" if is32 else "general_blocked"
    # accepted: 0 .. 3 where the creator's subtree key is on, blocked or not, alone and with the other subtree keys
    for P in SP.MASKS:
        for extra in ({}, {blk: 1}, {blk: 1, "subtree_ladder": 3, "subtree_wide": 1, "subtree_lds_panels": 4096, "task_cap": 4}):
            rc, msg = make(**dict(on, subtree_solve_panels=P, **extra))
            assert rc != CNL_ERR_ARG and (rc == 0 or "no HIP device" in msg), (P, extra, rc, msg)
    # out of range
    for P in (-1, 4, 7, 256):
        rc, msg = make(**dict(on, subtree_solve_panels=P))
        assert rc == CNL_ERR_ARG and "subtree_solve_panels" in msg, (P, rc, msg)
    # the creator's own subtree key off: absent, written out as 0
    for P in (1, 2, 3):
        for off in ({k: v for k, v in on.items() if k != sub}, dict(on, **{sub: 0})):
            rc, msg = make(**dict(off, subtree_solve_panels=P))
            assert rc == CNL_ERR_ARG and "subtree_solve_panels" in msg and "subtrees" in msg, (P, off, rc, msg)
    # together with float32_refine
    for P in (1, 2, 3):
        for base in (dict(float32_general=1, float32_subtrees=1), dict(float32_general=1, general_subtrees=1)):
            rc, msg = make(**dict(base, float32_refine=1, subtree_solve_panels=P))
            assert rc == CNL_ERR_ARG, (P, base, rc, msg)


def test_the_other_element_types_key_does_not_count():
    """a Float64 creator with the Float32 subtree key alone, and the reverse"""
    c = _creators(GS.structure(GS.FOREST3))
    for name in ("cnl_create_ex", "cnl_multi_create_ex"):
        rc, msg = c[name][1](**dict(F32_ON, subtree_solve_panels=3))
        assert rc == CNL_ERR_ARG and "general_subtrees" in msg, (name, rc, msg)
    rc, msg = c["cnl_create_f32_ex"][1](float32_general=1, subtree_solve_panels=3)
    assert rc == CNL_ERR_ARG and "float32_subtrees" in msg, (rc, msg)


# ---- 2. the key changes no plan ----
@pytest.mark.parametrize("shape,opt", [(GS.GRID12, dict(task_cap=4, general_blocked=1)), (GS.GRID32, dict(condense=0)),
                                       (GS.FOREST3, dict(general_blocked=1))], ids=("grid12-cap4", "grid32-uncondensed", "forest3"))
def test_the_key_changes_no_plan(shape, opt):
    s, off = GS.make_plan(shape, **opt)
    for P in (1, 2, 3):
        s, on = GS.make_plan(shape, **dict(opt, subtree_solve_panels=P))
        assert on.info == off.info
        for name in ARRAYS:
            assert np.array_equal(on.array(name), off.array(name)), (P, name)
    assert len(off.array("gtasks")) > 0


# ---- 3. the panel cut ----
def _plans():
    for shape in SP.CPU_SHAPES:
        caps = (4, 8) if shape in (GS.GRID12, GS.FOREST3) else (8,)
        for cap in caps:
            for cond in (1, 0):
                if shape in (SW.GRID48, SW.GRID70) and not cond:
                    continue
                yield shape, dict(task_cap=cap, condense=cond), GS.make_plan(shape, task_cap=cap, condense=cond, general_blocked=1)[1]
    for shape, cond in ((GS.GRID12, True), (GS.GRID12, False), (GS.GRID32, True), (GS.GRID32, False), (GS.FOREST4, False), (GS.FOREST3, True)):
        yield shape, dict(float32=True, cond=cond), FS.make_plan(shape, cond, SP.CAP.get(shape, 8), blocked=1)[1]
    yield SP.CHAIN, dict(), GS.make_plan(SP.CHAIN, general_blocked=1)[1]
    yield SP.CHAIN, dict(float32=True, cond=True), FS.make_plan(SP.CHAIN, True, 8, blocked=1)[1]


@pytest.fixture(scope="module")
def plans(key_known):
    return list(_plans())


def _check_cut(npiv, nupd):
    f = 1 + nupd + npiv
    bw, fw = SP.backward_panels(npiv, nupd), SP.forward_panels(npiv, nupd)
    n = -(-npiv // SP.PANEL_W)
    assert len(bw) == len(fw) == n
    # ascending from the first pivot row, descending from the last; consecutive, covering the pivots once
    assert bw[0][0] == nupd + 1 and bw[-1][1] == f and all(a[1] == b[0] for a, b in zip(bw, bw[1:]))
    assert fw[0][1] == f and fw[-1][0] == nupd + 1 and all(a[0] == b[1] for a, b in zip(fw, fw[1:]))
    # every panel PANEL_W wide but the last of its sweep, which is as short as it comes
    for cut in (bw, fw):
        w = [p1 - p0 for p0, p1 in cut]
        assert all(x == SP.PANEL_W for x in w[:-1]) and w[-1] == npiv - SP.PANEL_W * (n - 1) and 1 <= w[-1] <= SP.PANEL_W


def test_panel_cut_in_numpy(plans):
    for npiv, nupd in [(1, 0), (1, 5), (15, 3), (16, 0), (16, 11), (17, 2), (18, 7), (31, 0), (32, 40), (33, 1), (93, 0), (207, 0), (19, 355), (356, 0)]:
        _check_cut(npiv, nupd)
    assert SP.backward_panels(18, 2) == [(3, 19), (19, 21)] and SP.forward_panels(18, 2) == [(5, 21), (3, 5)]
    assert SP.backward_panels(7, 4) == [(5, 12)] == SP.forward_panels(7, 4)
    assert SP.backward_panels(16, 0) == [(1, 17)] == SP.forward_panels(16, 0)
    seen = set()
    for shape, opt, plan in plans:
        for fronts in SP.fronts_by_stage(plan):
            for npiv, nupd, indep, fmax in fronts:
                _check_cut(npiv, nupd)
                seen.add(npiv)
    # one short of a panel, exactly one, one over, and counts that are no multiple of 16
    assert set(range(1, 17)) <= seen and {18, 21, 22, 24, 31, 33, 39, 51, 57, 93, 207} <= seen, sorted(seen)


def test_the_gpu_shapes_have_the_fronts_the_tests_are_about(plans):
    """a front of exactly 16 pivots with 11 independent ones; roots; many update rows; and the chain-like tree's (19, 355) and (356, 0):
    more update rows than a workgroup has threads, and 23 panels in one front"""
    fronts = set()
    for shape, opt, plan in plans:
        if shape in (SW.GRID48, SW.GRID70):
            continue
        for st in SP.fronts_by_stage(plan):
            fronts |= {f[:3] for f in st}
    assert any(n == 16 and i == 11 for n, u, i in fronts)
    assert any(u == 0 and n >= 16 for n, u, i in fronts) and max(u for n, u, i in fronts if n < 100) >= 65
    assert any((n, u) == (19, 355) for n, u, i in fronts) and any((n, u) == (356, 0) for n, u, i in fronts)
    assert len(SP.backward_panels(356, 0)) == 23
    assert any(i > 0 and n > 16 for n, u, i in fronts)


# ---- 4. the LDS formula ----
def test_lds_areas_cannot_be_overrun(plans):
    """For every front of every stage: its vector fits vec (f <= the task's fmax <= F_s <= round4(F_s)), the panel's triangle and values
    end inside tri and pv, every carve offset is a multiple of 16 bytes in either element type, and need_s is what the formula says."""
    seen = 0
    for shape, opt, plan in plans:
        F, tasks, has = SW.stage_table(plan)
        for s, fronts in enumerate(SP.fronts_by_stage(plan)):
            o_vec, o_tri, o_pv, end = SP.carve(F[s])
            assert (o_vec, o_tri - o_vec, o_pv - o_tri, end - o_pv) == (0, int(SP.vec_elems(F[s])), 272, 16) and end == int(SP.vec_elems(F[s])) + 288
            for esz in (4, 8):
                assert all(o * esz % 16 == 0 for o in (o_vec, o_tri, o_pv, end))
                assert SP.need_bytes(F[s], esz) == end * esz
            for npiv, nupd, indep, fmax in fronts:
                v, t, p = SP.touched(npiv, nupd)
                assert 1 + nupd + npiv <= fmax <= F[s]
                assert o_vec + v < o_tri and o_tri + t < o_pv and o_pv + p < end, (shape, opt, s, npiv, nupd)
                seen += 1
        for esz in (4, 8):
            lds = SP.stage_lds((F, tasks, has), esz, 3)
            assert (lds == SP.need_bytes(F, esz)).all() and (lds > 0).all()      # every stage of these plans fits: none keeps the old launch
            assert (SP.stage_lds((F, tasks, has), esz, 0) == 0).all()
    assert seen > 1000
    # a stage beyond a workgroup's LDS keeps the unpanelled launch
    big = (np.array([100, 30000]), np.array([3, 1]), np.array([True, True]))
    assert SP.stage_lds(big, 8, 1).tolist() == [(100 + 288) * 8, 0] and SP.stage_lds(big, 4, 2).tolist() == [(100 + 288) * 4, (30000 + 288) * 4]
    assert SP.stage_lds(big, 4, 2, lds_cap=65536).tolist() == [(100 + 288) * 4, 0]


def test_grid70_root(key_known):
    s, plan = GS.make_plan(SW.GRID70, task_cap=8)
    F, tasks, has = SW.stage_table(plan)
    assert F[-1] == 208 and SP.need_bytes(F[-1], 8) == (208 + 288) * 8 and len(SP.backward_panels(207, 0)) == 13


# ---- 5. the sweeps of one front ----
def _front(rng, npiv, nupd, T):
    f = 1 + nupd + npiv
    L = np.tril(rng.standard_normal((f, f))).astype(T)
    L[np.arange(f), np.arange(f)] = (2.0 + rng.random(f)).astype(T)
    return L, rng.standard_normal(f).astype(T)


@pytest.mark.parametrize("T", (f64, f32), ids=("double", "float"))
def test_forward_in_panels_is_the_unpanelled_loop_bit_for_bit(T):
    rng = np.random.default_rng(5)
    for npiv, nupd, indep in ((1, 0, 0), (7, 4, 0), (15, 3, 15), (16, 13, 11), (17, 0, 0), (18, 7, 5), (33, 20, 0), (33, 20, 33), (40, 9, 20), (51, 2, 17)):
        L, z = _front(rng, npiv, nupd, T)
        z[0] = 0
        (Fa, za), (Fb, zb) = SP.forward_unpanelled(L, z, nupd, indep), SP.forward_panelled(L, z, nupd, indep)
        assert Fa.dtype == Fb.dtype == za.dtype == zb.dtype == T
        # the update entries handed to the parent, and every z_i stored
        assert np.array_equal(Fa[: nupd + 1].view(np.uint8), Fb[: nupd + 1].view(np.uint8)), (npiv, nupd, indep)
        assert np.array_equal(za.view(np.uint8), zb.view(np.uint8)), (npiv, nupd, indep)


def test_backward_in_panels_is_another_order_of_the_same_sums():
    rng = np.random.default_rng(6)
    for npiv, nupd in ((1, 0), (7, 4), (16, 0), (17, 30), (33, 20), (51, 2)):
        for lanes in (16, 64):
            L, x = _front(rng, npiv, nupd, f64)
            L[:, 1:] *= 0.1
            a, b = SP.backward_unpanelled(L, x, nupd), SP.backward_panelled(L, x, nupd, lanes)
            assert np.array_equal(a[: nupd + 1], b[: nupd + 1])
            assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max(), (npiv, nupd, lanes)
