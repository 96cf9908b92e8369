"""Running the lockstep loop on its active problems only, without a GPU: the four entry points (cnl_set_active_batch,
cnl_get_active_batch, cnl_outer_compact_dev, cnl_outer_compact_f32_dev) are exported, listed and declared; their argument checks
launch nothing; and the pairing rule of the compaction (tests/support/compact_sim.py, what the GPU tests compare the kernels with)
keeps its invariants: a permutation, the active set in front, a second pass the identity."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import device_loop as DL, hipldl, synthetic as syn
from tests.support import compact_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CNL_ERR_ARG = 1
NEW_SYMBOLS = ["cnl_set_active_batch", "cnl_get_active_batch", "cnl_outer_compact_dev", "cnl_outer_compact_f32_dev"]
SCALARS = ("B", "n", "m", "p", "P", "N", "nnzjF", "nnzjc", "max_inner", "dmin", "rhomax", "delta_dec", "smax", "gammaA", "eps2")
LS_ARRAYS = ("ls_g", "xl", "Fl", "cl", "lam_ls", "alpha", "Dphi", "phix", "eta", "nbk", "bt")


def test_symbols_are_exported_listed_and_declared(built):
    lib = C.CDLL(hipldl.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "cannoles_hip.h")).read()
    declared = set(re.findall(r"\b(cnl_[a-z0-9_]+)\s*\(", hdr))
    for sym in NEW_SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in hipldl.ABI_SYMBOLS, sym
        assert sym in declared, sym
    assert hipldl.lib().cnl_version() >= 300   # the ABI grew


def test_active_batch_argument_checks(built):
    lib = hipldl.lib()
    assert lib.cnl_set_active_batch(None, 1) == CNL_ERR_ARG
    n = C.c_int64(7)
    assert lib.cnl_get_active_batch(None, C.byref(n)) == CNL_ERR_ARG and n.value == 7


def _filled_state(cls):
    """every size positive and every array a (never dereferenced) non-null address"""
    st = cls()
    for k, _ in st._fields_:
        if k not in SCALARS:
            setattr(st, k, 4096)
    st.B, st.n, st.m, st.p, st.P, st.N, st.nnzjF, st.nnzjc, st.max_inner = 2, 3, 3, 1, 1, 7, 5, 2, 10
    return st


def _compact(fn, st, nextra=2, extra=True, rows=(4, 24), min_finished=1, orig=4096, counts=4096, work=4096):
    ptrs = (C.c_void_p * 2)(4096, 8192)
    rb = (C.c_int64 * 2)(*rows)
    return fn(C.byref(st) if st is not None else None, nextra, ptrs if extra else None, rb if extra else None, min_finished, orig, counts, work, None)


@pytest.mark.parametrize("f32", [False, True])
def test_compact_argument_checks_launch_nothing(built, f32):
    """CNL_ERR_ARG for a null state, B <= 0, every required array of the state left null in turn, and a null / inconsistent argument
    of the call itself.  The checks come before any launch, so this runs without a GPU."""
    fn = getattr(hipldl.lib(), "cnl_outer_compact_f32_dev" if f32 else "cnl_outer_compact_dev")
    cls = hipldl.cnl_outer_state_f32 if f32 else hipldl.cnl_outer_state
    assert _compact(fn, None) == CNL_ERR_ARG
    for bad_B in (0, -3):
        st = _filled_state(cls)
        st.B = bad_B
        assert _compact(fn, st) == CNL_ERR_ARG
    required = [k for k, _ in cls._fields_ if k not in SCALARS and k not in LS_ARRAYS]
    assert len(required) == 56
    for k in required:
        st = _filled_state(cls)
        setattr(st, k, None)
        assert _compact(fn, st) == CNL_ERR_ARG, k
    st = _filled_state(cls)
    assert _compact(fn, st, min_finished=0) == CNL_ERR_ARG
    assert _compact(fn, st, orig=None) == CNL_ERR_ARG
    assert _compact(fn, st, counts=None) == CNL_ERR_ARG
    assert _compact(fn, st, work=None) == CNL_ERR_ARG
    assert _compact(fn, st, extra=False) == CNL_ERR_ARG       # two extra arrays announced, none given
    assert _compact(fn, st, nextra=-1) == CNL_ERR_ARG
    assert _compact(fn, st, nextra=1000) == CNL_ERR_ARG
    assert _compact(fn, st, rows=(4, 0)) == CNL_ERR_ARG        # an extra array without row bytes


def _check_case(status, Bc, min_finished):
    status = np.asarray(status, dtype=np.int32)
    B = len(status)
    perm, (A, Bn) = compact_sim.compact(status, Bc, min_finished)
    assert np.array_equal(np.sort(perm), np.arange(B))                       # a permutation: nothing is lost
    assert np.array_equal(perm[Bc:], np.arange(Bc, B))                       # rows outside the working batch stay
    active = np.flatnonzero(status[:Bc] == 0)
    assert A == len(active)
    after = compact_sim.apply(perm, status)
    if Bc - A < min_finished:
        assert Bn == Bc and np.array_equal(perm, np.arange(B))
        return perm, (A, Bn)
    assert Bn == A
    assert np.array_equal(np.sort(perm[:A]), active)                         # the first A rows are exactly the active set
    assert (after[:A] == 0).all() and (after[A:Bc] != 0).all()
    stay = np.flatnonzero((status[:A] == 0))
    assert np.array_equal(perm[stay], stay)                                   # an active row below A does not move
    perm2, counts2 = compact_sim.compact(after, Bn if Bn > 0 else 1, min_finished)
    assert np.array_equal(perm2, np.arange(B))                               # a second pass is the identity
    if Bn > 0:
        assert counts2 == (A, A)
    return perm, (A, Bn)


def edge_cases(B=70):
    """(name, statuses, Bc, min_finished): the cases the GPU test of the kernels runs too"""
    rng = np.random.default_rng(B)
    code = lambda k: rng.integers(1, 6, k).astype(np.int32)
    prefix = np.concatenate([np.zeros(B - B // 3, np.int32), code(B // 3)])
    suffix_only = prefix.copy()
    mixed = np.where(rng.uniform(size=B) < 0.4, code(B), 0).astype(np.int32)
    few = np.zeros(B, np.int32)
    few[rng.choice(B, min(3, B), replace=False)] = 1
    return [("all active", np.zeros(B, np.int32), B, 1),
            ("none active", code(B), B, 1),
            ("active rows already the prefix", prefix, B, 1),
            ("finished rows only in the suffix", suffix_only, B, max(1, B // 3)),
            ("mixed", mixed, B, 1),
            ("mixed, working batch below B", mixed, max(1, B - B // 4), 1),
            ("threshold not reached", few, B, 4),
            ("threshold just reached", few, B, min(3, B))]


def test_pairing_rule_edge_cases():
    for B in (70, 1):
        for name, status, Bc, mf in edge_cases(B):
            perm, (A, Bn) = _check_case(status, Bc, mf)
            if name == "all active":
                assert (A, Bn) == (B, B) and np.array_equal(perm, np.arange(B))
            if name == "none active":
                assert (A, Bn) == (0, 0) and np.array_equal(perm, np.arange(B))
            if name in ("active rows already the prefix", "finished rows only in the suffix"):
                assert np.array_equal(perm, np.arange(B)) and Bn == A
            if name == "threshold not reached":
                assert Bn == Bc
    perm, counts = compact_sim.compact([0, 3, 0, 1, 0, 0], 6, 1)
    assert perm.tolist() == [0, 4, 2, 5, 1, 3] and counts == (4, 4)          # rows 1, 3 (finished) <-> rows 4, 5 (active), in order
    with pytest.raises(ValueError):
        compact_sim.compact([0, 1], 3, 1)
    with pytest.raises(ValueError):
        compact_sim.compact([0, 1], 2, 0)


def test_pairing_rule_random_cases():
    rng = np.random.default_rng(2024)
    for _ in range(300):
        B = int(rng.integers(1, 200))
        status = np.where(rng.uniform(size=B) < rng.uniform(), rng.integers(1, 6, B), 0)
        _check_case(status, int(rng.integers(1, B + 1)), int(rng.integers(1, B + 2)))


def test_family_head_is_a_view_of_the_first_problems(built):
    import torch
    s = syn.band_structure(300, 4)
    fam = DL.BandQuadFamily(s, 7, seed=304, torch=torch, device="cpu", dtype=np.float32)
    assert set(fam.per_problem_tensors()) == set(fam.d) and all(v.shape[0] == 7 for v in fam.per_problem_tensors().values())
    sub = fam.head(3)
    assert sub.B == 3 and fam.B == 7 and sub.s is fam.s and sub.row_ent_t is fam.row_ent_t
    for k, v in fam.d.items():
        assert sub.d[k].data_ptr() == v.data_ptr() and torch.equal(sub.d[k], v[:3]), k   # views, not copies
    x = fam.d["x0"]
    assert torch.equal(sub.residual(x[:3]), fam.residual(x)[:3])
    assert torch.equal(sub.cons(x[:3]), fam.cons(x)[:3])
    assert torch.equal(sub.jac_vals(x[:3]), fam.jac_vals(x)[:3])
    assert torch.equal(fam.head(7).residual(x), fam.residual(x))
    for bad in (0, 8):
        with pytest.raises(ValueError):
            fam.head(bad)
