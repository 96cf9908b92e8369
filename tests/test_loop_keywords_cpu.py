"""The keywords of the reference's `solve!` in the lockstep loop, without a GPU: the control block `cnl_outer_ctl` against the C compiler's
layout, the `_ex` entry points and the mask kernel (exported, listed, declared, argument checks that launch nothing), the Gauss-Newton
pattern, and the host mirror's `Newton_vanishing`, `use_initial_multiplier` and `LM` handling."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import device_loop as DL, hipldl, outer_loop, synthetic as syn
from tests.support.counting_model import CountingModel
from tests.test_oracle_pinning import oracle_newton, oracle_solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CNL_ERR_ARG = 1
EX = ["begin_ex", "trial_done_ex", "ls_test_ex", "end_ex", "hess_mask"]
SYMBOLS = [f"cnl_outer_{k}{sfx}" for k in EX for sfx in ("_dev", "_f32_dev")]
SCALARS = ("B", "n", "m", "p", "P", "N", "nnzjF", "nnzjc", "max_inner", "dmin", "rhomax", "delta_dec", "smax", "gammaA", "eps2")
DEFAULT = dict(curvature=0.3, start=0.3, noise=0.01)


def _family(p, B=12, **kind):
    import torch
    return DL.BandQuadFamily(syn.band_structure(40, p), B, seed=40 + p, torch=torch, device="cpu", **(kind or DEFAULT))


def test_ctl_layout_is_the_c_compilers(built, tmp_path):
    """sizeof and every member offset of the ctypes mirror, held by negative-size arrays in a small C99 program built with the header"""
    S = hipldl.cnl_outer_ctl
    lines = ["#include <stddef.h>", '#include "cannoles_hip.h"', f"typedef char size_ok[sizeof(cnl_outer_ctl) == {C.sizeof(S)} ? 1 : -1];"]
    lines += [f"typedef char off_{k}[offsetof(cnl_outer_ctl, {k}) == {getattr(S, k).offset} ? 1 : -1];" for k, _ in S._fields_]
    lines.append("int main(void) { return 0; }")
    src = tmp_path / "ctl.c"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "ctl.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [k for k, _ in S._fields_] == ["struct_size", "always_accept_extrapolation", "max_iter", "max_eval", "evals_per_point", "neval", "hess_upd"]
    c = hipldl.outer_ctl(4096, 2, True, 8, 12, 8192)
    assert (c.struct_size, c.always_accept_extrapolation, c.max_iter, c.max_eval, c.evals_per_point, c.neval, c.hess_upd) == (C.sizeof(S), 1, 8, 12, 2, 4096, 8192)


def test_new_symbols_are_exported_listed_and_declared(built):
    lib = C.CDLL(hipldl.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "cannoles_hip.h")).read()
    declared = set(re.findall(r"\b(cnl_[a-z0-9_]+)\s*\(", hdr))
    for sym in SYMBOLS:
        assert hasattr(lib, sym) and sym in hipldl.ABI_SYMBOLS and sym in declared, sym
    assert "typedef struct cnl_outer_ctl" in hdr
    assert hipldl.lib().cnl_version() >= 400   # 0.4.0: the ABI grew
    assert hipldl.OUTER_STATUS_NAMES == {0: "unknown", 1: "first_order", 2: "small_residual", 3: "exception", 4: "max_eval", 5: "stalled",
                                         6: "max_iter", 7: "max_time"}


def _filled_state(f32):
    """every size positive and every array a (never dereferenced) non-null address"""
    st = hipldl.cnl_outer_state_f32() if f32 else hipldl.cnl_outer_state()
    for k, _ in st._fields_:
        if k not in SCALARS:
            setattr(st, k, 4096)
    st.B, st.n, st.m, st.p, st.P, st.N, st.nnzjF, st.nnzjc, st.max_inner = 2, 3, 3, 1, 1, 7, 5, 2, 10
    return st


def _call(name, f32, st, ctl):
    fn = getattr(hipldl.lib(), f"cnl_outer_{name}" + ("_f32_dev" if f32 else "_dev"))
    ref, cref = C.byref(st) if st is not None else None, C.byref(ctl) if ctl is not None else None
    return fn(ref, 1, cref, None) if name == "ls_test_ex" else fn(ref, cref, None)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", EX)
def test_argument_checks_launch_nothing(built, name, f32):
    """CNL_ERR_ARG before any launch (so this runs without a GPU): a wrong struct_size, a null neval, evals_per_point outside {1, 2}, the
    state's own rules with a good block, and for the mask kernel a null block or a null hess_upd"""
    good = lambda: hipldl.outer_ctl(4096, 2, hess_upd=4096)
    for field, value in (("struct_size", C.sizeof(hipldl.cnl_outer_ctl) - 8), ("struct_size", 0), ("neval", None), ("evals_per_point", 0),
                         ("evals_per_point", 3), ("evals_per_point", -1)):
        ctl = good()
        setattr(ctl, field, value)
        assert _call(name, f32, _filled_state(f32), ctl) == CNL_ERR_ARG, (field, value)
    assert _call(name, f32, None, good()) == CNL_ERR_ARG
    st = _filled_state(f32)
    st.B = 0
    assert _call(name, f32, st, good()) == CNL_ERR_ARG
    st = _filled_state(f32)
    st.status = None
    assert _call(name, f32, st, good()) == CNL_ERR_ARG and _call(name, f32, st, None) == CNL_ERR_ARG
    if name == "hess_mask":
        assert _call(name, f32, _filled_state(f32), None) == CNL_ERR_ARG
        ctl = good()
        ctl.hess_upd = None
        assert _call(name, f32, _filled_state(f32), ctl) == CNL_ERR_ARG


class _Stop(Exception):
    pass


@pytest.mark.parametrize("p", [0, 4])
def test_gauss_newton_pattern_is_the_host_mirrors(built, params, p):
    """kkt_pattern_of(fam, "Newton_noFHess") is the pattern outer_loop.solve hands to make_solver: no H_F segment; the other methods keep it"""
    fam = _family(p, B=2)
    seen = {}

    def make_solver(N, rows, cols, vals, n, m, pp):
        seen.update(N=N, rows=rows.copy(), cols=cols.copy(), vals=vals.copy())
        raise _Stop

    for method in ("Newton_noFHess", "Newton", "Newton_vanishing"):
        with pytest.raises(_Stop):
            outer_loop.solve(fam.host_model(0), make_solver, oracle_newton, params, method=method)
        rows, cols, (nnzhF, nnzhc, nnzjF, nnzjc) = DL.kkt_pattern_of(fam, method)
        assert rows.dtype == np.int64 and np.array_equal(rows, seen["rows"]) and np.array_equal(cols, seen["cols"]), method
        nh = len(np.asarray(fam.s.hF[0]))
        assert nnzhF == (0 if method == "Newton_noFHess" else nh) and nnzhc == (nh if p else 0)
        assert len(rows) == nnzhF + nnzhc + nnzjF + nnzjc + fam.s.nequ + p + fam.s.nvar
    assert all(np.array_equal(a, b) for a, b in zip(DL.kkt_pattern_of(fam)[:2], DL.kkt_pattern_of(fam, "Newton")[:2]))


def test_lm_and_unknown_methods_are_refused(built, params):
    fam = _family(0, B=2)
    for method in ("LM", "newton", "BFGS", None):
        with pytest.raises(ValueError):
            DL.kkt_pattern_of(fam, method)
        with pytest.raises(ValueError):
            outer_loop.solve(fam.host_model(0), oracle_solver, oracle_newton, params, method=method)
        with pytest.raises(ValueError):
            DL.solve_batch_device(fam, method=method)


def test_host_mirror_newton_vanishing_skips_updates(built, params):
    """default family (40, 0), seed 40: problems 5, 9 and 10 come within dot(Fx, Fx) <= 1e-8 before they are first_order and skip one H_F
    refresh; the others never skip and run exactly as :Newton.  A model whose Hessian callback counts its calls shows the skip is a
    call not made."""
    fam = _family(0)
    for b in range(12):
        calls = []
        model = fam.host_model(b)
        hess = model.hess_coord_residual
        model.hess_coord_residual = lambda x, r: (calls.append(1), hess(x, r))[1]
        van = outer_loop.solve(model, oracle_solver, oracle_newton, params, method="Newton_vanishing")
        newton = outer_loop.solve(fam.host_model(b), oracle_solver, oracle_newton, params)
        assert van["status"] == newton["status"] == "first_order" and newton["hess_skipped"] == 0
        assert van["hess_skipped"] == (1 if b in (5, 9, 10) else 0), b
        assert len(calls) == van["nlinsolve"] - van["hess_skipped"]
        if van["hess_skipped"] == 0:
            assert van["iter"] == newton["iter"] and np.array_equal(van["solution"], newton["solution"])


def test_host_mirror_honours_the_initial_multiplier(built, params):
    """the first Newton system's right-hand side is [J'F - Jc'lam; 0; c] with the caller's lam when use_initial_multiplier, and with the
    least-squares estimate (whatever `lam` holds) when not; `x` is the start point"""
    fam = _family(4, B=2)
    model = fam.host_model(1)
    x = model.x0 + 0.125
    lam0 = np.array([0.5, -2.0, 0.0, 3.0])
    seen = []

    def newton(LDLT, n, m, p, rhs, vals, rho_old, prm):
        seen.append(rhs.copy())
        raise _Stop

    for kw in (dict(lam=lam0, use_initial_multiplier=True), dict(lam=lam0), dict()):
        with pytest.raises(_Stop):
            outer_loop.solve(fam.host_model(1), oracle_solver, newton, params, x=x, **kw)
    n, m = model.nvar, model.nequ
    g = model.jac_residual(x).T @ model.residual(x)
    assert np.array_equal(seen[0][:n], g - model.jac(x).T @ lam0)
    assert np.array_equal(seen[0][n + m:], model.cons(x)) and not seen[0][n:n + m].any()
    assert np.array_equal(seen[1], seen[2]) and not np.array_equal(seen[0][:n], seen[1][:n])
    lam_ls = outer_loop.cgls(model.jac(x).T, g)
    assert np.array_equal(seen[1][:n], g - model.jac(x).T @ lam_ls)
    # zero start multipliers stay zero (no ones-if-zero rule, src/CaNNOLeS.jl:512-518)
    with pytest.raises(_Stop):
        outer_loop.solve(fam.host_model(1), oracle_solver, newton, params, x=x, use_initial_multiplier=True)
    assert np.array_equal(seen[3][:n], g)


def test_counting_model_counts_residual_and_constraint_evaluations(built, params):
    for p, per_point in ((0, 1), (4, 2)):
        fam = _family(p, B=2)
        model = CountingModel(fam.host_model(0))
        out = outer_loop.solve(model, oracle_solver, oracle_newton, params)
        assert out["status"] == "first_order" and out["nbk"] == 0
        assert model.neval == per_point * (1 + out["nlinsolve"])   # the start point and one trial point per Newton system
