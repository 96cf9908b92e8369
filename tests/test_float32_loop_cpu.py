"""The Float32 lockstep outer loop, without a GPU: the nine `cnl_outer_*_f32_dev` entry points (exported, listed, declared, argument
checks that launch nothing), `cnl_outer_state_f32` against the C compiler's layout, the Float32 `BandQuadFamily`, and the band
programs the loop's patterns need for a Float32 handle."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import device_loop as DL, hipldl, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CNL_ERR_ARG = 1

OUTER = ["begin", "newton_done", "extrapolated", "trial_done", "end", "ls_begin", "ls_test", "ls_step", "ls_take"]
F32_SYMBOLS = [f"cnl_outer_{k}_f32_dev" for k in OUTER]
SCALARS = ("B", "n", "m", "p", "P", "N", "nnzjF", "nnzjc", "max_inner", "dmin", "rhomax", "delta_dec", "smax", "gammaA", "eps2")
LS_ARRAYS = ("ls_g", "xl", "Fl", "cl", "lam_ls", "alpha", "Dphi", "phix", "eta", "nbk", "bt")


def test_outer_f32_symbols_are_exported_listed_and_declared(built):
    lib = C.CDLL(hipldl.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "cannoles_hip.h")).read()
    declared = set(re.findall(r"\b(cnl_[a-z0-9_]+)\s*\(", hdr))
    for sym in F32_SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in hipldl.ABI_SYMBOLS, sym
        assert sym in declared, sym
    assert "typedef struct cnl_outer_state_f32" in hdr


def test_state_f32_layout_is_the_c_compilers(built, tmp_path):
    """size and every member offset of the ctypes mirror, held by negative-size arrays in a C99 translation unit; member names and
    order are cnl_outer_state's"""
    S = hipldl.cnl_outer_state_f32
    assert [f[0] for f in S._fields_] == [f[0] for f in hipldl.cnl_outer_state._fields_]
    for (k, ty), (_, ty64) in zip(S._fields_, hipldl.cnl_outer_state._fields_):
        assert ty is (C.c_float if ty64 is C.c_double else ty64), k
    lines = ["#include <stddef.h>", '#include "cannoles_hip.h"',
             f"typedef char size_ok[sizeof(cnl_outer_state_f32) == {C.sizeof(S)} ? 1 : -1];"]
    for k, _ in S._fields_:
        lines.append(f"typedef char off_{k}[offsetof(cnl_outer_state_f32, {k}) == {getattr(S, k).offset} ? 1 : -1];")
    lines.append("int main(void) { return 0; }")
    src = tmp_path / "state_f32.c"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "state_f32.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _call(name, st):
    fn = getattr(hipldl.lib(), f"cnl_outer_{name}_f32_dev")
    ref = C.byref(st) if st is not None else None
    return fn(ref, 1, None) if name in ("newton_done", "ls_test") else fn(ref, None)


def _filled_state():
    """every size positive and every array a (never dereferenced) non-null address"""
    st = hipldl.cnl_outer_state_f32()
    for k, _ in st._fields_:
        if k not in SCALARS:
            setattr(st, k, 4096)
    st.B, st.n, st.m, st.p, st.P, st.N, st.nnzjF, st.nnzjc, st.max_inner = 2, 3, 3, 1, 1, 7, 5, 2, 10
    return st


@pytest.mark.parametrize("name", OUTER)
def test_argument_checks_launch_nothing(built, name):
    """CNL_ERR_ARG for a null state, B <= 0, and a state with one required array left null — for every required array of the entry
    point (the line-search arrays are required by the ls_* entries only).  The checks come before any launch, so this runs without a GPU."""
    assert _call(name, None) == CNL_ERR_ARG
    st = _filled_state()
    st.B = 0
    assert _call(name, st) == CNL_ERR_ARG
    required = [k for k, _ in hipldl.cnl_outer_state_f32._fields_ if k not in SCALARS and (name.startswith("ls_") or k not in LS_ARRAYS)]
    assert len(required) == (67 if name.startswith("ls_") else 56)
    for k in required:
        st = _filled_state()
        setattr(st, k, None)
        assert _call(name, st) == CNL_ERR_ARG, k


def test_float32_family_on_the_cpu(built):
    import torch
    s = syn.band_structure(300, 4)
    f64 = DL.BandQuadFamily(s, 6, seed=304, torch=torch, device="cpu")
    f32 = DL.BandQuadFamily(s, 6, seed=304, torch=torch, device="cpu", dtype=np.float32)
    assert f64.dtype == np.float64 and f32.dtype == np.float32
    for k, v in f32.h.items():
        assert v.dtype == np.float64 and np.array_equal(v.astype(np.float32).astype(np.float64), v), k   # float32-representable
        assert np.array_equal(v, f64.h[k].astype(np.float32).astype(np.float64)), k                     # the float64 data, rounded once
        assert f32.d[k].dtype == torch.float32 and np.array_equal(f32.d[k].numpy().astype(np.float64), v), k
        assert f64.d[k].dtype == torch.float64
    x = f32.d["x0"]
    for out in (f32.residual(x), f32.jac_vals(x), f32.hess_vals(x, f32.residual(x)), f32.cons(x), f32.jacc_vals(x)):
        assert out.dtype == torch.float32
    # the host twin evaluates the rounded data in float64: the device residual is its float32 evaluation
    F64 = f32.host_model(2).residual(f32.h["x0"][2])
    assert np.abs(f32.residual(x)[2].numpy() - F64).max() <= 64 * np.finfo(np.float32).eps * max(1.0, np.abs(F64).max())
    for a, b in zip(DL.kkt_pattern_of(f32)[:2], DL.kkt_pattern_of(f64)[:2]):
        assert np.array_equal(a, b)
    assert DL.kkt_pattern_of(f32)[2] == DL.kkt_pattern_of(f64)[2]
    with pytest.raises(TypeError):
        DL.BandQuadFamily(s, 2, seed=1, torch=torch, device="cpu", dtype=np.float16)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_take_selects_problems_and_shares_the_structure(built, dtype):
    import torch
    s = syn.band_structure(300, 4)
    fam = DL.BandQuadFamily(s, 7, seed=304, torch=torch, device="cpu", dtype=dtype)
    idx = [5, 0, 3]
    sub = fam.take(idx)
    assert sub.B == 3 and sub.dtype == fam.dtype and sub.s is fam.s and sub.row_ent_t is fam.row_ent_t and fam.B == 7
    for k in fam.h:
        assert np.array_equal(sub.h[k], fam.h[k][idx]) and torch.equal(sub.d[k], fam.d[k][idx])
    x = sub.d["x0"]
    assert torch.equal(sub.residual(x), fam.residual(fam.d["x0"])[idx])
    assert torch.equal(sub.cons(x), fam.cons(fam.d["x0"])[idx])
    assert np.array_equal(sub.host_model(1).x0, fam.host_model(0).x0)
    one = fam.take(range(5)).take([4])
    assert one.B == 1 and np.array_equal(one.h["y"][0], fam.h["y"][4])


def test_element_type_of_a_run_is_the_familys(built):
    """the driver refuses a family of the other element type before it touches the device (the C side cannot tell the arrays apart)"""
    import torch
    s = syn.band_structure(300, 4)
    f64 = DL.BandQuadFamily(s, 2, seed=304, torch=torch, device="cpu")
    f32 = DL.BandQuadFamily(s, 2, seed=304, torch=torch, device="cpu", dtype=np.float32)
    for solve in (DL.solve_batch_device, DL.solve_batch_device_framework):
        with pytest.raises(TypeError):
            solve(f64, dtype=np.float32)
        with pytest.raises(TypeError):
            solve(f32, dtype=np.float64)
        with pytest.raises(TypeError):
            solve(f32, dtype=np.float16)


@pytest.mark.parametrize("shape", [(300, 4), (300, 0), (600, 6), (1000, 10)])
def test_loop_patterns_carry_a_float32_band_program(built, shape):
    """throughput plans of the pattern the loop hands over (kkt_pattern_of: H_c with the model's Hessian structure when p > 0): the wide
    4-byte program for a constrained family, the 15-piece 4-byte program without constraints"""
    import torch
    n, p = shape
    s = syn.band_structure(n, p)
    fam = DL.BandQuadFamily(s, 1, seed=n + p, torch=torch, device="cpu", dtype=np.float32)
    rows, cols, _ = DL.kkt_pattern_of(fam)
    pl = hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT))
    assert pl.array("bandw4_info" if p > 0 else "band4_info")[0] == 1
