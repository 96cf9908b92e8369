"""Float32 handles on the general multifrontal kernel (tuning float32_general), without a GPU: the tuning key, what handle creation
answers on a machine without a device, the ABI version, and the plan of such a handle — the throughput analysis without
condensation — interpreted in float32 on the CPU (tests/support/plan_sim_f32.py) against the fp64 oracle on the widened inputs,
within the project's Float32 tolerances.  That pins, without a GPU, that the plan's operation order in float32 stays within them."""
import ctypes as C

import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn
from oracle import oracle as O
from tests.support import f32_general as G
from tests.support.plan_sim_f32 import PlanSimF32


def test_tuning_key_is_known(built):
    """cnl_options.tuning accepts float32_general = 1 (an unknown key is CNL_ERR_ARG: tuning_parse)"""
    s = syn.random_structure(60, 80, 4, 0.1, seed=3)
    rows, cols = s.kkt_pattern()
    pl = hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(float32_general=1))
    assert pl.info["N"] == s.N
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(float32_generic=1))
    assert e.value.code == 1 and "unknown key" in str(e.value)


def test_version_is_0_3_1(built):
    """0.3.1 in the header's encoding, major * 10000 + minor * 100 + patch (0.3.0 was 300)"""
    assert hipldl.lib().cnl_version() >= 301


def test_create_without_a_device(built):
    """no device: with the option a non-band pattern gets as far as the device check (CNL_ERR_HIP); without it the pattern is refused
    for the band kernels' reason (CNL_ERR_ARG naming build_band_plan), as on a machine with a device — where the option gives a handle"""
    s = syn.random_structure(60, 80, 4, 0.1, seed=3)
    rows, cols = hipldl._i64(s.kkt_pattern()[0]), hipldl._i64(s.kkt_pattern()[1])
    lib = hipldl.lib()
    try:
        import torch
        have_device = torch.cuda.device_count() > 0
    except Exception:
        have_device = False
    h = C.c_void_p()
    on, off = hipldl.Options(float32_general=1), hipldl.Options()
    rc = lib.cnl_create_f32_ex(C.byref(h), s.N, len(rows), rows, cols, s.nvar, s.nequ, s.ncon, 4, 0, C.byref(on))
    if have_device:
        assert rc == 0 and h.value, lib.cnl_last_error()
        lib.cnl_destroy(h)
    else:
        assert rc == 4 and not h.value, lib.cnl_last_error()      # CNL_ERR_HIP
    h = C.c_void_p()
    rc = lib.cnl_create_f32_ex(C.byref(h), s.N, len(rows), rows, cols, s.nvar, s.nequ, s.ncon, 4, 0, C.byref(off))
    assert rc == 1 and not h.value and b"build_band_plan" in lib.cnl_last_error()   # CNL_ERR_ARG


CASES = ([("random", seed) for seed in range(100, 106)] + [("band3", seed) for seed in range(4000, 4004)])


@pytest.fixture(scope="module")
def sims(built):
    out = {}
    for name, s in (("random", syn.random_structure(60, 80, 4, 0.1, seed=3)), ("band3", syn.band_structure(400, 4, hw=3))):
        rows, cols = s.kkt_pattern()
        pl = hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(**G.GENERAL_PLAN))
        assert pl.info["ncond"] == 0
        out[name] = (s, PlanSimF32(pl))
    return out


@pytest.mark.parametrize("name,seed", CASES)
def test_plan_in_float32_stays_within_the_tolerances(sims, name, seed):
    s, sim = sims[name]
    gen = syn.random_values if name == "random" else syn.band_values
    vals, rhs = G.stack32([gen(s, seed)])
    p32 = hipldl.default_params(np.float32)
    ref = G.oracle_newton(O, s, vals, rhs, np.zeros(1, np.float32), p32)
    assert ref["ok"][0] and ref["nf"][0] == 1
    d, ok, rho, ro, nf = sim.newton_system(vals[0], rhs[0], s.nvar, s.nequ, s.ncon, 0.0, p32)
    assert d.dtype == np.float32
    be, fe = G.check_results(s, ref, vals, rhs, d, [ok], [rho], [ro], [nf])
    print(f"{name} seed {seed}: backward error {be / G.EPS32:.1f} eps32, forward error {fe:.2e}")
