"""Float32 general handles on the register-front kernel (tuning float32_register_front), without a GPU: the tuning key, the ABI
version, and the plan cnl_create_f32_ex builds for such a handle — the throughput analysis of the condensed system with
register-front records that are never direct (tests/support/f32_register_front.py: RF_PLAN) — on the patterns the GPU tests name:
the front classes the kernel's three elimination paths see, and the pattern whose front is too large for them."""
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn
from tests.support.f32_register_front import RF_PLAN


def _plan(s, **opt):
    rows, cols = s.kkt_pattern()
    return hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(**opt))


def test_tuning_key_is_known(built):
    """cnl_options.tuning accepts float32_register_front = 1; a misspelt key is still CNL_ERR_ARG (tuning_parse)"""
    s = syn.random_structure(60, 80, 4, 0.1, seed=3)
    assert _plan(s, float32_register_front=1).info["N"] == s.N
    with pytest.raises(hipldl.CnlError) as e:
        _plan(s, float32_register_fronts=1)
    assert e.value.code == 1 and "unknown key" in str(e.value)


def test_version_is_0_4_1(built):
    assert hipldl.lib().cnl_version() >= 401


@pytest.mark.parametrize("name,make,classes,ustack", [
    ("chain", lambda: syn.band_structure(60, 2, hw=3), (7, 0, 0), 36),
    ("class32", lambda: syn.random_structure(30, 40, 2, 0.15, seed=1), (0, 2, 0), None),
    ("class32-dense", lambda: syn.dense_structure(24, 40), (0, 1, 0), None),
    ("class64", lambda: syn.random_structure(60, 80, 4, 0.1, seed=3), (0, 0, 2), None),
    ("class64-dense", lambda: syn.dense_structure(60, 90), (0, 0, 1), None),
    ("all-classes", lambda: syn.random_structure(40, 56, 2, 0.06, seed=3), (2, 3, 1), None),
    ("lockstep", lambda: syn.band_structure(300, 4, hw=3), (38, 0, 0), None)])
def test_front_classes_of_the_named_patterns(built, name, make, classes, ustack):
    pl = _plan(make(), **RF_PLAN)
    v2 = pl.info["v2"]
    assert v2 is not None and pl.info["ncond"] > 0, pl.info
    assert (v2["fronts16"], v2["fronts32"], v2["fronts64"]) == classes, v2
    assert pl.info["fmax"] <= 64
    if ustack is not None:
        assert v2["ustack"] == ustack


def test_chain_with_small_ubig_keeps_its_update_matrices_in_global_scratch(built):
    pl = _plan(syn.band_structure(60, 2, hw=3), ubig=4, **RF_PLAN)
    assert pl.info["v2"]["ustack"] == 2 and pl.info["v2"]["fronts16"] == 7


def test_front_above_order_64_has_no_register_front_records(built):
    pl = _plan(syn.dense_structure(100, 160), **RF_PLAN)
    assert pl.info["v2"] is None and pl.info["fmax"] == 101 and pl.info["ncond"] == 160
