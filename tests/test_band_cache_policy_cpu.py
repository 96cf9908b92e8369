"""Tuning band_cache_policy (csrc/options.h; csrc/band.hip, BAND_POL_*) without a GPU: the key parses, a mask that asks for both
forms of record store (bits 4 and 8) or that the band kernel has no instance for is refused at plan creation, and the plan is the
plan without the key — the policy changes no word of a band program."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn

BUILT = (7,)    # csrc/band.hip: BAND_POLICY_MASKS (beside 0, the plain instance)
DEFAULT = 7     # csrc/options.h: the arm that passed the rule of DESIGN section 4


def _plan(**opt):
    s = syn.band_structure(200, 4)
    rows, cols = s.kkt_pattern()
    return hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT, **opt))


def test_the_key_parses_and_changes_no_program(built):
    base = _plan()
    for mask in (0,) + BUILT:
        pl = _plan(band_cache_policy=mask)
        for name in ("bandr_info", "bandm_info", "bandm_table0", "bandm_table1", "bandr_epochs0", "bandr_fops0", "bandr_bops1"):
            assert np.array_equal(pl.array(name), base.array(name)), (mask, name)
    assert base.array("bandm_info")[0] == 1


def test_the_key_is_a_tuning_key_only(built):
    assert "band_cache_policy" not in [f[0] for f in hipldl.cnl_options._fields_]
    o = hipldl.Options(band_cache_policy=3)
    assert b"band_cache_policy=3" in o.tuning
    assert b"band_cache_policy" not in hipldl.Options().tuning   # the default is the library's (options.h), not the wrapper's


@pytest.mark.parametrize("mask", [12, 13, 15, 28, 31])
def test_both_forms_of_record_store_are_refused(built, mask):
    with pytest.raises(hipldl.CnlError, match="band_cache_policy.*exclude each other"):
        _plan(band_cache_policy=mask)


@pytest.mark.parametrize("mask", [1, 2, 3, 4, 8, 11, 16, 23, 27, 32, 64, -1])
def test_a_mask_without_an_instance_is_refused(built, mask):
    assert mask not in BUILT
    with pytest.raises(hipldl.CnlError, match="band_cache_policy"):
        _plan(band_cache_policy=mask)


def test_the_default_is_a_built_mask(built):
    """default options make a plan, and so does naming the default or the plain instance (what a handle then reports is checked on
    the GPU: tests/test_band_cache_policy_gpu.py)"""
    assert DEFAULT in (0,) + BUILT
    _plan()
    _plan(band_cache_policy=DEFAULT)
    _plan(band_cache_policy=0)
