"""The cache policies of the band kernel's mover-table instance on the GPU (tuning band_cache_policy; csrc/band.hip: BAND_POL_*).  -m gpu.

A policy changes which cache bits the once-touched streams carry — typed vals and factor loads, record stores, d stores — and no
instruction besides: for every mask that is built, try_to_factorize -> solve_ldl! -> newton_system! on an interleaved handle must
give every output bit for bit what mask 0 gives.  The handle reports its mask in config["band_cache_policy"]; a handle that does
not run the mover-table instance ignores the key and reports 0."""
import numpy as np
import pytest

from tests.test_band_cache_policy_cpu import BUILT, DEFAULT
from tests.test_band_mover_table_gpu import _inputs, _opt, _run
from tests.test_band_resident_gpu import _values
from tests.test_band_wide_gpu import _bit_equal
from tests.test_gpu_parity import _mods

pytestmark = pytest.mark.gpu

CASES = [(200, 4, 2, 45, 1, None), (360, 6, 1, 33, 1, None), (1000, 10, 2, 70, 2, None), (200, 4, 2, 70, 1, 45)]
_base = {}


def _case(case):
    """structure, inputs and the outputs of mask 0, computed once per case"""
    if case not in _base:
        hipldl, syn, O = _mods()
        n, p, hw, B, kernel, active = case
        s = syn.band_structure(n, p, hw=hw)
        ladder, vals, rhs, ro = _inputs(syn, s, n, B)
        cfg0, out0 = _run(s, vals, rhs, ro, active=active, band_cache_policy=0, **_opt(hipldl, kernel))
        assert cfg0["band_mover_table"] and cfg0["band_cache_policy"] == 0 and cfg0["band_parts"] == (1 if kernel == 2 else 2)
        nb = B if active is None else active
        nf, ok = out0[5], out0[6]
        assert all(nf[b] > 1 for b in ladder if b < nb) and not ok[9] and ok[:nb].sum() == nb - 1
        _base[case] = (s, vals, rhs, ro, out0)
    return _base[case]


@pytest.mark.parametrize("mask", BUILT)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-p%d-hw%d-B%d-k%d-act%s" % c)
def test_every_policy_is_bit_equal_to_policy_zero(built, case, mask):
    """a last workgroup that is not full, ladder climbers, a problem no rho rescues, starts from rho_old > 0, one and two parts, an
    active prefix of 45 of 70 problems"""
    hipldl, syn, O = _mods()
    s, vals, rhs, ro, out0 = _case(case)
    cfg, out = _run(s, vals, rhs, ro, active=case[5], band_cache_policy=mask, **_opt(hipldl, case[4]))
    assert cfg["band"] and cfg["band_resident"] and cfg["band_mover_table"] and cfg["band_nl"] == 32
    assert cfg["band_cache_policy"] == mask
    assert _bit_equal(out, out0)


def test_the_default_handle_runs_the_shipped_default(built):
    hipldl, syn, O = _mods()
    s, vals, rhs, ro, out0 = _case(CASES[0])
    cfg, out = _run(s, vals, rhs, ro, **_opt(hipldl, 1))
    assert cfg["band_mover_table"] and cfg["band_cache_policy"] == DEFAULT
    assert _bit_equal(out, out0)


def test_other_instances_ignore_the_key(built):
    """a plan without a mover table (the resident instance) and a 16-problem handle: policy 0 reported whatever the key names, outputs
    those of policy 0"""
    hipldl, syn, O = _mods()
    mask = BUILT[-1]
    for s, extra in ((syn.band_structure(100, 2), {}), (syn.band_structure(200, 4), {"band_problems_per_group": 16})):
        vals, rhs = _values(syn, s, 40)
        opt = dict(_opt(hipldl, 1), **extra)
        cfg1, out1 = _run(s, vals, rhs, np.zeros(40), band_cache_policy=mask, **opt)
        cfg0, out0 = _run(s, vals, rhs, np.zeros(40), band_cache_policy=0, **opt)
        assert cfg1["band"] and not cfg1["band_mover_table"] and cfg1["band_cache_policy"] == 0 and cfg1 == cfg0
        assert out1[6].all() and _bit_equal(out1, out0)
