"""The mover-table instance of the band kernel on the GPU (csrc/band.hip: BAND_NPIECE_MOVER).  -m gpu.

It runs the resident program with every piece's address taken from the host-built table instead of decoded from a descriptor: same
loads, same slots, same steps.  One handle configuration run with the table (the default where the plan has one) and with tuning
band_mover_table = 0 (the resident instance) must give every output bit for bit — success of try_to_factorize, d of solve_ldl!, d,
rho_old, rho, nfact, success of newton_system! and `vals` with the rho slots written back."""
import numpy as np
import pytest

from tests.test_band_resident_gpu import _values
from tests.test_band_wide_gpu import _bit_equal
from tests.test_gpu_parity import _mods

pytestmark = pytest.mark.gpu


def _run(s, vals, rhs, ro_h, active=None, **opt):
    """try_to_factorize -> solve_ldl!, then newton_system! on device arrays of one handle, `vals` interleaved; active: the handle works
    on its first `active` problems (cnl_set_active_batch) — the arrays keep the created batch's size and the rows behind stay untouched"""
    import torch
    hipldl, syn, O = _mods()
    rows, cols = s.kkt_pattern()
    B = vals.shape[0]
    dev = torch.device("cuda", 0)
    L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, options=hipldl.Options(**opt))
    cfg = dict(L.config)
    p_ = hipldl.default_params(np.float64)
    tv, tr = torch.from_numpy(vals).to(dev), torch.from_numpy(rhs).to(dev)
    tin = torch.full((hipldl.layout_len(L, 0),), 9.0, dtype=torch.float64, device=dev)
    hipldl.interleave_dev(L, 0, tv, tin)
    if active is not None:
        hipldl.set_active_batch(L, active)
    su = torch.full((B,), -5, dtype=torch.int32, device=dev)
    d2 = torch.full((B, s.N), 7.0, dtype=torch.float64, device=dev)
    hipldl.factorize_dev(L, tin, float(p_[0]), su)
    hipldl.solve_dev(L, tr, d2)
    d = torch.full((B, s.N), 3.0, dtype=torch.float64, device=dev)
    ro, rho = torch.from_numpy(ro_h.copy()).to(dev), torch.full((B,), -1.0, dtype=torch.float64, device=dev)
    nf, ok = torch.full((B,), -5, dtype=torch.int32, device=dev), torch.full((B,), -5, dtype=torch.int32, device=dev)
    hipldl.newton_system_dev(L, tin, tr, d, ro, rho, nf, ok, p_)
    torch.cuda.synchronize()
    out = [x.cpu().numpy() for x in (su, d2, d, ro, rho, nf, ok, tin)]
    L.close()
    return cfg, out


def _opt(hipldl, kernel):
    return dict(plan_kind=hipldl.PLAN_THROUGHPUT, batch_layout=hipldl.LAYOUT_INTERLEAVED, band_problems_per_group=32, band_kernel=kernel)


def _inputs(syn, s, n, B):
    ladder = (1, 5, 17, 31, B - 1)
    vals, rhs = _values(syn, s, B, cfg=3 if n >= 10000 else 4, ladder=ladder, hopeless=9)
    ro = np.zeros(B)
    ro[5] = 0.3
    ro[2] = 1e-3
    return ladder, vals, rhs, ro


@pytest.mark.parametrize("n,p,hw,B,kernel", [(200, 4, 2, 45, 1), (400, 4, 2, 100, 1), (1000, 10, 2, 70, 2), (360, 6, 1, 33, 1), (10000, 50, 2, 70, 1)])
def test_mover_table_is_bit_equal_to_the_resident_instance(built, n, p, hw, B, kernel):
    """batches that are no multiple of 32, ladder climbers, a problem no rho rescues, starts from rho_old > 0, one and two parts"""
    hipldl, syn, O = _mods()
    s = syn.band_structure(n, p, hw=hw)
    ladder, vals, rhs, ro = _inputs(syn, s, n, B)
    cfg1, out1 = _run(s, vals, rhs, ro, **_opt(hipldl, kernel))
    cfg0, out0 = _run(s, vals, rhs, ro, band_mover_table=0, **_opt(hipldl, kernel))
    assert cfg1["band"] and cfg1["band_resident"] and cfg1["band_mover_table"] and cfg1["band_nl"] == 32 and cfg1["batch_layout"] == 1
    assert cfg0["band"] and cfg0["band_resident"] and not cfg0["band_mover_table"] and cfg0["band_nl"] == 32 and not cfg0["float32"]
    nf, ok = out1[5], out1[6]
    assert all(nf[b] > 1 for b in ladder) and ok[list(ladder)].all() and not ok[9] and ok.sum() == B - 1
    assert _bit_equal(out1, out0)


def test_mover_table_on_an_active_prefix_of_the_batch(built):
    """cnl_set_active_batch to 45 of 70 problems: the second workgroup holds 13 problems, the rows behind the prefix keep what they held"""
    hipldl, syn, O = _mods()
    s = syn.band_structure(200, 4)
    B, nb = 70, 45
    ladder, vals, rhs, ro = _inputs(syn, s, 200, B)
    cfg1, out1 = _run(s, vals, rhs, ro, active=nb, **_opt(hipldl, 1))
    cfg0, out0 = _run(s, vals, rhs, ro, active=nb, band_mover_table=0, **_opt(hipldl, 1))
    assert cfg1["band_mover_table"] and cfg0["band_resident"] and not cfg0["band_mover_table"]
    su, d2, d, _, rho, nf, ok, _ = out1
    assert (su[nb:] == -5).all() and (d2[nb:] == 7.0).all() and (d[nb:] == 3.0).all() and (rho[nb:] == -1.0).all() and (nf[nb:] == -5).all() and (ok[nb:] == -5).all()
    assert all(nf[b] > 1 for b in (1, 5, 17, 31)) and not ok[9] and ok[:nb].sum() == nb - 1
    assert _bit_equal(out1, out0)
    # ... and the prefix is what the whole batch gives for those problems
    _, full = _run(s, vals, rhs, ro, **_opt(hipldl, 1))
    assert all(np.array_equal(x[:nb], y[:nb]) for x, y in zip(out1[:7], full[:7]))


def test_a_plan_without_a_table_stays_on_the_resident_instance(built):
    """a pattern whose epochs do not fit the typed sets (tests/test_band_mover_table_cpu.py); 16 problems per workgroup"""
    hipldl, syn, O = _mods()
    s = syn.band_structure(100, 2)
    vals, rhs = _values(syn, s, 40)
    cfg, out = _run(s, vals, rhs, np.zeros(40), **_opt(hipldl, 1))
    assert cfg["band_resident"] and not cfg["band_mover_table"] and out[6].all()
    s = syn.band_structure(200, 4)
    vals, rhs = _values(syn, s, 40)
    cfg, out = _run(s, vals, rhs, np.zeros(40), **dict(_opt(hipldl, 1), band_problems_per_group=16))
    assert cfg["band"] and not cfg["band_resident"] and not cfg["band_mover_table"] and out[6].all()
