"""The resident form of the band program on the GPU (csrc/band.hip: the BAND_NPIECE_RESIDENT instance).  -m gpu.

Same steps, same arithmetic, same summation order as the 15-piece program: one handle configuration run with the resident program
(the default where it qualifies: Float64, `vals` interleaved, 32 problems per workgroup) and with tuning band_resident = 0 must
give every output bit for bit — success of try_to_factorize, d of solve_ldl!, d, rho_old, rho, nfact, success of newton_system!
and the rho slots written back to `vals`."""
import numpy as np
import pytest

from tests.test_band_wide_gpu import _bit_equal, _run_dev
from tests.test_gpu_parity import _mods

pytestmark = pytest.mark.gpu


def _values(syn, s, B, cfg=4, ladder=(), hopeless=None):
    vals, rhs = syn.batch_values(s, B, cfg=cfg)
    for b in ladder:
        vals[b], rhs[b] = syn.band_values(s, 5000 + b, stress="ladder")
    if hopeless is not None:
        vals[hopeless, s.offsets()[0]] = -1e300
    return vals, rhs


@pytest.mark.parametrize("n,p,hw,B,kernel", [(200, 4, 2, 45, 1), (400, 4, 2, 100, 1), (1000, 10, 2, 70, 2), (360, 6, 1, 33, 1), (10000, 50, 2, 70, 1)])
def test_resident_program_is_bit_equal_to_the_fifteen_piece_one(built, n, p, hw, B, kernel):
    """batches that are no multiple of 32 (the last workgroup is partly empty), ladder climbers (the forward sweep runs again from
    its first epoch, nfact = 6), a problem no rho rescues, starts from rho_old > 0, one and two parts"""
    hipldl, syn, O = _mods()
    s = syn.band_structure(n, p, hw=hw)
    ladder = (1, 5, 17, 31, B - 1)
    vals, rhs = _values(syn, s, B, cfg=3 if n >= 10000 else 4, ladder=ladder, hopeless=9)
    ro = np.zeros(B)
    ro[5] = 0.3
    ro[2] = 1e-3
    opt = dict(plan_kind=hipldl.PLAN_THROUGHPUT, batch_layout=hipldl.LAYOUT_INTERLEAVED, band_problems_per_group=32, band_kernel=kernel)
    cfg1, out1 = _run_dev(s, vals, rhs, ro, **opt)
    cfg0, out0 = _run_dev(s, vals, rhs, ro, band_resident=0, **opt)
    assert cfg1["band"] and cfg1["band_resident"] and cfg1["band_nl"] == 32 and cfg1["batch_layout"] == 1 and cfg1["band_pieces"] == 15
    assert cfg0["band"] and not cfg0["band_resident"] and cfg0["band_nl"] == 32
    nf, ok = out1[5], out1[6]
    assert all(nf[b] > 1 for b in ladder) and ok[list(ladder)].all() and not ok[9] and ok.sum() == B - 1
    assert _bit_equal(out1, out0)


def test_only_qualifying_handles_run_the_resident_program(built):
    """problem-major `vals`, 16 problems per workgroup and Float32 keep the 15-piece program"""
    hipldl, syn, O = _mods()
    s = syn.band_structure(200, 4)
    vals, rhs = _values(syn, s, 40)
    ro = np.zeros(40)
    base = dict(plan_kind=hipldl.PLAN_THROUGHPUT)
    for opt, dtype in ((dict(band_problems_per_group=32), np.float64), (dict(batch_layout=hipldl.LAYOUT_INTERLEAVED), np.float64),
                       (dict(batch_layout=hipldl.LAYOUT_INTERLEAVED, band_problems_per_group=32), np.float32)):
        cfg, out = _run_dev(s, vals, rhs, ro, dtype=dtype, **base, **opt)
        assert cfg["band"] and not cfg["band_resident"], (opt, cfg)
        assert out[6].all()
