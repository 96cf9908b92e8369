"""The epoch-block look-ahead of the mover-table instance of the band kernel on the GPU (csrc/band.hip: ebk).  -m gpu.

The instance loads the block of the epoch two ahead into a register and hands its fields out with v_readlane; the resident instance
(tuning band_mover_table = 0) reads every field where it needs it.  Same program, same arithmetic: on one handle configuration the
two must agree bit for bit in everything they write — d, rho, rho_old, nfact, success, success of try_to_factorize, d of solve_ldl!
and `vals` with the rho slots written back — in newton_system!, in try_to_factorize + solve_ldl!, and in a second newton_system! on
the same handle (which starts from the rho_old and the rho slots the first left).  Every array has sentinels behind it that must
survive.  The shapes sit on the ends of a sweep, where a look-ahead can read the wrong block or past the last one; what each is
there for is asserted from the plan in tests/test_band_epoch_lookahead_cpu.py."""
import numpy as np
import pytest

from tests.test_band_epoch_lookahead_cpu import CASES, IDS
from tests.test_band_resident_gpu import _values
from tests.test_gpu_parity import _mods

pytestmark = pytest.mark.gpu

PAD = 64            # sentinel elements behind every array
SENT_F, SENT_I = -777.25, -7777
NAMES = ("success of try_to_factorize", "d of solve_ldl!", "d", "rho_old", "rho", "nfact", "success", "d (second call)", "rho_old (second call)",
         "rho (second call)", "nfact (second call)", "success (second call)", "vals")


def _padded(torch, dev, n, fill, dtype):
    """(the first n elements, the whole buffer) of a device array of n elements `fill` with PAD sentinels behind"""
    buf = torch.full((n + PAD,), SENT_I if dtype == torch.int32 else SENT_F, dtype=dtype, device=dev)
    buf[:n] = fill
    return buf[:n], buf


def _run(s, vals, rhs, ro_h, **opt):
    import torch
    hipldl, syn, O = _mods()
    rows, cols = s.kkt_pattern()
    B, N = vals.shape[0], s.N
    dev = torch.device("cuda", 0)
    L = hipldl.HIPLDLStruct(N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, options=hipldl.Options(**opt))
    cfg = dict(L.config)
    p_ = hipldl.default_params(np.float64)
    f64, i32 = torch.float64, torch.int32
    bufs = []

    def arr(n, fill, dtype=f64):
        a, whole = _padded(torch, dev, n, fill, dtype)
        bufs.append((n, whole))
        return a

    tv, tr = arr(B * vals.shape[1], 0.0), arr(B * N, 0.0)
    tv.copy_(torch.from_numpy(vals).reshape(-1))
    tr.copy_(torch.from_numpy(rhs).reshape(-1))
    tin = arr(hipldl.layout_len(L, 0), 9.0)
    hipldl.interleave_dev(L, 0, tv, tin)
    su, d2 = arr(B, -5, i32), arr(B * N, 7.0)
    hipldl.factorize_dev(L, tin, float(p_[0]), su)
    hipldl.solve_dev(L, tr, d2)
    outs = [su, d2]
    ro = arr(B, 0.0)
    ro.copy_(torch.from_numpy(ro_h))
    for call in range(2):   # the second call starts from the first's rho_old, with the rho slots the first wrote
        d, rho, nf, ok = arr(B * N, 3.0), arr(B, -1.0), arr(B, -5, i32), arr(B, -5, i32)
        hipldl.newton_system_dev(L, tin, tr, d, ro, rho, nf, ok, p_)
        torch.cuda.synchronize()
        outs += [d, ro.clone(), rho, nf, ok]
    outs.append(tin)
    out = [x.cpu().numpy() for x in outs]
    for n, whole in bufs:
        tail = whole[n:].cpu().numpy()
        assert (tail == (SENT_I if whole.dtype == i32 else SENT_F)).all(), "a sentinel behind an array was overwritten"
    L.close()
    return cfg, out


def _opt(hipldl):
    return dict(plan_kind=hipldl.PLAN_THROUGHPUT, batch_layout=hipldl.LAYOUT_INTERLEAVED, band_problems_per_group=32, band_kernel=1)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lookahead_is_bit_equal_to_the_resident_instance(built, case):
    hipldl, syn, O = _mods()
    s = syn.band_structure(case["n"], case["p"], hw=case["hw"])
    B, ladder = case["B"], case["ladder"]
    vals, rhs = _values(syn, s, B, cfg=4, ladder=ladder)
    ro = np.zeros(B)
    ro[B // 2] = 0.3   # a start from rho_old > 0
    cfg1, out1 = _run(s, vals, rhs, ro, **_opt(hipldl))
    cfg0, out0 = _run(s, vals, rhs, ro, band_mover_table=0, **_opt(hipldl))
    assert cfg1["band"] and cfg1["band_resident"] and cfg1["band_mover_table"] and cfg1["band_nl"] == 32 and cfg1["batch_layout"] == 1
    assert cfg0["band"] and cfg0["band_resident"] and not cfg0["band_mover_table"] and cfg0["band_nl"] == 32 and not cfg0["float32"]
    nf, ok = out1[5], out1[6]
    assert ok.all() and all(nf[b] > 1 for b in ladder) and all(nf[b] == 1 for b in range(B) if b not in ladder and b != B // 2)
    for name, x, y in zip(NAMES, out1, out0):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
