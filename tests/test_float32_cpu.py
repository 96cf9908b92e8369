"""Float32 on the band kernels, without a GPU: ParamCaNNOLeS(Float32) bit for bit, the exported symbols, and the band program
for 4-byte elements — word for word the 8-byte one, with every LDS byte offset halved (csrc/band.h, build_band_plan's esz)."""
import ctypes as C

import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn

# ParamCaNNOLeS(Float32) (src/CaNNOLeS.jl:48-62): eig_tol, dmin, kdec, kinc, klargeinc (= sizeof(Float32) * 16), rho0, rhomax,
# rhomin, gammaA — what Julia computes on Float32 operands
F32_PARAMS = [0x34000000, 0x39b504f3, 0x3eaaaaab, 0x41000000, 0x42800000, 0x3ba14516, 0x56800000, 0x39b504f3, 0x3c9837f0]

F32_SYMBOLS = ["cnl_default_params_f32", "cnl_create_f32", "cnl_create_f32_ex", "cnl_factorize_f32", "cnl_solve_f32", "cnl_newton_system_f32",
               "cnl_factorize_f32_dev", "cnl_solve_f32_dev", "cnl_newton_system_f32_dev", "cnl_interleave_f32_dev", "cnl_deinterleave_f32_dev"]

# step block (band.h): word 0 flags, words BS_DG0 .. BS_DX LDS byte offsets, BS_BORDER a table index; every word of a row block is
# an LDS byte offset
BAND_SW, BAND_RW, BS_DG0, BS_DX = 20, 8, 1, 18


def test_default_params_f32_bit_patterns(built):
    p = np.zeros(9, np.float32)
    hipldl.lib().cnl_default_params_f32(p.ctypes.data)
    assert p.view(np.uint32).tolist() == F32_PARAMS
    q = hipldl.default_params(np.float32)
    assert q.dtype == np.float32 and q.view(np.uint32).tolist() == F32_PARAMS
    assert np.array_equal(hipldl.default_params(), hipldl.default_params(np.float64))
    with pytest.raises(TypeError):
        hipldl.default_params(np.float16)


def test_float32_symbols_are_exported_and_listed(built):
    lib = C.CDLL(hipldl.LIB_PATH)
    for sym in F32_SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in hipldl.ABI_SYMBOLS, sym


def _offset_mask(stream, nsteps):
    """positions of the LDS-offset words in a fops / bops stream of nsteps step blocks (the padding behind them: none)"""
    mask = np.zeros(len(stream), bool)
    o = 0
    for _ in range(nsteps):
        rows = (int(stream[o]) >> 8) & 255
        mask[o + BS_DG0:o + BS_DX + 1] = True
        mask[o + BAND_SW:o + BAND_SW + BAND_RW * rows] = True
        o += BAND_SW + BAND_RW * rows
    return mask, o


@pytest.mark.parametrize("shape,opt", [
    ((10000, 50, 2), {}),                 # cfg3 (the headline pattern)
    ((1000, 10, 2), {}),                  # cfg4
    ((200, 0, 2), {}),                    # no constraints
    ((360, 6, 1), {}),                    # half-width 1
    ((1000, 10, 2), {"band_kernel": 2}),  # one part
])
def test_four_byte_program_is_the_eight_byte_one_with_halved_offsets(built, shape, opt):
    n, p, hw = shape
    s = syn.band_structure(n, p, hw=hw)
    rows, cols = s.kkt_pattern()
    pl = hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT, **opt))
    info8, info4 = pl.array("band_info"), pl.array("band4_info")
    assert info8[0] == 1 and np.array_equal(info8, info4)
    nparts = int(info8[1])
    assert nparts == (1 if opt.get("band_kernel") == 2 else 2)
    checked = 0
    for q in range(nparts):
        part8, part4 = pl.array(f"band_part{q}"), pl.array(f"band4_part{q}")
        assert np.array_equal(part8, part4)
        for k in ("epochs", "borders"):   # element indices and flags: no LDS offsets
            assert np.array_equal(pl.array(f"band_{k}{q}"), pl.array(f"band4_{k}{q}"))
        for k in ("fops", "bops"):
            a8, a4 = pl.array(f"band_{k}{q}"), pl.array(f"band4_{k}{q}")
            assert a8.shape == a4.shape
            mask, used = _offset_mask(a8, int(part8[0]))
            assert np.array_equal(a8[~mask], a4[~mask])
            off8, off4 = a8[mask], a4[mask]
            assert (off8 % 8 == 0).all() and (off8 >= 0).all()
            assert np.array_equal(off8 // 2, off4)
            assert not a8[used:].any() and not a4[used:].any()
            checked += int(mask.sum())
    assert checked > 0


def test_no_band_no_four_byte_program(built):
    """a pattern the band kernels do not serve has neither program (cnl_create_f32 then fails: the caller stays on the CPU)"""
    s = syn.random_structure(60, 80, 4, 0.1, seed=3)
    rows, cols = s.kkt_pattern()
    pl = hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT))
    assert pl.array("band_info")[0] == 0 and pl.array("band4_info")[0] == 0
