"""Float32 rows f1 / f2 / f4 and the trial point, without a GPU: the exported `_f32_dev` symbols, their refusal of a null handle, and
tests/support/f32_rows.py (the float32 restatement the GPU tests compare against) pinned bit for bit to the fp64 oracle on inputs
where float32 arithmetic is exact (small dyadic values)."""
import ctypes as C

import numpy as np

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn
from oracle import oracle as O
from tests.support import f32_rows as R

ROW_SYMBOLS = ["cnl_prepare_newton_system_f32_dev", "cnl_residual_vectors_f32_dev", "cnl_residual_vectors_jac_f32_dev",
               "cnl_cgls_multipliers_f32_dev", "cnl_cgls_multipliers_jac_f32_dev", "cnl_trial_point_f32_dev"]
CNL_ERR_ARG = 1


def test_row_symbols_are_exported_and_listed(built):
    lib = C.CDLL(hipldl.LIB_PATH)
    for sym in ROW_SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym in hipldl.ABI_SYMBOLS, sym


def test_null_handle_is_refused(built):
    lib = hipldl.lib()
    buf = np.zeros(256, np.float32)
    a = buf.ctypes.data
    calls = [
        lambda: lib.cnl_prepare_newton_system_f32_dev(None, 0, 0, 1, 0, a, a, a, a, a, a, None),
        lambda: lib.cnl_residual_vectors_f32_dev(None, a, a, a, a, a, a, a, None),
        lambda: lib.cnl_residual_vectors_jac_f32_dev(None, 1, 1, a, a, a, a, a, a, a, a, None),
        lambda: lib.cnl_cgls_multipliers_f32_dev(None, a, a, a, None, 1e-4, 1e-4, 0, 1, None, None),
        lambda: lib.cnl_cgls_multipliers_jac_f32_dev(None, 1, 1, a, a, a, a, None, 1e-4, 1e-4, 0, 1, None, None),
        lambda: lib.cnl_trial_point_f32_dev(None, a, a, a, a, 1e4, a, a, a, a, None),
    ]
    for call in calls:
        assert call() == CNL_ERR_ARG
    assert not buf.any()


def _dyadic(rng, *shape):
    """k / 4 for small integers k: products and short sums stay exact in float32"""
    return rng.integers(-8, 9, shape).astype(np.float64) / 4


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_restated_prepare_and_f1_are_the_oracle_on_exact_inputs():
    for ncon in (2, 0):
        s = syn.band_structure(24, ncon)
        rows, cols = s.kkt_pattern()
        rng = np.random.default_rng(11 + ncon)
        B = 3
        old = _dyadic(rng, B, s.nnzNS)
        hF, hc, Jx, Jcx = _dyadic(rng, B, s.nnzhF), _dyadic(rng, B, s.nnzhc), _dyadic(rng, B, s.nnzjF), _dyadic(rng, B, s.nnzjc)
        hc[:, ::3] = 0.0   # -0.0 in H_c
        delta = np.abs(_dyadic(rng, B))
        delta[0] = 0.0
        r, lam, Fx, cx = _dyadic(rng, B, s.nequ), _dyadic(rng, B, s.ncon), _dyadic(rng, B, s.nequ), _dyadic(rng, B, s.ncon)
        for hess in (True, False):
            got = R.prepare(old.astype(np.float32), s.nvar, s.nequ, s.ncon, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc,
                            hF if hess else None, hc, Jx, Jcx, delta)
            for b in range(B):
                want = old[b].copy()
                O.prepare(want, s.nvar, s.nequ, s.ncon, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, hF[b] if hess else None, hc[b], Jx[b], Jcx[b],
                          float(delta[b]))
                assert np.array_equal(_bits(got[b]), _bits(want)), (ncon, hess, b)
        vals = got
        rhs, nrm = R.residual_vectors(rows, cols, vals, s.nvar, s.nequ, s.ncon, r, lam, Fx, cx)
        assert rhs.dtype == np.float32 and nrm.dtype == np.float32
        for b in range(B):
            rhs0, n0 = O.residual_vectors(rows, cols, vals[b].astype(np.float64), s.nvar, s.nequ, s.ncon, r[b], lam[b], Fx[b], cx[b])
            assert np.array_equal(_bits(rhs[b]), _bits(rhs0)), (ncon, b)
            assert np.array_equal(_bits(nrm[b]), _bits(n0)), (ncon, b)
        # a NaN in r reaches the dual part and both norms, as norm(., Inf) propagates it
        r2 = r.copy()
        r2[1, 5] = np.nan
        rhs, nrm = R.residual_vectors(rows, cols, vals, s.nvar, s.nequ, s.ncon, r2, lam, Fx, cx)
        rhs0, n0 = O.residual_vectors(rows, cols, vals[1].astype(np.float64), s.nvar, s.nequ, s.ncon, r2[1], lam[1], Fx[1], cx[1])
        assert np.array_equal(np.isnan(rhs[1]), np.isnan(rhs0)) and np.isnan(rhs[1, :s.nvar]).any()
        assert np.isnan(nrm[1]).all() and np.isnan(n0).all()


def test_restated_trial_point_is_the_oracle_on_exact_inputs():
    s = syn.band_structure(24, 2)
    rng = np.random.default_rng(5)
    B = 4
    x, r, lam, d = _dyadic(rng, B, s.nvar), _dyadic(rng, B, s.nequ), _dyadic(rng, B, s.ncon), _dyadic(rng, B, s.N)
    # dlambda = -(3k, 4k) * 1000: norms 5000 k, the cap 1e4 applies for k >= 3 (exact quotients)
    for b, k in enumerate((1, 2, 3, 4)):
        d[b, s.nvar + s.nequ:] = [3000.0 * k, 4000.0 * k]
    xt, rt, lt, dl = R.trial_point(s.nvar, s.nequ, s.ncon, x, r, lam, d, 1e4)
    capped = 0
    for b in range(B):
        xt0, rt0, lt0, dl0 = O.trial_point(s.nvar, s.nequ, s.ncon, x[b], r[b], lam[b], d[b], 1e4)
        for got, want in ((xt[b], xt0), (rt[b], rt0), (lt[b], lt0), (dl[b], dl0)):
            assert np.array_equal(_bits(got), _bits(want)), b
        capped += not np.array_equal(dl0, -d[b, s.nvar + s.nequ:])
    assert capped == 2


def test_restated_cgls_is_the_oracle_on_exact_inputs():
    """one constraint whose Jacobian row has four entries of 1 (A'A = 4): CGLS ends after one step with alpha = 1/4, exactly"""
    s = syn.band_structure(24, 1)
    rows, cols = s.kkt_pattern()
    off = s.offsets()
    rng = np.random.default_rng(9)
    for b in range(3):
        vals = _dyadic(rng, s.nnzNS)
        vals[off[3]:off[4]] = 0.0
        vals[off[3] + np.array([1, 5, 6, 20])] = 1.0
        r = _dyadic(rng, s.nequ)
        lam, jt, it, margin = R.cgls_multipliers(rows, cols, vals, s.nvar, s.nequ, s.ncon, r)
        lam0, jt0, it0 = O.cgls_multipliers(rows, cols, vals, s.nvar, s.nequ, s.ncon, r)
        assert it == it0 == 1 and margin > 0
        assert np.array_equal(_bits(jt), _bits(jt0)) and np.array_equal(_bits(lam), _bits(lam0)), b
    # r = 0: no step, lambda = 1
    lam, jt, it, _ = R.cgls_multipliers(rows, cols, vals, s.nvar, s.nequ, s.ncon, np.zeros(s.nequ))
    lam0, jt0, it0 = O.cgls_multipliers(rows, cols, vals, s.nvar, s.nequ, s.ncon, np.zeros(s.nequ))
    assert it == it0 == 0 and np.array_equal(lam, np.ones(1, np.float32)) and np.array_equal(lam0, np.ones(1))
