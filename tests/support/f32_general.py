"""What the tests of the Float32 general multifrontal kernel share (test infrastructure): the project's Float32 tolerances, the
inputs the tests name, the fp64 oracle on the widened float32 data, and the error measures — restated from
tests/test_float32_gpu.py, which stays as it is."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
BWD_TOL = 512 * EPS32     # backward error
FWD_TOL = 1e-3            # forward error against the oracle's d
MARGIN = 1e-3             # oracle pivots at least this far (relative to max |D|) from eig_tol: decisions cannot flip in float32

# the plan of a Float32 general handle, as Plan options (cnl_create_f32_ex forces the same switches internally)
GENERAL_PLAN = dict(plan_kind=1, condense=0, register_front=0, dense_backend=0, general_dense=0, staged=0, band_kernel=0)


def stack32(pairs):
    """[(vals, rhs), ...] -> float32 arrays [B][nnz], [B][N] (generator values rounded to float32)"""
    pairs = list(pairs)
    return (np.ascontiguousarray(np.stack([v for v, _ in pairs]), np.float32), np.ascontiguousarray(np.stack([r for _, r in pairs]), np.float32))


def random_inputs(syn, s, seeds, posdef=True):
    return stack32(syn.random_values(s, seed, posdef=posdef) for seed in seeds)


def band_inputs(syn, s, seeds, stress=None):
    return stack32(syn.band_values(s, seed, stress=stress) for seed in seeds)


def dense_inputs(syn, s, seeds):
    return stack32(syn.dense_values(s, seed) for seed in seeds)


def backward_error(s, vals, rhs, d):
    import scipy.sparse as sp
    rows, cols = s.kkt_pattern()
    Kl = sp.coo_matrix((np.asarray(vals, np.float64), (rows - 1, cols - 1)), shape=(s.N, s.N)).tocsr()
    K = Kl + sp.tril(Kl, -1).T
    d, rhs = np.asarray(d, np.float64), np.asarray(rhs, np.float64)
    res = K @ d + rhs
    return np.abs(res).max() / (abs(K).sum(axis=1).max() * np.abs(d).max() + np.abs(rhs).max())


_ORACLES = {}


def oracle_of(O, s):
    key = (s.name, s.nvar, s.nequ, s.ncon, s.nnzNS)
    if key not in _ORACLES:
        rows, cols = s.kkt_pattern()
        _ORACLES[key] = O.Oracle(s.N, rows, cols, O.canonical_perm(s.nvar, s.nequ, s.ncon))
    return _ORACLES[key]


def oracle_newton(O, s, vals32, rhs32, rho_old32, p32):
    """the fp64 oracle on the widened Float32 data with ParamCaNNOLeS(Float32) widened; asserts the pivot margin of every problem's
    last factorisation"""
    orc = oracle_of(O, s)
    p64 = np.asarray(p32, np.float32).astype(np.float64)
    B = vals32.shape[0]
    out = {"d": np.zeros((B, s.N)), "ok": np.zeros(B, bool), "rho": np.zeros(B), "ro": np.zeros(B), "nf": np.zeros(B, np.int64),
           "vals": vals32.astype(np.float64)}
    for b in range(B):
        d, ok, rho, ro, nf = O.newton_system(orc, s.nvar, s.nequ, s.ncon, rhs32[b].astype(np.float64), out["vals"][b], float(rho_old32[b]), p64)
        D = orc.D
        margin = np.abs(np.abs(D) - p64[0]).min()
        assert margin >= MARGIN * np.abs(D).max(), f"problem {b}: an oracle pivot lies within {margin:.3g} of eig_tol"
        out["d"][b], out["ok"][b], out["rho"][b], out["ro"][b], out["nf"][b] = d, ok, rho, ro, nf
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_results(s, ref, vals32_out, rhs32, d, ok, rho, ro, nf, rows=None):
    """decisions identical, rho / rho_old / rho slots bit-equal to the oracle's rounded to float32, errors within the tolerances;
    returns the largest backward and forward error seen"""
    B = rhs32.shape[0]
    d = np.asarray(d).reshape(B, s.N)
    assert np.array_equal(np.asarray(ok, bool).reshape(B), ref["ok"])
    assert np.array_equal(np.asarray(nf, np.int64).reshape(B), ref["nf"])
    assert np.array_equal(bits(rho).reshape(B), bits(ref["rho"]))
    assert np.array_equal(bits(ro).reshape(B), bits(ref["ro"]))
    assert np.array_equal(bits(np.asarray(vals32_out).reshape(B, -1)[:, -s.nvar:]), bits(ref["vals"][:, -s.nvar:]))
    worst_b = worst_f = 0.0
    for b in (range(B) if rows is None else rows):
        if ref["ok"][b]:
            be = backward_error(s, np.asarray(vals32_out).reshape(B, -1)[b], rhs32[b], d[b])
            fe = np.abs(d[b] - ref["d"][b]).max() / np.abs(ref["d"][b]).max()
            assert be <= BWD_TOL, (b, be)
            assert fe <= FWD_TOL, (b, fe)
            worst_b, worst_f = max(worst_b, be), max(worst_f, fe)
    return worst_b, worst_f
