"""What the tests of the Float32 dense backend share (tests/test_float32_dense_cpu.py, tests/test_float32_dense_gpu.py): numpy only.

Inputs are those of tests/support/dense_cases.py (its `structure`, `values` and SHAPES, seed 1, MIX = 5) rounded to float32.  The
float kernels (csrc/dense_f32.hip) keep every size of the double kernels — tile 64, macro tile 128, row chunk 16, 2048-row rounds of
the right-hand-side kernel, 7 row tiles per ladder pass, 3 row tiles per panel workgroup — so those shapes are the smallest at each
of their edges too, and no shape is added.

The reference is the fp64 oracle on the widened float32 data with ParamCaNNOLeS(Float32) widened, on the canonical order, through
the batch entry that takes the NaN problem.  What vouches for the decisions is order-independent: a factorisation of the KKT matrix
succeeds (n positive, m + p negative pivots, none zero) exactly when the Schur complement onto the variables
    M(rho) = H + rho I + J' W J + Jc' Jc / delta         (W = -1 / d_r > 0, -delta the diagonal of the constraint block)
is positive definite, and `eig_margins` gives, for every rung of every problem that is not hopeless, lambda_min(M(rho)) relative to
the largest |eigenvalue|: the CPU test requires 1e-3 with the right sign, three orders above what float32 rounding of an order-470
system (470 eps32 = 6e-5) can move.
"""
import numpy as np

from tests.support import dense_cases as dc
from tests.support import f32_general as G

EPS32, BWD_TOL, FWD_TOL, bits = G.EPS32, G.BWD_TOL, G.FWD_TOL, G.bits
EIG_MARGIN = 1e-3
SHAPES, TALL, MIX, SEED, GRAPH_CASE, shape_id = dc.SHAPES, dc.TALL, dc.MIX, dc.SEED, dc.GRAPH_CASE, dc.shape_id
OPTIONS = dict(float32_general=1, float32_dense=1)

_cache = {}


def params32():
    """ParamCaNNOLeS(Float32) as the library states it (cnl_default_params_f32)"""
    from cannoles_jl_amd import hipldl
    return hipldl.default_params(np.float32)


def case(shape, B=MIX, seed=SEED):
    """The float32 case and what the fp64 oracle makes of it, computed once per session and shared (read-only):
    dict(s, rows, cols, vals, rhs, rho_old [float32], p32, d, ok, rho, ro, nf, vals_after [the oracle's, float64])."""
    key = (shape, B, seed)
    if key not in _cache:
        from oracle import oracle as O
        s = dc.structure(*shape, seed)
        rows, cols = s.kkt_pattern()
        v64, r64, ro64 = dc.values(s, B, seed)
        vals, rhs, ro = (np.ascontiguousarray(a, np.float32) for a in (v64, r64, ro64))
        p32 = params32()
        orc = O.Oracle(s.N, rows, cols, O.canonical_perm(s.nvar, s.nequ, s.ncon))
        va = vals.astype(np.float64)
        d, ok, rho, rold, nf = O.newton_system_batch(orc, B, s.nvar, s.nequ, s.ncon, rhs.astype(np.float64), va, ro.astype(np.float64),
                                                     p32.astype(np.float64))
        c = dict(s=s, rows=rows, cols=cols, vals=vals, rhs=rhs, rho_old=ro, p32=p32, d=d, ok=np.asarray(ok, bool), rho=rho, ro=rold,
                 nf=np.asarray(nf, np.int64), vals_after=va)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def blocks(s, vals):
    """(H, J, dr, Jc, delta) of one problem as dense float64 blocks of the KKT matrix, the rho slots left out of H"""
    n, m, p = s.nvar, s.nequ, s.ncon
    rows, cols = s.kkt_pattern()
    v = np.array(vals, np.float64)
    v[-n:] = 0.0
    K = np.zeros((s.N, s.N))
    np.add.at(K, (rows - 1, cols - 1), v)
    K = K + np.tril(K, -1).T
    return K[:n, :n], K[n:n + m, :n], np.diag(K[n:n + m, n:n + m]).copy(), K[n + m:, :n], -np.diag(K[n + m:, n + m:]).copy()


def eig_margins(c, b):
    """[(rho, lambda_min(M(rho)) / max |lambda(M(rho))|, expected success)] for every rung problem b climbed (by the oracle's nfact)"""
    s = c["s"]
    H, J, dr, Jc, delta = blocks(s, c["vals"][b])
    M0 = H + J.T @ (J * (-1.0 / dr)[:, None]) + (Jc.T @ (Jc / delta[:, None]) if s.ncon else 0.0)
    lam = np.linalg.eigvalsh(M0)
    rungs = dc.rungs(float(c["rho_old"][b]), int(c["nf"][b]), c["p32"].astype(np.float64))
    out = []
    for k, rho in enumerate(rungs):
        lo, hi = lam[0] + rho, max(abs(lam[0] + rho), abs(lam[-1] + rho))
        out.append((rho, lo / hi, bool(c["ok"][b]) and k == len(rungs) - 1))
    return out


def emulate32(s, vals32, rhs32):
    """The dense backend's arithmetic in plain numpy float32, one healthy problem: S = [H + J'WJ, Jc'; Jc, -delta I] formed in float32,
    LDL' without pivoting, both sweeps, the residual components recovered from J x.  Returns d (float32)."""
    n, m, p = s.nvar, s.nequ, s.ncon
    f = np.float32
    H, J, dr, Jc, delta = (np.asarray(a, f) for a in blocks(s, vals32))
    w = (f(-1.0) / dr).astype(f)
    ns = n + p
    S = np.zeros((ns, ns), f)
    S[:n, :n] = H + (J.T @ (J * w[:, None])).astype(f)
    if p:
        S[n:, :n] = Jc
        S[:n, n:] = Jc.T
        S[n:, n:] = -np.diag(delta)
    r = np.asarray(rhs32, f)
    y = np.concatenate([r[:n] + J.T @ (w * r[n:n + m]), r[n + m:]]).astype(f)
    A = S.copy()
    L = np.eye(ns, dtype=f)
    D = np.zeros(ns, f)
    for j in range(ns):
        D[j] = A[j, j]
        l = (A[j + 1:, j] / D[j]).astype(f)
        L[j + 1:, j] = l
        A[j + 1:, j + 1:] -= np.outer(l, A[j + 1:, j]).astype(f)
    z = y.copy()
    for j in range(ns):
        z[j + 1:] -= L[j + 1:, j] * z[j]
    z = (z / D).astype(f)
    for j in range(ns - 1, -1, -1):
        z[j] -= L[j + 1:, j] @ z[j + 1:]
    x = z
    return np.concatenate([-x[:n], w * (r[n:n + m] - (J @ x[:n]).astype(f)), -x[n:]]).astype(f)


def check_outputs(c, out, idx, vals_in):
    """One call's outputs (dict vals, d, ro, rho, nf, ok; d preset to 7) for the problems `idx` of case `c` against the oracle:
    decisions and nfact identical; rho, rho_old and the rho slots bit-equal to the oracle's rounded to float32, the rest of vals
    untouched; d untouched where no rho repairs the problem; backward error of every successful problem, forward error of those
    that succeeded at once.  Returns the largest (backward, forward) error seen."""
    s = c["s"]
    n = s.nvar
    ok0, nf0 = c["ok"][idx], c["nf"][idx]
    assert np.array_equal(np.asarray(out["ok"]), ok0.astype(np.int32)), (out["ok"], ok0)
    assert np.array_equal(np.asarray(out["nf"], np.int64), nf0), (out["nf"], nf0)
    assert np.array_equal(bits(out["rho"]), bits(c["rho"][idx]))
    assert np.array_equal(bits(out["ro"]), bits(c["ro"][idx]))
    assert np.array_equal(bits(out["vals"][:, -n:]), bits(c["vals_after"][idx][:, -n:]))
    assert np.array_equal(bits(out["vals"][:, :-n]), bits(vals_in[:, :-n]))      # (bit patterns: the NaNs of the hopeless problem compare)
    worst_b = worst_f = 0.0
    for k, b in enumerate(idx):
        d = out["d"][k]
        if not ok0[k]:
            assert (d == 7.0).all(), b
            continue
        be = G.backward_error(s, out["vals"][k], c["rhs"][b], d)
        assert be <= BWD_TOL, (b, be)
        worst_b = max(worst_b, be)
        if nf0[k] == 1:
            fe = np.abs(d - c["d"][b]).max() / np.abs(c["d"][b]).max()
            assert fe <= FWD_TOL, (b, fe)
            worst_f = max(worst_f, fe)
    return worst_b, worst_f
