"""Rows f1, f2, f4 and the trial point restated in float32 (test infrastructure, not part of the product).

The recipes of oracle.residual_vectors / prepare / trial_point / cgls_multipliers with T = Float32, batched over a leading
problem axis: numpy on float32 arrays, so every operation is rounded to float32 once (numpy never fuses a multiply and an add),
and the transposed products are summed per column in COO order.  One step leaves float32: the trial point sums the squares of
dlambda in float64 and rounds the norm to float32 once, as the kernel does.
"""
import numpy as np

F = np.float32


def column_ranks(rows, cols, nvar, nequ, ncon):
    """The J_F and the J_c entries of every variable column (column <= nvar < row), in COO order, grouped by their rank inside the
    column: two lists whose entry u holds (columns, slots, indices) of the u-th entry of every column that has one."""
    i0 = np.asarray(rows, np.int64) - 1
    j0 = np.asarray(cols, np.int64) - 1
    out = []
    for sel, base in (((j0 < nvar) & (i0 >= nvar) & (i0 < nvar + nequ), nvar), ((j0 < nvar) & (i0 >= nvar + nequ), nvar + nequ)):
        k = np.nonzero(sel)[0]
        o = np.argsort(j0[k], kind="stable")   # by column; COO order inside a column
        k = k[o]
        col = j0[k]
        rank = np.arange(len(k)) - np.searchsorted(col, col, side="left")
        out.append([(col[rank == u], k[rank == u], i0[k[rank == u]] - base) for u in range(int(rank.max()) + 1 if len(k) else 0)])
    return out


def column_sums(ranks, vals, x, nvar, dtype=F):
    """y[:, j] = sum over the entries of column j, in COO order, of vals[:, slot] * x[:, index] (multiply, then add)"""
    y = np.zeros((vals.shape[0], nvar), dtype)
    for c, sl, ix in ranks:
        y[:, c] = y[:, c] + vals[:, sl] * x[:, ix]
    return y


def _ninf(v):
    """norm(v, Inf) of every row: NaN propagates, an empty row gives 0"""
    return np.max(np.abs(v), axis=1) if v.shape[1] else np.zeros(v.shape[0], F)


def _rows(a, B, n):
    return np.asarray(a, F).reshape(B, n) if n else np.zeros((B, 0), F)


def residual_vectors(rows, cols, vals, nvar, nequ, ncon, r, lam, Fx, cx):
    """rows f1 for a batch: rhs [B][N] = [Jx' r - Jc' lam ; Fx - r ; cx] and norms [B][2] = (||dual||_inf, ||primal||_inf), the
    Jacobian values read from the J segments of vals [B][nnz]"""
    vals = np.asarray(vals, F)
    B = vals.shape[0]
    r, Fx, lam, cx = _rows(r, B, nequ), _rows(Fx, B, nequ), _rows(lam, B, ncon), _rows(cx, B, ncon)
    rF, rC = column_ranks(rows, cols, nvar, nequ, ncon)
    dual = column_sums(rF, vals, r, nvar) - column_sums(rC, vals, lam, nvar)
    primal = np.concatenate([Fx - r, cx], axis=1)
    return np.concatenate([dual, primal], axis=1), np.stack([_ninf(dual), _ninf(primal)], axis=1).astype(F)


def prepare(vals, nvar, nequ, ncon, nnzhF, nnzhc, nnzjF, nnzjc, hF, hc, Jx, Jcx, delta):
    """prepare_newton_system! for a batch, into a copy of vals [B][nnz]: H_F <- hF (left alone when hF is None), H_c <- -hc,
    J_F <- Jx, J_c <- Jcx, -delta I <- -delta[b], rho I <- 0; the -I segment is left alone"""
    v = np.array(vals, F, copy=True)
    o1 = nnzhF
    o2 = o1 + nnzhc
    o3 = o2 + nnzjF
    o4 = o3 + nnzjc
    o5 = o4 + nequ
    o6 = o5 + ncon
    if hF is not None:
        v[:, :o1] = np.asarray(hF, F)
    if ncon:
        v[:, o1:o2] = -np.asarray(hc, F)
        v[:, o3:o4] = np.asarray(Jcx, F)
        v[:, o5:o6] = -np.asarray(delta, F).reshape(-1, 1)
    v[:, o2:o3] = np.asarray(Jx, F)
    v[:, o6:] = F(0)
    return v


def trial_point(nvar, nequ, ncon, x, r, lam, d, max_dlambda=1e4):
    """xt = x + dx, rt = r + dr, dl = -d[n+m+1:N], dl = dl * M / ||dl||_2 where the norm exceeds M, lamt = lam + dl, for a batch;
    the norm: squares summed in float64, rounded to float32 once.  Returns (xt, rt, lamt, dl)."""
    d = np.asarray(d, F)
    B = d.shape[0]
    x, r, lam = _rows(x, B, nvar), _rows(r, B, nequ), _rows(lam, B, ncon)
    xt = x + d[:, :nvar]
    rt = r + d[:, nvar:nvar + nequ]
    dl = -d[:, nvar + nequ:nvar + nequ + ncon]
    nrm = np.sqrt(np.sum(dl.astype(np.float64) ** 2, axis=1)).astype(F)
    M = F(max_dlambda)
    with np.errstate(all="ignore"):
        dl = np.where((nrm > M)[:, None], (dl * M) / nrm[:, None], dl)
    return xt, rt, lam + dl, dl


def cgls_multipliers(rows, cols, vals, nvar, nequ, ncon, r, atol=None, rtol=None, itmax=0, ones_if_zero=True, dtype=F, trace=None):
    """row f4 for ONE problem with element type `dtype` (oracle.cgls_multipliers' recurrence; Float32 unless told otherwise, and with
    dtype = float64 the oracle's own results bit for bit).  Returns (lambda, Jxtr, iterations, margin): margin is the smallest relative
    distance | ||s|| - tol | / tol over the stopping tests taken; `trace` (a list) receives ||s|| / tol of every one of them."""
    T = np.dtype(dtype).type
    vals = np.asarray(vals, T).reshape(1, -1)
    rF, rC = column_ranks(rows, cols, nvar, nequ, ncon)
    Jxtr = column_sums(rF, vals, np.asarray(r, T).reshape(1, -1), nvar, T)[0]
    A = np.zeros((nvar, ncon), T)   # A = Jc'
    for c, sl, ix in rC:
        A[c, ix] = vals[0, sl]
    eps = np.finfo(T).eps
    atol = T(np.sqrt(eps) if atol is None else atol)
    rtol = T(np.sqrt(eps) if rtol is None else rtol)
    x = np.zeros(ncon, T)
    res = Jxtr.copy()
    s = A.T @ res
    p = s.copy()
    gamma = T(s @ s)
    tol = atol + rtol * np.sqrt(gamma)
    itmax = nvar + ncon if itmax <= 0 else itmax
    it = 0
    margin = np.inf
    while it < itmax:
        ng = np.sqrt(gamma)
        margin = min(margin, abs(float(ng) - float(tol)) / float(tol))
        if trace is not None:
            trace.append(float(ng) / float(tol))
        if not ng > tol:
            break
        q = A @ p
        delta = T(q @ q)
        if delta == 0:
            break
        alpha = gamma / delta
        x = x + alpha * p
        res = res - alpha * q
        s = A.T @ res
        gnext = T(s @ s)
        p = s + (gnext / gamma) * p
        gamma = gnext
        it += 1
    if ones_if_zero and T(x @ x) == 0:
        x = np.ones(ncon, T)
    return x, Jxtr, it, margin
