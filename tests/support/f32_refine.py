"""What the tests of the refined handles (tuning float32_refine: a Float64 handle on a Float32 factor, refined with a Float64
residual) share: the inputs the GPU tests name, the error measures and the two DERIVED bounds, and a numpy model of the
refinement — an unpivoted float32 LDL' with the residual in float64 — which the CPU test holds against those bounds.

Notation.  m: the largest number of entries in a row of the full K (duplicates counted).  omega(d): max over rows i of
|rhs + K d|_i / (|K||d| + |rhs|)_i, K from the Float64 vals as returned (rho tail included), formed in numpy longdouble.

The bounds are derived, not measured: a Float64 residual of m + 2 terms has a componentwise error of at most about
(m + 1) eps64 (|K||d| + |rhs|) in any summation order, and converged fixed-precision refinement reaches that level (Skeel;
Higham, Accuracy and Stability of Numerical Algorithms, section 12).  Each gets a factor 2:
  backward  omega(d) <= 2 (m + 2) eps64
  forward   max|d - d*| / max|d*| <= cond_inf(K) 2 (m + 2) eps64,  d* numpy's Float64 solve of that K."""
import numpy as np

EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
CONTRACTION = 1000.0   # every refinement step shrinks max|rhs + K d| by more than this (cond ~ 1e2: eps32 cond << 1e-3)


def full_rows(s):
    """(rows, cols, slot) of the FULL matrix, 0-based: every COO entry, and every strict-lower one mirrored"""
    rows, cols = s.kkt_pattern()
    r, c = np.asarray(rows) - 1, np.asarray(cols) - 1
    e = np.arange(len(r))
    off = r != c
    return np.concatenate([r, c[off]]), np.concatenate([c, r[off]]), np.concatenate([e, e[off]])


def max_row_entries(s):
    fr, _, _ = full_rows(s)
    return int(np.bincount(fr, minlength=s.N).max())


def bwd_bound(s):
    return 2 * (max_row_entries(s) + 2) * EPS64


def kkt_long(s, vals):
    """dense symmetric K in longdouble, duplicates summed"""
    fr, fc, fs = full_rows(s)
    K = np.zeros((s.N, s.N), np.longdouble)
    np.add.at(K, (fr, fc), np.asarray(vals, np.longdouble)[fs])
    return K


def residual_long(s, vals, rhs, d):
    """g = rhs + K d and the componentwise scale |K||d| + |rhs|, both longdouble"""
    K = kkt_long(s, vals)
    d, rhs = np.asarray(d, np.longdouble), np.asarray(rhs, np.longdouble)
    return rhs + K @ d, np.abs(K) @ np.abs(d) + np.abs(rhs)


def omega(s, vals, rhs, d):
    g, scale = residual_long(s, vals, rhs, d)
    return float((np.abs(g) / scale).max())


def forward(s, vals, rhs, d):
    """(max|d - d*| / max|d*|, its bound): d* = -(K^-1 rhs) by numpy's Float64 solve, cond_inf by numpy"""
    K = kkt_long(s, vals).astype(np.float64)
    dstar = -np.linalg.solve(K, np.asarray(rhs, np.float64))
    err = float(np.abs(np.asarray(d, np.float64) - dstar).max() / np.abs(dstar).max())
    return err, float(np.linalg.cond(K, np.inf)) * bwd_bound(s)


def check_bounds(s, vals, rhs, d, what=""):
    """asserts both bounds for one problem; returns (omega / bound, forward error / bound)"""
    om, fb = omega(s, vals, rhs, d), forward(s, vals, rhs, d)
    print(f"{what}: omega {om:.2e} (bound {bwd_bound(s):.2e}), forward {fb[0]:.2e} (bound {fb[1]:.2e})")
    assert om <= bwd_bound(s), (what, om, bwd_bound(s))
    assert fb[0] <= fb[1], (what,) + fb
    return om / bwd_bound(s), fb[0] / fb[1]


# ---- the numpy model: unpivoted LDL' in float32 (the KKT matrices here are quasi-definite: every order has one), residual in float64 ----
def ldlt32(K):
    """unit lower L and D of K rounded to float32, every operation in float32"""
    A = np.array(K, np.float32)
    n = A.shape[0]
    D = np.zeros(n, np.float32)
    for j in range(n):
        D[j] = A[j, j]
        col = A[j + 1:, j].copy()
        A[j + 1:, j] = col / D[j]
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], col)
    return np.tril(A, -1), D


def solve32(L, D, g):
    """-(K^-1 g) on the float32 factor, in float32 (solve_ldl! returns d = -(K^-1 rhs))"""
    x = np.array(g, np.float32)
    n = len(x)
    for j in range(n):
        x[j + 1:] -= L[j + 1:, j] * x[j]
    x /= D
    for j in range(n - 1, -1, -1):
        x[j] -= np.dot(L[j + 1:, j], x[j + 1:])
    return -x


def refine_model(s, vals, rhs, k):
    """the refined call in numpy: returns d (float64) and norms[j] = max|rhs + K d_j| in front of correction j (and behind the last)"""
    K = kkt_long(s, vals).astype(np.float64)
    L, D = ldlt32(K)
    d = solve32(L, D, np.asarray(rhs, np.float32)).astype(np.float64)
    norms = []
    for _ in range(k):
        g = rhs + K @ d
        norms.append(float(np.abs(g).max()))
        d = d + solve32(L, D, g.astype(np.float32)).astype(np.float64)
    norms.append(float(np.abs(rhs + K @ d).max()))
    return d, norms


# ---- the inputs the GPU tests name (Float64 values of the project's generators) ----
def _stack(pairs):
    pairs = list(pairs)
    return np.ascontiguousarray(np.stack([v for v, _ in pairs])), np.ascontiguousarray(np.stack([r for _, r in pairs]))


def inputs(syn, name):
    """name -> (structure, vals [B][nnz], rhs [B][N]), all problems positive definite on the variables"""
    if name == "random":
        s = syn.random_structure(60, 80, 4, 0.1, 1)
        return (s,) + _stack(syn.random_values(s, seed) for seed in range(100, 108))
    if name == "band":
        s = syn.band_structure(300, 4, hw=3)
        # (seeds 301 and 308 are left out: the model's natural-order float32 LDL' meets a small pivot there and contracts by 5e4 only,
        #  so two steps stop at omega 1e-13 — the input is changed, not the bound)
        return (s,) + _stack(syn.band_values(s, seed) for seed in (300, 302, 303, 304, 305, 306, 307, 309))
    if name == "dense":
        s = syn.dense_structure(40, 70)
        return (s,) + _stack(syn.dense_values(s, seed) for seed in range(400, 403))
    if name == "random-large-front":
        s = syn.random_structure(129, 150, 0, 0.06, 5)
        return (s,) + _stack(syn.random_values(s, seed) for seed in range(500, 502))
    raise KeyError(name)


INPUT_NAMES = ("random", "band", "dense", "random-large-front")

# the residual kernel's own cases: (name, batch)
# ("band-300": N = 604 at two problems cuts a problem into chunks of rows in the lane instance too — csrc/refine.h, KKT_TARGET_WORKGROUPS)
RESIDUAL_CASES = (("random", 5), ("dense", 3), ("model-band", 2), ("band-300", 2))


def residual_inputs(syn, name, B):
    """(structure, vals, rhs, d): random Float64 data, the residual kernel assumes nothing about them"""
    s = {"random": lambda: syn.random_structure(60, 80, 4, 0.1, 1), "dense": lambda: syn.dense_structure(40, 70),
         "model-band": lambda: syn.model_band_structure(30, 3), "band-300": lambda: syn.band_structure(300, 4, hw=3)}[name]()
    rng = np.random.default_rng(7 + B)
    return s, rng.normal(size=(B, s.nnzNS)), rng.normal(size=(B, s.N)), rng.normal(size=(B, s.N))


def mixed_ladder_inputs(syn):
    """the "random" batch with problem 5 indefinite (it climbs the rho ladder of the demoted Float64 parameters to rho = 6) and problem 6
    so indefinite — the Hessian values of an indefinite problem times 30 — that only the next rung, 600 > RHO_MAX_SMALL, would
    rescue it; both sit in the workgroup of problems 4 .. 7 (v1_ppb = 4)"""
    s, vals, rhs = inputs(syn, "random")
    vals, rhs = vals.copy(), rhs.copy()
    vals[5], rhs[5] = syn.random_values(s, 205, posdef=False)
    v6, r6 = syn.random_values(s, 206, posdef=False)
    off = s.offsets()
    v6[off[0]:off[1]] *= 30.0
    vals[6], rhs[6] = v6, r6
    return s, vals, rhs


RHO_MAX_SMALL = 100.0
FAILS, CLIMBS = 6, 5


def demoted_params(hipldl, rho_max=None):
    """(Float64 parameters, what the refined handle hands its inner handle): narrowed to float, eig_tol raised to eps(Float32)"""
    p64 = hipldl.default_params(np.float64).copy()
    if rho_max is not None:
        p64[6] = rho_max
    p32 = p64.astype(np.float32)
    p32[0] = max(p32[0], np.float32(EPS32))
    return p64, p32
