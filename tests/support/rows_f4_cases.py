"""Cases for row f4 (`cgls_kernel`) and the trial point (`trial_point_kernel`) at every loop edge, in both element types (test
infrastructure, not part of the product).  Pure numpy; the CPU tests check these inputs, the GPU tests run them.

Patterns.  Diagonal H_F, diagonal H_c, J_F = I (one entry per residual row), so the KKT analysis is trivial; only J_c varies:
  coupled_rows(n, p, empty)  constraint row k on columns k, k+1, k+2 (mod n): neighbouring rows share columns, Jc Jc' is
                             tridiagonal-plus (a wrong beta or p update changes the answer, not only the iteration count); rows named
                             in `empty` have no entry
  long_rows(n, lens, seed)   row k on lens[k] distinct random columns: the wavefront loop of a row takes zero to four passes
  rect(n)                    coupled_rows(n, 3) and one more residual row on column 1: nvar + nequ = 2 n + 1
A pattern is a synthetic.Structure whose meta["jc_values"](rng) draws the J_c values of one problem (float64).

Restatement.  `restated` is tests/support/f32_rows.cgls_multipliers with the element type passed on: numpy in that type, every
operation rounded once.  In float64 it is oracle.cgls_multipliers bit for bit (asserted by the CPU tests).

Judges.  `Judge` forms A = Jc' and b = Jx' r in longdouble from the inputs and measures a multiplier vector against the least-squares
problem itself, so that a mistake the kernel and the restatement share still fails:
  ne_residual(lam) = ||A'(A lam - b)||, to be held against the recurrence's own stopping threshold atol + rtol ||A' b||;
  distance(lam)    = ||lam - lam_ls|| <= ||A'(A lam - b)|| / sigma_min(A)^2: with g = A'(A lam - b) and A' A lam_ls = A' b,
                     g = A'A (lam - lam_ls), and ||(A'A)^-1|| = 1 / sigma_min^2 — holds for any vector.
"""
import functools

import numpy as np

from tests.support import f32_rows as R

LD = np.longdouble
LONG_LENS = (1, 63, 64, 65, 128, 129, 200)


def _structure(n, nequ, jF, jc_rows, jc_cols, p, gen, name):
    from cannoles_jl_amd import synthetic as syn
    d = np.arange(1, n + 1, dtype=np.int64)
    z = np.zeros(0, np.int64)
    hc = (d, d) if p else (z, z)
    jc = (np.asarray(jc_rows, np.int64) + 1, np.asarray(jc_cols, np.int64) + 1) if p else (z, z)
    return syn.Structure(n, nequ, p, (d, d), hc, jF, jc, name=name, meta={"jc_values": gen})


def coupled_rows(n, p, empty=(), extra_residual=False):
    rows = np.array([k for k in range(p) if k not in empty for _ in range(3)], np.int64)
    cols = np.array([(k + j) % n for k in range(p) if k not in empty for j in range(3)], np.int64)

    def gen(rng):
        m = len(rows) // 3
        v = np.empty((m, 3))
        v[:, 0] = rng.choice([-1.0, 1.0], m) * (1.5 + 0.5 * rng.uniform(-1, 1, m))
        v[:, 1:] = 0.4 * rng.uniform(-1, 1, (m, 2))
        return v.ravel()

    d = np.arange(1, n + 1, dtype=np.int64)
    if extra_residual:
        jF, nequ = (np.concatenate([d, [n + 1]]), np.concatenate([d, [1]])), n + 1
    else:
        jF, nequ = (d, d), n
    return _structure(n, nequ, jF, rows, cols, p, gen, f"coupled-{n}-{p}")


def long_rows(n, lens, seed):
    rng = np.random.default_rng(seed)
    rows = np.concatenate([np.full(ln, k, np.int64) for k, ln in enumerate(lens)])
    cols = np.concatenate([np.sort(rng.choice(n, ln, replace=False)) for ln in lens])
    d = np.arange(1, n + 1, dtype=np.int64)
    return _structure(n, n, (d, d), rows, cols, len(lens), lambda g: g.uniform(-1, 1, len(rows)), f"long-{n}")


def rect(n):
    return coupled_rows(n, 3, extra_residual=True)


@functools.lru_cache(maxsize=None)
def pattern(name):
    if name.startswith("p-"):
        p = int(name[2:])
        return coupled_rows(1100, p, empty=(2,) if p > 3 else ())
    return {"few-vars": lambda: coupled_rows(200, 130), "long-300": lambda: long_rows(300, LONG_LENS, 1),
            "long-200": lambda: long_rows(200, LONG_LENS, 2), "over-1100": lambda: coupled_rows(1200, 1100),
            "over-1025": lambda: coupled_rows(1100, 1025), "one-chunk": lambda: coupled_rows(512, 3), "rect": lambda: rect(512),
            "no-constraints": lambda: coupled_rows(300, 0)}[name]()


def model(s, B, seed, dtype):
    """the model's arrays of a batch in `dtype`: Hessian and Jacobian values, delta, and the vectors the two rows take"""
    rng = np.random.default_rng(seed)
    f = lambda *sh: rng.standard_normal(sh)   # noqa: E731
    m = {"hF": 1.0 + np.abs(f(B, s.nnzhF)), "hc": 0.1 * f(B, s.nnzhc), "Jx": f(B, s.nnzjF),
         "Jcx": np.stack([s.meta["jc_values"](rng) for _ in range(B)]).reshape(B, s.nnzjc), "delta": 0.1 + np.abs(f(B)),
         "x": f(B, s.nvar), "r": f(B, s.nequ), "lam": f(B, s.ncon), "d": f(B, s.N)}
    return {k: np.ascontiguousarray(v, dtype) for k, v in m.items()}


def vals_of(s, m):
    """`vals` [B][nnz] as prepare_newton_system! leaves them: [H_F | -H_c | J_F | J_c | -I | -delta I | rho I = 0]"""
    B, dt = m["Jx"].shape[0], m["Jx"].dtype
    off = s.offsets()
    v = np.zeros((B, s.nnzNS), dt)
    v[:, off[0]:off[1]] = m["hF"]
    v[:, off[1]:off[2]] = -m["hc"]
    v[:, off[2]:off[3]] = m["Jx"]
    v[:, off[3]:off[4]] = m["Jcx"]
    v[:, off[4]:off[5]] = -1
    v[:, off[5]:off[6]] = -m["delta"][:, None]
    return v


# ---- CGLS cases: name -> (pattern, B, seed, what the batch is changed to, keyword arguments of the call) ------------------------------
# The seeds of the long-row cases are chosen, and tests/test_rows_f4_trial_cpu.py asserts what they are chosen for:
#  * cond(Jc') <= 31: a row of one entry near zero makes its multiplier ill-determined, and the Float32 distance to the least-squares
#    solution is then an input's property, not the kernel's;
#  * no more steps than constraints.  With p constraints CGLS ends after p steps in exact arithmetic, so the ||s|| of the test after
#    step p is rounding noise: another summation order changes it by its whole size, not by an eps, and the margin of that test means
#    nothing.  A Float32 restatement that goes on to step p + 1 (noise above the threshold) is an input the kernel may rightly leave
#    after p; where it stops after p, its noise must be at most a tenth of the threshold (NOISE_ROOM).
NOISE_ROOM = 0.1


def _zeros(s, m):
    m["r"][1] = 0
    m["Jcx"][2] = 0


def _isolation(s, m):
    m["r"][1] = 0
    m["r"][3, 17] = np.nan


HUGE_ITMAX = (2 ** 63 - 1, 2 ** 32)
CGLS_CASES = {
    **{f"p-{p}": (f"p-{p}", 3, 1, None, {}) for p in (1, 3, 255, 256, 257, 1024)},
    "few-vars": ("few-vars", 3, 1, None, {}),
    "long-300": ("long-300", 3, 7, None, {}),
    "long-200": ("long-200", 3, 89, None, {}),
    "itmax-3": ("long-300", 3, 7, None, {"itmax": 3}),
    "rtol": ("long-300", 3, 86, None, {"atol": 0.0, "rtol": 1e-3}),   # (a seed at which the looser threshold ends a problem earlier)
    "itmax-max": ("long-300", 3, 7, None, {"itmax": HUGE_ITMAX[0]}),
    "itmax-2^32": ("long-300", 3, 7, None, {"itmax": HUGE_ITMAX[1]}),
    "zeros": ("long-300", 4, 8, _zeros, {}),
    "zeros-kept": ("long-300", 4, 8, _zeros, {"ones_if_zero": False}),
    "isolation": ("long-300", 5, 77, _isolation, {}),
}
DTYPES = (np.float64, np.float32)


@functools.lru_cache(maxsize=None)
def cgls_case(name, dtype):
    """(structure, model arrays, vals, keyword arguments) of a case; cached, treat as read-only"""
    pat, B, seed, change, kw = CGLS_CASES[name]
    s = pattern(pat)
    m = model(s, B, seed, dtype)
    if change:
        change(s, m)
    return s, m, vals_of(s, m), kw


def restated(s, vals_b, r_b, dtype, **kw):
    """(lambda, Jxtr, iterations, margin) of ONE problem by the recurrence restated in `dtype`"""
    rows, cols = s.kkt_pattern()
    return R.cgls_multipliers(rows, cols, vals_b, s.nvar, s.nequ, s.ncon, r_b, dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def cgls_reference(name, dtype):
    """the restatement's results for every problem of a case: a list of (lambda, Jxtr, iterations, margin)"""
    s, m, vals, kw = cgls_case(name, dtype)
    with np.errstate(invalid="ignore"):
        return [restated(s, vals[b], m["r"][b], dtype, **kw) for b in range(vals.shape[0])]


@functools.lru_cache(maxsize=None)
def cgls_last_ratio(name, dtype):
    """||s|| / threshold at the last stopping test of every problem of a case (restated)"""
    s, m, vals, kw = cgls_case(name, dtype)
    out = []
    with np.errstate(invalid="ignore"):
        for b in range(vals.shape[0]):
            tr = []
            restated(s, vals[b], m["r"][b], dtype, trace=tr, **kw)
            out.append(tr[-1])
    return out


class Judge:
    """the least-squares problem of ONE problem of a case in longdouble, from the inputs (see the module docstring).  A constraint row
    without entries is a zero column of A: the problem does not involve its multiplier, CGLS started at 0 leaves it 0 (`dead`, to be
    asserted exactly), and sigma_min, cond and the distances are those of the other columns (`live`)."""

    def __init__(self, s, m, b, dtype, atol=None, rtol=None, **_):
        jr, jc = np.asarray(s.jc[0]) - 1, np.asarray(s.jc[1]) - 1
        A = np.zeros((s.nvar, s.ncon), LD)   # A = Jc'
        A[jc, jr] = m["Jcx"][b].astype(LD)
        bb = np.zeros(s.nvar, LD)
        np.add.at(bb, np.asarray(s.jF[1]) - 1, m["Jx"][b].astype(LD) * m["r"][b].astype(LD)[np.asarray(s.jF[0]) - 1])
        self.live = np.bincount(jr, minlength=s.ncon) > 0
        self.dead = ~self.live
        self.A, self.b = A[:, self.live], bb
        self.A64 = self.A.astype(np.float64)
        self._U, self.sv, self._Vt = np.linalg.svd(self.A64, full_matrices=False)
        eps = float(np.finfo(dtype).eps)
        atol = np.sqrt(eps) if atol is None else atol
        rtol = np.sqrt(eps) if rtol is None else rtol
        g0 = self.A.T @ bb
        self.s0 = float(np.sqrt(np.sum(g0 * g0)))
        self.threshold = atol + rtol * self.s0
        self._ls = None

    @property
    def cond(self):
        return float(self.sv.max() / self.sv.min()) if self.sv.min() > 0 else np.inf

    def ne_residual(self, lam):
        lam = np.asarray(lam).astype(LD)[self.live]
        g = self.A.T @ (self.A @ lam - self.b)
        return float(np.sqrt(np.sum(g * g)))

    @property
    def ls(self):
        """the least-squares solution: the fp64 SVD's, refined twice with the residual formed in longdouble"""
        if self._ls is None:
            x = np.zeros(self.A.shape[1], LD)
            for _ in range(3):
                res = (self.b - self.A @ x).astype(np.float64)
                x = x + (self._Vt.T @ ((self._U.T @ res) / self.sv)).astype(LD)
            self._ls = x
        return self._ls

    def distance(self, lam):
        """(||lam - lam_ls||, ||lam_ls||) over the live multipliers"""
        e = np.asarray(lam).astype(LD)[self.live] - self.ls
        return float(np.sqrt(np.sum(e * e))), float(np.sqrt(np.sum(self.ls * self.ls)))

    def distance_bound(self, lam):
        """||A'(A lam - b)|| / sigma_min^2, times 1 + 1e-6 for the fp64 SVD, plus the judge's own rounding: the residual is a
        difference of terms of size ||A|| (||A|| ||lam|| + ||b||) formed in longdouble — 64 eps(longdouble) of that over sigma_min^2,
        and of ||lam_ls|| (with one constraint the bound is an equality, and a Float64 lambda sits 1e-16 from lam_ls)"""
        smax, smin = float(self.sv.max()), float(self.sv.min())
        nl = float(np.linalg.norm(np.asarray(lam, np.float64)[self.live]))
        nb = float(np.sqrt(np.sum(self.b * self.b)))
        floor = 64 * float(np.finfo(LD).eps) * (smax * (smax * nl + nb) / smin ** 2 + float(np.sqrt(np.sum(self.ls * self.ls))))
        return self.ne_residual(lam) / smin ** 2 * (1 + 1e-6) + floor


# ---- trial point -------------------------------------------------------------------------------------------------------------------
TRIAL_SHAPES = ("few-vars", "one-chunk", "rect", "p-1024", "over-1100", "p-255", "p-256", "p-257", "no-constraints")
# "exact": d has -max_dlambda in one constraint slot and zeros elsewhere.  That alone cannot tell `>` from `>=`: scaled by
# max_dlambda / norm = 1e4 / 1e4, the entries 1e4 and -0.0 come back bit for bit (1e8 is exact in both types).  "exact-dust" has the same
# norm after rounding — the other entries are near 1e-6, their squares vanish below half an ulp of 1e8 in the double sum — and those
# entries are CHOSEN so that (x * 1e4) / 1e4 != x in the element type: a kernel that scales at equality changes them.
TRIAL_VARIANTS = ("under", "exact", "one-ulp-above", "far-above", "zero", "nan", "exact-dust", "overflow")   # the last one: Float32 only
MAX_DLAMBDA = 1e4


def _dust(rng, n, T):
    """n values near 1e-6 of type T that (x * max_dlambda) / max_dlambda does not reproduce"""
    c = (rng.uniform(1, 2, 64 * n + 64) * 1e-6).astype(T)
    c = c[(c * T(MAX_DLAMBDA)) / T(MAX_DLAMBDA) != c]
    assert len(c) >= n
    return c[:n] * rng.choice(np.array([-1, 1], T), n)


def trial_batch(s, dtype, seed=7):
    """x, r, lam, d of one batch that carries every dlambda variant (problem i: TRIAL_VARIANTS[i]) and the slot of the NaN"""
    B = len(TRIAL_VARIANTS) if dtype == np.float32 else len(TRIAL_VARIANTS) - 1
    m = model(s, B, seed, dtype)
    d, c0, p = m["d"], s.nvar + s.nequ, s.ncon
    nan_slot = p // 2
    if p:
        T = np.dtype(dtype).type
        d[1, c0:] = 0
        d[1, c0 + p - 1] = -T(MAX_DLAMBDA)
        d[2, c0:] = 0
        d[2, c0 + p - 1] = -np.nextafter(T(MAX_DLAMBDA), T(np.inf))
        d[3, c0:] *= T(1e6)
        d[4, c0:] = 0
        d[5, c0 + nan_slot] = np.nan
        d[6, c0:c0 + p - 1] = _dust(np.random.default_rng(seed + 1), p - 1, T)
        d[6, c0 + p - 1] = -T(MAX_DLAMBDA)
        if B > 7:
            d[7, c0:] *= T(1e25)
    return m["x"], m["r"], m["lam"], d, nan_slot


def trial_reference(s, x, r, lam, d, dtype):
    """(xt, rt, lambdat, dlambda) of the batch by the restatement of the element type: oracle.trial_point, f32_rows.trial_point"""
    if dtype == np.float32:
        return R.trial_point(s.nvar, s.nequ, s.ncon, x, r, lam, d, MAX_DLAMBDA)
    from oracle import oracle as O
    with np.errstate(invalid="ignore"):
        out = [O.trial_point(s.nvar, s.nequ, s.ncon, x[b], r[b], lam[b], d[b], MAX_DLAMBDA) for b in range(d.shape[0])]
    return tuple(np.stack([o[i] for o in out]) for i in range(4))
