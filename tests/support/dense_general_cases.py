"""What the tests of the general form of the dense backend in DOUBLE share (Route::GeneralDense: an irregular pattern whose condensed
system runs as ONE dense LDL' on csrc/dense.hip — dn_set_counts, dn_scatter_general, dn_shift, dn_yrhs_general, dn_out_general around
the panel, ladder and solve kernels of the residual-block form), and of the positive residual pivots on every route that counts
residual pivots outside its factor — tests/test_dense_general_cpu.py and tests/test_dense_general_gpu.py: numpy only.

Shapes: those of tests/support/f32_general_dense.py (one table for both element types: orders 96, 96 with constraints, 128, 129 with
a -delta pivot alone in the third tile, 129, 454) and BIG, order 800 with more than 262 144 condensed slots: the second trip of
dn_scatter_general's grid-stride loop (its grid is min(1024, ...) workgroups of 256).

Values: problem b takes syn.random_values(s, 40 + b) in double, and a SEVEN-problem mix goes by b % 7:
    0, 4  healthy                                                     ok, nfact 1
    1     hopeless (H_F = NaN)                                        fails, nfact 20, rho_old kept
    2     indefinite (the H_F segment times -20), rho_old = 0         ok, nfact 6
    3     the same from rho_old = 2                                   ok, nfact 4
    5     the residual pivot off[4] + m // 2 set to +0.5              ok, nfact 1, inertia (nvar, 0)
    6     kind 5 and kind 2 together                                  fails, nfact 20
Kind 5: the condensed matrix has nvar - 1 positive eigenvalues, so the call succeeds only if the one positive residual pivot counted
outside the dense factor is added; a kernel that drops that count climbs the ladder.  Kind 6: once rho makes the variable block
positive definite the total is nvar + 1, so no rho gives the right inertia; a kernel that keeps the outside count for the first
factorisation only answers success at about the sixth rung.  ZERO residual pivots are left out: a zero diagonal entry of the residual
block does not make K singular, and what the reference does with it depends on the elimination order.

Reference: the CPU oracle with its own default params on the canonical order (and, in the GPU tests, on the handle's own order).
What vouches for the decisions of kinds 5 and 6 is order-independent: the eigenvalues of the condensed matrix
K_kk - K_kr D_r^-1 K_rk (k: variables and multipliers, r: residual rows) at every rung, `rung_verdict`.

Run as a script (python -m tests.support.dense_general_cases) it runs the two smallest shapes on the device entry and prints one
line of hexadecimal digests per shape: the test of what earlier kernels left behind runs it in child processes."""
import hashlib

import numpy as np

from tests.support import dense_cases as dc
from tests.support import f32_general_dense as GD32

F32_SHAPES, shape_id, SMALLEST = GD32.SHAPES, GD32.shape_id, GD32.SMALLEST
BIG = (800, 900, 0, 0.05, 1)              # order 800, T = 13; 292 243 condensed slots
SHAPES = dict(F32_SHAPES)
SHAPES[BIG] = (800, None)                 # (the float table fixes the largest front of its shapes; here the CPU test asks fmax > 64)
SECOND = (92, 110, 4, 0.08, 2)
SCATTER_TRIP = 1024 * 256                 # slots one trip of dn_scatter_general's loop covers
MIX = 7
WANT_OK = [True, False, True, True, True, True, False]
WANT_NF = [1, 20, 6, 4, 1, 1, 20]
EIG_MARGIN = 1e-6     # seven orders above what a double LDL' of order 800 can perturb (800 eps = 1.8e-13)
EIG_MARGIN32 = 1e-3   # Float32 rows of the route table: the margin of the Float32 tests (f32_dense.EIG_MARGIN)


def structure(shape):
    from cannoles_jl_amd import synthetic as syn
    n, m, p, dens, seed = shape
    return syn.random_structure(n, m, p, dens, seed=seed)


def apply_kind(s, vals, kind, pivot=None):
    """the change of mix kind `kind` on one problem's values, in place; returns its rho_old"""
    off = s.offsets()
    if kind == 1:
        vals[off[0]:off[1]] = np.nan
    if kind in (2, 3, 6):
        vals[off[0]:off[1]] *= -20.0
    if kind in (5, 6):
        vals[off[4] + (s.nequ // 2 if pivot is None else pivot)] = 0.5
    return 2.0 if kind == 3 else 0.0


def values(s, B):
    """(vals, rhs, rho_old) of B problems of the mix, float64"""
    from cannoles_jl_amd import synthetic as syn
    vals, rhs, ro = np.zeros((B, s.nnzNS)), np.zeros((B, s.N)), np.zeros(B)
    for b in range(B):
        vals[b], rhs[b] = syn.random_values(s, 40 + b)
        ro[b] = apply_kind(s, vals[b], b % MIX)
    return vals, rhs, ro


_cache, _own = {}, {}


def _freeze(c):
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _oracle_case(key, s, vals, rhs, ro, params, kinds):
    """the case dict: inputs in their element type, the oracle's results (float64) on the canonical order"""
    from oracle import oracle as O
    rows, cols = s.kkt_pattern()
    B = len(vals)
    orc = O.Oracle(s.N, rows, cols, O.canonical_perm(s.nvar, s.nequ, s.ncon))
    va = np.array(vals, np.float64)
    d, ok, rho, rold, nf = O.newton_system_batch(orc, B, s.nvar, s.nequ, s.ncon, np.array(rhs, np.float64), va, np.array(ro, np.float64),
                                                 np.array(params, np.float64))
    return _freeze(dict(key=key, s=s, rows=rows, cols=cols, vals=vals, rhs=rhs, rho_old=ro, params=np.array(params), d=d,
                        ok=np.asarray(ok, bool), rho=rho, ro=rold, nf=np.asarray(nf, np.int64), vals_after=va, kinds=np.asarray(kinds)))


def case(shape, B=MIX):
    """The mix on a shape of the table and what the CPU oracle (its own default params) makes of it on the canonical order, computed
    once per session and shared (read-only): dict(s, rows, cols, vals, rhs, rho_old, params, d, ok, rho, ro, nf, vals_after, kinds)."""
    key = (shape, B)
    if key not in _cache:
        from oracle import oracle as O
        s = structure(shape)
        vals, rhs, ro = values(s, B)
        _cache[key] = _oracle_case(key, s, vals, rhs, ro, O.default_params(), np.arange(B) % MIX)
    return _cache[key]


def healthy_case(shape, nbase=8):
    """nbase healthy problems of a shape (syn.random_values at seeds 40, 45, ...): what the 256-problem test repeats over its batch"""
    key = (shape, "healthy", nbase)
    if key not in _cache:
        from cannoles_jl_amd import synthetic as syn
        from oracle import oracle as O
        s = structure(shape)
        vr = [syn.random_values(s, 40 + 5 * k) for k in range(nbase)]
        vals, rhs = np.stack([v for v, _ in vr]), np.stack([r for _, r in vr])
        _cache[key] = _oracle_case(key, s, vals, rhs, np.zeros(nbase), O.default_params(), np.zeros(nbase, np.int64))
    return _cache[key]


def subcase(c, idx):
    """problems `idx` of a case as a case of their own (the oracle treats every problem by itself)"""
    idx = np.asarray(idx)
    key = (c["key"], tuple(int(i) for i in idx))
    if key not in _cache:
        out = {k: (v[idx] if isinstance(v, np.ndarray) and k != "params" and v.shape[:1] == c["ok"].shape else v) for k, v in c.items()}
        out["key"] = key
        _cache[key] = _freeze({k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in out.items()})
    return _cache[key]


def oracle_on(perm, c):
    """the oracle's results for a double case on the elimination order `perm` (the handle's), once per (case, order)"""
    key = (c["key"], perm.tobytes())
    if key not in _own:
        from oracle import oracle as O
        s = c["s"]
        if np.array_equal(perm, O.canonical_perm(s.nvar, s.nequ, s.ncon)):    # (the handle eliminates in the canonical order)
            return c
        B = len(c["vals"])
        orc = O.Oracle(s.N, c["rows"], c["cols"], perm)
        v = np.array(c["vals"], np.float64)
        d, ok, rho, ro, nf = O.newton_system_batch(orc, B, s.nvar, s.nequ, s.ncon, np.array(c["rhs"], np.float64), v,
                                                   np.array(c["rho_old"], np.float64), np.array(c["params"], np.float64))
        _own[key] = dict(d=d, ok=np.asarray(ok, bool), rho=rho, ro=ro, nf=np.asarray(nf, np.int64), vals_after=v)
    return _own[key]


# ---- what vouches for kinds 5 and 6: eigenvalues ----
def kkt_dense(s, vals, rho=None):
    """the full symmetric KKT matrix of one problem in float64; rho (where given) replaces the rho slots"""
    rows, cols = s.kkt_pattern()
    v = np.array(vals, np.float64)
    if rho is not None:
        v[-s.nvar:] = rho
    K = np.zeros((s.N, s.N))
    np.add.at(K, (rows - 1, cols - 1), v)
    return K + np.tril(K, -1).T


def condensed_eigs(s, vals, rho):
    """(eigenvalues of K_kk - K_kr D_r^-1 K_rk at `rho`, ascending; residual pivots d_r)"""
    n, m = s.nvar, s.nequ
    K = kkt_dense(s, vals, rho)
    k = np.r_[0:n, n + m:s.N]
    dr = np.diag(K)[n:n + m].copy()
    assert not (K[n:n + m, n:n + m] - np.diag(dr)).any()
    Kkr = K[np.ix_(k, np.arange(n, n + m))]
    return np.linalg.eigvalsh(K[np.ix_(k, k)] - (Kkr / dr) @ Kkr.T), dr


def rung_verdict(lam, xpos, nvar, succeeds, margin=EIG_MARGIN):
    """Is the decision of a rung a property of the matrix?  `lam`: eigenvalues of the condensed matrix, `xpos`: positive residual
    pivots counted outside, `succeeds`: the oracle's decision.  Returns (determined, smallest |lambda| / largest |lambda|, how):
    "all": every eigenvalue is at least `margin` of the largest in modulus and count + xpos == nvar is the oracle's decision;
    "count" (failing rungs only): at least nvar eigenvalues lie above the margin and one more positive comes from outside."""
    big = np.abs(lam).max()
    rel = np.abs(lam).min() / big
    if rel >= margin:
        return (int((lam > 0).sum()) + xpos == nvar) == bool(succeeds), rel, "all"
    if not succeeds and int((lam >= margin * big).sum()) >= nvar and xpos == 1:
        return True, rel, "count"
    return False, rel, "undetermined"


def rung_verdicts(c, b, margin=EIG_MARGIN):
    """[(rho, determined, rel, how)] for every rung problem b took (by the oracle's nfact and dc.rungs)"""
    s = c["s"]
    p = np.array(c["params"], np.float64)
    rr = dc.rungs(float(c["rho_old"][b]), int(c["nf"][b]), p)
    out = []
    for k, rho in enumerate(rr):
        lam, dr = condensed_eigs(s, c["vals"][b], rho)
        assert (np.abs(dr) >= 0.5).all()       # no residual pivot near zero: the outside zero count is 0 in any arithmetic
        out.append((rho,) + rung_verdict(lam, int((dr > 0).sum()), s.nvar, bool(c["ok"][b]) and k == len(rr) - 1, margin))
    return out


_inertia = {}


def numpy_inertia(c, b, margin=EIG_MARGIN):
    """(npos, nzero, smallest |lambda| / largest) of the KKT matrix of problem b as given (rho slots as they are), from numpy's
    eigenvalues; nzero counts nothing while the margin holds, which the CPU test asserts"""
    key = (c["key"], b)
    if key not in _inertia:
        lam = np.linalg.eigvalsh(kkt_dense(c["s"], c["vals"][b]))
        big = np.abs(lam).max()
        _inertia[key] = (int((lam > 0).sum()), int((np.abs(lam) < margin * big).sum()), float(np.abs(lam).min() / big))
    return _inertia[key]


def condensed_slots(s):
    """lower-triangle entries of the condensed pattern: the pattern of K_kk together with that of J'J, in numpy"""
    n, m = s.nvar, s.nequ
    rows, cols = s.kkt_pattern()
    A = np.zeros((s.N, s.N), bool)
    A[rows - 1, cols - 1] = True
    A |= A.T
    k = np.r_[0:n, n + m:s.N]
    J = A[np.ix_(np.arange(n, n + m), k)].astype(np.float32)
    P = A[np.ix_(k, k)] | ((J.T @ J) > 0)
    P[np.arange(n), np.arange(n)] = True     # (the rho slots)
    return int(np.tril(P).sum())


# ---- the 16 / 17 decision of prefer_dense ----
# tools/time_dense_route.py's generator (fuzz_structure, family 2) at seed PREFER_SEED: a latency plan whose fronts reach the 64 class
# on a condensed system of order <= 512 — the dense route up to batch 16, the register-front kernel from 17 on
PREFER_SEED = 4
PREFER_KINDS = (0, 2, 5)


def fuzz_structure(seed):
    """the structures of tools/fuzz_parity.py, as tools/time_dense_route.py restates them"""
    from cannoles_jl_amd import synthetic as syn
    rng = np.random.default_rng(100000 + seed)
    fam = rng.integers(3)
    if fam == 0:
        n = int(rng.integers(6, 120)); m = int(rng.integers(max(2, n // 2), 2 * n)); pc = int(rng.integers(0, min(6, n // 2) + 1))
        return syn.random_structure(n, m, pc, float(rng.uniform(0.03, 0.3)), seed, hess=bool(rng.integers(4)))
    if fam == 1:
        return None
    n = int(rng.integers(130, 400)); m = int(rng.integers(n, n + 60)); pc = int(rng.integers(0, 4))
    return syn.random_structure(n, m, pc, float(rng.uniform(0.01, 0.04)), seed)


def prefer_case():
    key = "prefer"
    if key not in _cache:
        from cannoles_jl_amd import synthetic as syn
        from oracle import oracle as O
        s = fuzz_structure(PREFER_SEED)
        vals, rhs, ro = np.zeros((3, s.nnzNS)), np.zeros((3, s.N)), np.zeros(3)
        for b, kind in enumerate(PREFER_KINDS):
            vals[b], rhs[b] = syn.random_values(s, 40 + kind)
            ro[b] = apply_kind(s, vals[b], kind)
        _cache[key] = _oracle_case(key, s, vals, rhs, ro, O.default_params(), PREFER_KINDS)
    return _cache[key]


# ---- positive residual pivots on every route that counts them outside the factor ----
ROUTE_KINDS = (0, 5, 6)
# id: (element type, options, pattern).  Patterns: "smallest" = SMALLEST; "records" = random_structure(60, 80, 4, 0.1, seed=3);
# "resblock" = dense_cases.structure(65, 130, 0); "band" = band_structure(200, 4)
ROUTES = {
    "general-dense": (np.float64, {}, "smallest"),
    "condensed-general-kernel": (np.float64, dict(general_dense=0), "smallest"),
    "register-front-direct": (np.float64, {}, "records"),
    "v2-staged": (np.float64, {}, "band"),
    "dense-residual-block": (np.float64, {}, "resblock"),
    "band": (np.float64, dict(plan_kind=1), "band"),
    "float32-condense": (np.float32, dict(float32_general=1, float32_condense=1), "smallest"),
    "float32-general-dense": (np.float32, dict(float32_general=1, float32_general_dense=1), "smallest"),
    "float32-dense": (np.float32, dict(float32_general=1, float32_dense=1), "resblock"),
}


def route_pattern(name):
    from cannoles_jl_amd import synthetic as syn
    if name == "smallest":
        return structure(SMALLEST)
    if name == "records":
        return syn.random_structure(60, 80, 4, 0.1, seed=3)
    if name == "resblock":
        return dc.structure(65, 130, 0, dc.SEED)
    assert name == "band"
    return syn.band_structure(200, 4)


def route_case(name, dtype=np.float64):
    """B = 3, kinds 0, 5 and 6 on a pattern of the route table: the pattern's own generator at seeds 40, 45 and 46 (the healthy
    problems 0, 5 and 10 of dense_cases.values for the residual-block pattern), then the two rules of `apply_kind`; for Float32 the
    inputs are rounded to float32 and the oracle runs on the widened data with ParamCaNNOLeS(Float32) widened."""
    key = ("route", name, np.dtype(dtype).name)
    if key not in _cache:
        from cannoles_jl_amd import synthetic as syn
        from oracle import oracle as O
        s = route_pattern(name)
        B = len(ROUTE_KINDS)
        vals, rhs, ro = np.zeros((B, s.nnzNS)), np.zeros((B, s.N)), np.zeros(B)
        if name == "resblock":
            v, r, _ = dc.values(s, 11, dc.SEED)
            vals[:], rhs[:] = v[[0, 5, 10]], r[[0, 5, 10]]
        for b, kind in enumerate(ROUTE_KINDS):
            if name != "resblock":
                vals[b], rhs[b] = (syn.band_values if name == "band" else syn.random_values)(s, 40 + kind)
            ro[b] = apply_kind(s, vals[b], kind)
        if np.dtype(dtype) == np.float32:
            from tests.support import f32_dense as FD
            vals, rhs, ro = (np.ascontiguousarray(a, np.float32) for a in (vals, rhs, ro))
            params = FD.params32()
        else:
            params = O.default_params()
        _cache[key] = _oracle_case(key, s, vals, rhs, ro, params, ROUTE_KINDS)
    return _cache[key]


# ---- the device entry ----
class Args:
    """one argument set of cnl_newton_system_dev on the device (double)"""

    def __init__(self, s, B):
        import torch
        dev = torch.device("cuda:0")
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        self.vals, self.rhs, self.d = torch.zeros((B, s.nnzNS), **f64), torch.zeros((B, s.N), **f64), torch.zeros((B, s.N), **f64)
        self.ro, self.rho = torch.zeros(B, **f64), torch.zeros(B, **f64)
        self.nf, self.ok = torch.zeros(B, **i32), torch.zeros(B, **i32)

    def fill(self, vals, rhs, ro):
        import torch
        self.vals.copy_(torch.from_numpy(np.array(vals)))   # (copies: the shared cases are read-only)
        self.rhs.copy_(torch.from_numpy(np.array(rhs)))
        self.ro.copy_(torch.from_numpy(np.array(ro)))
        self.d.fill_(7.0)
        self.rho.fill_(-1.0)
        self.nf.fill_(-1)
        self.ok.fill_(-1)
        torch.cuda.synchronize()

    def call(self, hipldl, L, p):
        import torch
        hipldl.newton_system_dev(L, self.vals.data_ptr(), self.rhs.data_ptr(), self.d.data_ptr(), self.ro.data_ptr(), self.rho.data_ptr(),
                                 self.nf.data_ptr(), self.ok.data_ptr(), p, stream=torch.cuda.current_stream().cuda_stream)

    def read(self):
        import torch
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("vals", "d", "ro", "rho", "nf", "ok")}


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_outputs(out, refs, c, rhs, idx, bwd_tol, fwd_tol, backward_error):
    """One call's outputs (dict vals, d, ro, rho, nf, ok; d preset to 7) for the problems `idx` of case `c`, against the oracle on
    every order of `refs` — the assertions of tests/test_dense_gpu.py::_check_dev_outputs, bit patterns where that compares values:
    decisions, nfact, rho, rho_old and the whole of vals (only the rho slots change) bit for bit; d untouched for a failed problem;
    the forward error of a problem that succeeded at once, the backward error of every success.  Returns the largest (backward,
    forward) error seen."""
    s = c["s"]
    idx = np.asarray(idx)
    worst_b = worst_f = 0.0
    for ref in refs:
        ok0, nf0 = ref["ok"][idx], ref["nf"][idx]
        assert np.array_equal(out["ok"], ok0.astype(np.int32)), (out["ok"], ok0)
        assert np.array_equal(out["nf"], nf0), (out["nf"], nf0)
        assert np.array_equal(bits64(out["rho"]), bits64(ref["rho"][idx])) and np.array_equal(bits64(out["ro"]), bits64(ref["ro"][idx]))
        assert np.array_equal(out["vals"], ref["vals_after"][idx], equal_nan=True)
        assert np.array_equal(bits64(out["vals"][:, -s.nvar:]), bits64(ref["vals_after"][idx][:, -s.nvar:]))
        for k in range(len(idx)):
            d, d0 = out["d"][k], ref["d"][idx[k]]
            if not ok0[k]:
                assert (d == 7.0).all(), idx[k]
            elif nf0[k] == 1:
                fe = np.abs(d - d0).max() / np.abs(d0).max()
                worst_f = max(worst_f, fe)
                assert fe <= fwd_tol, (idx[k], fe)
    for k in range(len(idx)):   # (the decisions are those of every order by now)
        if out["ok"][k]:
            be = backward_error(s, out["vals"][k], rhs[k], out["d"][k])
            worst_b = max(worst_b, be)
            assert be <= bwd_tol, (idx[k], be)
    return worst_b, worst_f


def on_the_route(L):
    return L.config["kernel"] == "dense" and not L.config["float32"] and not L.config["band"] and L.info["ncond"] > 0


def main():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl
    for shape in (SMALLEST, SECOND):
        s = structure(shape)
        rows, cols = s.kkt_pattern()
        vals, rhs, ro = values(s, MIX)
        L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=MIX)
        assert on_the_route(L), L.config
        A = Args(s, MIX)
        A.fill(vals, rhs, ro)
        A.call(hipldl, L, hipldl.default_params())
        out = A.read()
        L.close()
        print(shape_id(shape), " ".join(hashlib.sha256(np.ascontiguousarray(out[k]).tobytes()).hexdigest()[:16] for k in sorted(out)))
    print("done")


if __name__ == "__main__":
    main()
