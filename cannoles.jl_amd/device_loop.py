"""Device-resident batched outer loop: B problems of one closed-form family are solved in
LOCKSTEP with everything in HBM between iterations.

`solve_batch_device` restates `SolverCore.solve!` (/root/reference/src/CaNNOLeS.jl:418-864), the Armijo `line_search`
(:1054-1112) and `small_residual` handling for a BATCH: every quantity of the single-problem loop (outer_loop.solve, the
numpy mirror that is pinned to the reference's known answers) becomes a [B, ...] tensor and every branch a mask, so each
problem follows exactly the decisions it would take alone.  One "global step" is one pass of the inner `while` for every
active problem.  The linear algebra of the path goes through the C ABI on device pointers:

    prepare_newton_system!  -> cnl_prepare_newton_system_dev      (row a4 / f2)
    rhs = [dual; primal], norms -> cnl_residual_vectors_dev       (row f1)
    newton_system!          -> cnl_newton_system_dev               (the hot path)
    xt, rt, dlambda cap, lambdat -> cnl_trial_point_dev            (row f1)
    least-squares multipliers -> cnl_cgls_multipliers_dev          (row f4)

Only the model callbacks (residuals, Jacobian / Hessian values) are torch expressions of a closed-form family
(`BandQuadFamily`; `BandQuadConFamily` with nonlinear constraints); `vals`, `rhs` and `d` never cross PCIe.  There is no CPU fallback.

Constraints.  A family whose `linear_constraints` is False (missing: True) provides `hess_cons_vals(X, LAM)`, the
coordinates of sum_k lam_k Hess c_k(x) on the Hessian structure: the loop evaluates it in front of every Newton system (H_c) and the
constraint Jacobian again at every trial point.  Above 1024 constraints the handle gets tuning cgls_wide = 1 (row f4).

Element types: `solve!` is generic in T, and so is this loop — a family built with dtype = float32 runs it in Float32 throughout
(a Float32 band handle, the `_f32_dev` passes, `cnl_outer_state_f32` and the `cnl_outer_*_f32_dev` kernels, ParamCaNNOLeS(Float32) and
the tolerances of eps(Float32)); nothing of a Float32 run is computed in Float64 except the reductions that csrc/outer_step.hip
documents.  A pattern without a Float32 band program raises CnlError: there is no fallback to Float64.
"""
import numpy as np


class BandQuadFamily:
    """Closed-form constrained NLS family on the band structure of synthetic.band_structure (BASELINE configs 3 / 4):
        F_i(x) = sum_{j in band(i)} A_ij x_j + q_i x_i^2 / 2 - y_i,        c_k(x) = sum_{j in block k} C_kj x_j - e_k.
    Jacobian values in the structure's COO order: A + [i == j] q_i x_i and C; sum_i r_i Hess F_i = diag(q r) on the
    lower-band Hessian structure (off-diagonal slots are structural zeros); the constraints are linear (zero Hessian).
    `host_model(b)` is the numpy twin of problem b with the callbacks outer_loop.solve expects (an NLPModels-like object).
    dtype = float32: the data is generated as for float64 and then rounded to float32; `h` keeps the rounded values as float64, so
    host_model(b) is the Float64 twin of exactly the data the device sees, and `d` and every device callback work in torch.float32."""

    def __init__(self, s, B, seed, torch, device, curvature=0.3, start=0.3, noise=0.01, dtype=np.float64):
        self.s, self.B, self.torch, self.device = s, int(B), torch, device
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.float64, np.float32):
            raise TypeError(f"BandQuadFamily({self.dtype}): Float64 and Float32 only")
        self.tdtype = torch.float32 if self.dtype == np.float32 else torch.float64
        n, m, p = s.nvar, s.nequ, s.ncon
        rng = np.random.default_rng(seed)
        jr, jc = np.asarray(s.jF[0]) - 1, np.asarray(s.jF[1]) - 1
        self.jr, self.jc = jr, jc
        A = np.where(jr == jc, 2.0 + rng.uniform(0, 1, (B, len(jr))), rng.uniform(-0.5, 0.5, (B, len(jr))))
        q = rng.uniform(-curvature, curvature, (B, n))
        xs = rng.normal(size=(B, n))                      # a point near which the residual is small
        cr, cc = (np.asarray(s.jc[0]) - 1, np.asarray(s.jc[1]) - 1) if p else (np.zeros(0, int), np.zeros(0, int))
        self.cr, self.cc = cr, cc
        Cv = rng.uniform(-1, 1, (B, len(cr)))
        # padded per-row entry lists: sums over a short fixed dimension instead of atomics (deterministic)
        self.row_ent = self._row_lists(jr, m, len(jr))
        self.crow_ent = self._row_lists(cr, p, len(cr)) if p else None
        self.h = dict(A=A, q=q, Cv=Cv, x0=xs + start * rng.normal(size=(B, n)))
        self.h["y"] = self._F_np(A, q, xs, np.zeros((B, m))) + noise * rng.normal(size=(B, m))
        self.h["e"] = self._c_np(Cv, xs, np.zeros((B, p)))
        if self.dtype == np.float32:
            self.h = {k: v.astype(np.float32).astype(np.float64) for k, v in self.h.items()}
        self.hr, self.hcl = np.asarray(s.hF[0]) - 1, np.asarray(s.hF[1]) - 1
        t = lambda a, dt=None: torch.as_tensor(a, dtype=dt or self.tdtype, device=device)
        self.d = {k: t(v) for k, v in self.h.items()}
        self.jr_t, self.jc_t = t(jr, torch.long), t(jc, torch.long)
        self.cc_t = t(cc, torch.long)
        self.row_ent_t = t(self.row_ent, torch.long)
        self.crow_ent_t = t(self.crow_ent, torch.long) if p else None
        self.jdiag_t = t((jr == jc).astype(np.float64))
        self.hdiag_t = t((self.hr == self.hcl).astype(np.float64))
        self.hr_t = t(self.hr, torch.long)

    def take(self, indices):
        """the family of the selected problems, in the given order: the structure (index lists, their tensors) is shared, the model data
        is copied — for running sub-batches"""
        idx = np.asarray(list(indices), dtype=np.int64)
        sub = object.__new__(type(self))
        sub.__dict__.update(self.__dict__)
        sub.B = len(idx)
        sub.h = {k: v[idx] for k, v in self.h.items()}
        idx_t = self.torch.as_tensor(idx, dtype=self.torch.long, device=self.device)
        sub.d = {k: v[idx_t].contiguous() for k, v in self.d.items()}
        return sub

    def per_problem_tensors(self):
        """the device tensors that hold one row per problem (the model's data), by name: what a caller that reorders the problems of a
        batch has to reorder with them (solve_batch_device(compact=True) hands them to cnl_outer_compact_dev)"""
        return dict(self.d)

    def head(self, nb):
        """the family of the first nb problems as VIEWS of this family's data (nothing is copied; `take` copies): the structure is
        shared, every callback works on [nb, ...] arrays"""
        nb = int(nb)
        if not 1 <= nb <= self.B:
            raise ValueError(f"head({nb}) of a family of {self.B} problems")
        sub = object.__new__(type(self))
        sub.__dict__.update(self.__dict__)
        sub.B = nb
        sub.h = {k: v[:nb] for k, v in self.h.items()}
        sub.d = {k: v[:nb] for k, v in self.d.items()}
        return sub

    @staticmethod
    def _row_lists(rows, nrows, pad):
        cnt = np.bincount(rows, minlength=nrows) if len(rows) else np.zeros(nrows, int)
        K = int(cnt.max()) if nrows else 0
        out = np.full((nrows, max(K, 1)), pad, np.int64)
        fill = np.zeros(nrows, int)
        for e, r in enumerate(rows):
            out[r, fill[r]] = e
            fill[r] += 1
        return out

    # ---- numpy forms (data generation and the host twins)
    def _F_np(self, A, q, x, y):
        prod = np.concatenate([A * x[:, self.jc], np.zeros((len(x), 1))], axis=1)
        return prod[:, self.row_ent].sum(axis=2) + 0.5 * q * x * x - y

    def _c_np(self, Cv, x, e):
        if self.s.ncon == 0:
            return np.zeros((len(x), 0))
        prod = np.concatenate([Cv * x[:, self.cc], np.zeros((len(x), 1))], axis=1)
        return prod[:, self.crow_ent].sum(axis=2) - e

    # ---- device callbacks, batched: X [B, n] -> ...
    def residual(self, X):
        t = self.torch
        prod = t.cat([self.d["A"] * X[:, self.jc_t], t.zeros((self.B, 1), dtype=self.tdtype, device=self.device)], dim=1)
        return prod[:, self.row_ent_t].sum(dim=2) + 0.5 * self.d["q"] * X * X - self.d["y"]

    def jac_vals(self, X):
        return self.d["A"] + self.jdiag_t * (self.d["q"] * X)[:, self.jr_t]

    def hess_vals(self, X, R):
        return self.hdiag_t * (self.d["q"] * R)[:, self.hr_t]

    def cons(self, X):
        t = self.torch
        if self.s.ncon == 0:
            return t.zeros((self.B, 1), dtype=self.tdtype, device=self.device)
        prod = t.cat([self.d["Cv"] * X[:, self.cc_t], t.zeros((self.B, 1), dtype=self.tdtype, device=self.device)], dim=1)
        return prod[:, self.crow_ent_t].sum(dim=2) - self.d["e"]

    def jacc_vals(self, X):
        return self.d["Cv"]

    def host_model(self, b):
        fam, s = self, self.s
        n, m, p = s.nvar, s.nequ, s.ncon
        A, q, y, Cv, e = (fam.h[k][b] for k in ("A", "q", "y", "Cv", "e"))

        class M:
            nvar, nequ, ncon = n, m, p
            x0 = fam.h["x0"][b].copy()
            h_rows, h_cols = np.asarray(s.hF[0]), np.asarray(s.hF[1])
            jF_rows, jF_cols = np.asarray(s.jF[0]), np.asarray(s.jF[1])
            jc_rows, jc_cols = (np.asarray(s.jc[0]), np.asarray(s.jc[1])) if p else (np.zeros(0, np.int64), np.zeros(0, np.int64))
            neval = 0

            def residual(self, x):
                self.neval += 1
                return fam._F_np(A[None], q[None], x[None], y[None])[0]

            def jac_residual(self, x):
                J = np.zeros((m, n))
                J[fam.jr, fam.jc] = A + (fam.jr == fam.jc) * (q * x)[fam.jr]
                return J

            def hess_coord_residual(self, x, r):
                return (fam.hr == fam.hcl) * (q * r)[fam.hr]

            def cons(self, x):
                return fam._c_np(Cv[None], x[None], e[None])[0]

            def jac(self, x):
                J = np.zeros((p, n))
                J[fam.cr, fam.cc] = Cv
                return J

            def hess_coord_cons(self, x, lam):
                return np.zeros(len(self.h_rows))

        return M()


class BandQuadConFamily(BandQuadFamily):
    """BandQuadFamily with NONLINEAR constraints: every block constraint gets a quadratic term of its own curvature g_k,
        c_k(x) = sum_{j in block k} (C_kj x_j + g_k x_j^2 / 2) - e_k,        g ~ U(-con_curvature, con_curvature),
    drawn behind every draw of the base class (the base data of a seed are those of BandQuadFamily), e such that c(xs) = 0.
    Jacobian values in COO order: C + g[row] x[col]; sum_k lam_k Hess c_k = diag_j(sum_{k: j in block k} lam_k g_k) on the model's
    Hessian structure s.hF (what hess_coord!(nls, x, lam; obj_weight = 0) returns; prepare negates it).  `linear_constraints = False`
    tells the loop to evaluate `hess_cons_vals` in front of every system and the constraint Jacobian at the trial point."""
    linear_constraints = False

    def __init__(self, s, B, seed, torch, device, curvature=0.3, start=0.3, noise=0.01, dtype=np.float64, con_curvature=0.2):
        super().__init__(s, B, seed, torch, device, curvature=curvature, start=start, noise=noise, dtype=dtype)
        n, m, p = s.nvar, s.nequ, s.ncon
        if p == 0:
            raise ValueError("BandQuadConFamily: a structure with constraints expected")
        # the base class's draws again, in its order (its generator is local to its constructor), for xs and the generator's state
        rng = np.random.default_rng(seed)
        nj = len(self.jr)
        rng.uniform(0, 1, (B, nj)), rng.uniform(-0.5, 0.5, (B, nj)), rng.uniform(-curvature, curvature, (B, n))
        xs = rng.normal(size=(B, n))
        rng.uniform(-1, 1, (B, len(self.cr)))
        x0 = xs + start * rng.normal(size=(B, n))
        rng.normal(size=(B, m))
        if not np.array_equal(x0.astype(self.dtype).astype(np.float64), self.h["x0"]):
            raise RuntimeError("BandQuadConFamily: the draws of BandQuadFamily are not the ones restated here")
        g = rng.uniform(-con_curvature, con_curvature, (B, p))
        self.ccol_ent = self._row_lists(self.cc, n, len(self.cr))   # per variable: the J_c entries of its column
        sq = np.concatenate([xs[:, self.cc] ** 2, np.zeros((B, 1))], axis=1)[:, self.crow_ent].sum(axis=2)
        new = dict(g=g, e=self.h["e"] + 0.5 * g * sq)
        if self.dtype == np.float32:
            new = {k: v.astype(np.float32).astype(np.float64) for k, v in new.items()}
        self.h.update(new)
        t = lambda a, dt=None: torch.as_tensor(a, dtype=dt or self.tdtype, device=device)
        self.d.update({k: t(v) for k, v in new.items()})
        self.cr_t = t(self.cr, torch.long)
        self.ccol_ent_t = t(self.ccol_ent, torch.long)

    def _c_np(self, Cv, x, e, g=None):
        """(the base class calls this with its own three arguments while it generates e for the linear part: g = None there)"""
        c = super()._c_np(Cv, x, e)
        if g is None:
            return c
        sq = np.concatenate([x[:, self.cc] ** 2, np.zeros((len(x), 1))], axis=1)[:, self.crow_ent].sum(axis=2)
        return c + 0.5 * g * sq

    def cons(self, X):
        t = self.torch
        zero = t.zeros((self.B, 1), dtype=self.tdtype, device=self.device)
        Xc = X[:, self.cc_t]
        prod = t.cat([self.d["Cv"] * Xc, zero], dim=1)
        sq = t.cat([Xc * Xc, zero], dim=1)
        return prod[:, self.crow_ent_t].sum(dim=2) + 0.5 * self.d["g"] * sq[:, self.crow_ent_t].sum(dim=2) - self.d["e"]

    def jacc_vals(self, X):
        return self.d["Cv"] + self.d["g"][:, self.cr_t] * X[:, self.cc_t]

    def hess_cons_vals(self, X, LAM):
        t = self.torch
        lg = t.cat([(LAM[:, :self.s.ncon] * self.d["g"])[:, self.cr_t], t.zeros((self.B, 1), dtype=self.tdtype, device=self.device)], dim=1)
        return self.hdiag_t * lg[:, self.ccol_ent_t].sum(dim=2)[:, self.hr_t]

    def host_model(self, b):
        fam, s = self, self.s
        n, p = s.nvar, s.ncon
        base = super().host_model(b)
        Cv, e, g = (fam.h[k][b] for k in ("Cv", "e", "g"))

        class M(type(base)):
            def cons(self, x):
                return fam._c_np(Cv[None], x[None], e[None], g[None])[0]

            def jac(self, x):
                J = np.zeros((p, n))
                J[fam.cr, fam.cc] = Cv + g[fam.cr] * x[fam.cc]
                return J

            def hess_coord_cons(self, x, lam):
                dj = np.bincount(fam.cc, weights=(lam * g)[fam.cr], minlength=n)
                return (fam.hr == fam.hcl) * dj[fam.hr]

        return M()


def kkt_pattern_of(fam, method="Newton"):
    """rows, cols (1-based int64) and the segment offsets, exactly as outer_loop.solve builds them from a model
    (/root/reference/src/CaNNOLeS.jl:276-315): with constraints the H_c segment has the model's Hessian structure.
    method = "Newton_noFHess" (Gauss-Newton): get_nnzh is 0 (hessian_approx.jl:12), the H_F segment is empty."""
    from .outer_loop import check_method
    check_method(method)
    s = fam.s
    n, m, p = s.nvar, s.nequ, s.ncon
    hr, hc = np.asarray(s.hF[0]), np.asarray(s.hF[1])
    nnzhF, nnzhc = (0 if method == "Newton_noFHess" else len(hr)), (len(hr) if p > 0 else 0)
    jFr, jFc = np.asarray(s.jF[0]), np.asarray(s.jF[1])
    jcr, jcc = (np.asarray(s.jc[0]), np.asarray(s.jc[1])) if p else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    N = n + m + p
    rows = np.concatenate([hr[:nnzhF], hr[:nnzhc], jFr + n, jcr + n + m, np.arange(n + 1, n + m + 1), np.arange(n + m + 1, N + 1), np.arange(1, n + 1)]).astype(np.int64)
    cols = np.concatenate([hc[:nnzhF], hc[:nnzhc], jFc, jcc, np.arange(n + 1, n + m + 1), np.arange(n + m + 1, N + 1), np.arange(1, n + 1)]).astype(np.int64)
    return rows, cols, (nnzhF, nnzhc, len(jFr), len(jcr))


def _element_type(fam, dtype):
    """(numpy dtype, is Float32) of a run: the family's by default; a run in another element type than the family's data is refused"""
    fdt = np.dtype(getattr(fam, "dtype", np.float64))
    dt = fdt if dtype is None else np.dtype(dtype)
    if dt not in (np.float64, np.float32):
        raise TypeError(f"element type {dt}: the lockstep loop runs in Float64 or Float32")
    if dt != fdt:
        raise TypeError(f"a {fdt} family cannot run in {dt}: build the family with dtype={dt} (the model data is rounded once, at construction)")
    return dt, dt == np.float32


def _element_ops(t, tdt, dev, f32):
    """(rdot, rsum, fdiv, fsqrt) for the loop's framework expressions.  Float64: the plain expressions.  Float32: the reductions as
    csrc/outer_step.hip computes them — exactly widened operands, summed in double, rounded to float once —, and quotient / square root
    rounded correctly (computed in double and rounded once, which gives the correctly rounded Float32 result; the framework's own
    Float32 division by a host scalar is a multiplication by its reciprocal)."""
    if not f32:
        return (lambda a, b: (a * b).sum(dim=1)), (lambda a: a.sum(dim=1)), (lambda a, b: a / b), t.sqrt
    wide = lambda a: a.double() if hasattr(a, "double") else t.full((), float(a), dtype=t.float64, device=dev)
    return (lambda a, b: (a.double() * b.double()).sum(dim=1).to(tdt)), (lambda a: a.double().sum(dim=1).to(tdt)), \
           (lambda a, b: (wide(a) / wide(b)).to(tdt)), (lambda a: a.double().sqrt().to(tdt))


PROFILE = False   # tools/time_device_loop.py --profile: wall time per section of a global step (synchronises at every section)


def solve_batch_device(fam, params=None, max_steps=400, max_inner=10000, atol=None, rtol=None, Fatol=None, Frtol=None, delta_dec=0.1,
                       device_index=0, layout="auto", tuning=None, dtype=None, compact=False, compact_min_finished=None, method="Newton",
                       x=None, lam=None, use_initial_multiplier=False, max_iter=-1, max_eval=100000, max_time=None,
                       always_accept_extrapolation=False):
    """All B problems of `fam` in lockstep on the device.  Returns a dict of numpy arrays: solution [B, n], multipliers,
    status (list of strings), iter, nfact, nlinsolve, nbk, neval, objective, and `steps` (global steps = batched Newton rounds);
    `jct_shared` (one constraint-Jacobian array serves the current and the trial point: linear constraints) and the handle's `cgls_wide`.

    The keywords of the reference's `solve!` (src/CaNNOLeS.jl:418-437) and of its solver constructor (:228-271):
      method   "Newton"; "Newton_noFHess" (Gauss-Newton: no H_F segment in the pattern, `fam.hess_vals` is never called and need not
               exist); "Newton_vanishing" (a problem's H_F values are refreshed only while dot(Fx, Fx) > 1e-8, cnl_outer_hess_mask_dev;
               the result reports `hess_skipped`, the skipped refreshes per problem).  "LM" and unknown names raise ValueError.
      x        [B, n] start points (default: the family's x0);  lam [B, p] with use_initial_multiplier = True: the start multipliers
               instead of the least-squares estimate (:512-518)
      max_iter, max_eval   per problem, < 0: no limit; statuses `max_iter`, `max_eval`.  `neval` counts what the problem's
               single-problem run evaluates: residual (and constraints, when p > 0) at the start point, at every extrapolation trial point
               and at every line-search candidate — not the evaluations this loop makes on rows that did not need them
      max_time seconds of wall clock for the WHOLE batch (None: no limit), looked at once per global step: the problems still active then
               end with status `max_time`
      always_accept_extrapolation   (:627, :735)

    compact=True: a global step runs on the ACTIVE problems only.  Behind every step cnl_outer_compact_dev moves the active problems to
    the front of every per-problem array (the state, a working copy of the family's data, the row -> problem map), once at least
    `compact_min_finished` problems have finished since the last pass (default max(32, working batch // 8): a policy knob, no result
    depends on it); the loop goes on with that prefix — the state's B, the handle (cnl_set_active_batch; a handle that cannot, e.g. a
    staged one, stays at the full batch and works on finished rows as before) and every framework expression on prefix views.  The
    counts come back with the next step's branch flags: no further host synchronisation.  Every problem takes the decisions it takes
    without compaction, the outputs are in the original problem order and `fam` is not touched.  The result then also holds
    `compactions`, `problem_steps` (the sum of the working batch over the global steps; steps * B without compaction) and
    `handle_shrunk`.

    Round 4: the masks and the masked state updates of a global step are FOUR device kernels working in place on the state
    (cnl_outer_begin_dev / _newton_done_dev / _trial_done_dev / _end_dev, csrc/outer_step.hip) instead of ~150 framework launches;
    the step costs two host reads of a few flag words.  The model callbacks, the Armijo line search and the rare small-residual
    branch are still framework expressions."""
    import ctypes as C
    from . import hipldl
    t = fam.torch
    dev = fam.device
    dt, f32 = _element_type(fam, dtype)
    tdt = t.float32 if f32 else t.float64
    eps = float(np.finfo(dt).eps)
    atol = np.sqrt(eps) if atol is None else atol
    rtol = np.sqrt(eps) if rtol is None else rtol
    Fatol = np.sqrt(eps) if Fatol is None else Fatol
    Frtol = eps if Frtol is None else Frtol
    params = hipldl.default_params(dt) if params is None else np.ascontiguousarray(params, dtype=dt)
    dmin, rhomax, gammaA = float(params[1]), float(params[6]), float(params[8])
    s, B = fam.s, fam.B
    n, m, p = s.nvar, s.nequ, s.ncon
    N = n + m + p
    P = max(p, 1)
    rows, cols, (nnzhF, nnzhc, nnzjF, nnzjc) = kkt_pattern_of(fam, method)   # (refuses "LM" and unknown names)
    nnz = len(rows)
    vanishing = method == "Newton_vanishing"
    max_iter, max_eval = int(max_iter), int(max_eval)
    epp = 2 if p > 0 else 1   # evaluations per point: residual, and constraints when there are any (eval_fun, :559)
    import time as _time
    t_start = _time.perf_counter()
    # tuning: further hipldl.Options fields for the handle — e.g. {"band_pieces": 20}: a constrained family's pattern (H_c as wide as H_F)
    # on the wide band kernels, which a Float64 handle takes on request only
    tuning = dict(tuning or {})
    if p > 1024:   # row f4 keeps its ncon-vectors in LDS up to 1024 constraints; above, the instance with them in the handle's workspace
        tuning.setdefault("cgls_wide", 1)
    # a family with nonlinear constraints (fam.linear_constraints False; missing: linear): H_c = sum_k lam_k Hess c_k from
    # fam.hess_cons_vals in front of every system, and a constraint Jacobian of its own for the trial point
    nonlinear = p > 0 and not getattr(fam, "linear_constraints", True)
    # `vals` interleaved over groups of 32 problems where the band kernels serve the batch (cnl_options.batch_layout, round 6): row f2
    # writes that layout, newton_system reads it; rows f1 / f4 read the Jacobian values from the model's arrays, whatever the layout
    L = None
    if layout in ("auto", "interleaved"):
        try:
            L = hipldl.HIPLDLStruct(N, rows, cols, None, n, m, p, batch=B, device=device_index,
                                    options=hipldl.Options(batch_layout=hipldl.LAYOUT_INTERLEAVED, **tuning), dtype=dt)
        except hipldl.CnlError:
            if layout == "interleaved":
                raise
    if L is None:
        L = hipldl.HIPLDLStruct(N, rows, cols, None, n, m, p, batch=B, device=device_index, options=hipldl.Options(**tuning) if tuning else None,
                                dtype=dt)
    lib = hipldl.lib()
    f64 = dict(dtype=tdt, device=dev)   # (the run's element type)
    rdot, rsum, fdiv, fsqrt = _element_ops(t, tdt, dev, f32)
    huge = float("inf") if f32 else 1e60   # T(1e60), src/CaNNOLeS.jl:638, 647
    Z = lambda *sh: t.zeros(sh, **f64)
    ZI = lambda dt, *sh: t.zeros(sh, dtype=dt, device=dev)
    o_I = nnzhF + nnzhc + nnzjF + nnzjc

    st = t.cuda.current_stream(dev).cuda_stream
    ptr = lambda a: a.data_ptr()

    def new_vals():
        v = t.ones((B, nnz), **f64)
        v[:, o_I:o_I + m] = -1.0     # the -I block is set once (src/CaNNOLeS.jl:306); prepare never writes it
        if L.config.get("batch_layout"):
            vi = t.empty(hipldl.layout_len(L, 0), **f64)
            hipldl.interleave_dev(L, 0, ptr(v), ptr(vi), st)
            return vi
        return v

    vals_cur = new_vals()   # (ONE vals array: only newton_system reads it; the trial point's products read Jt)
    hc0 = Z(B, max(nnzhc, 1))
    # compaction (compact=True): nb = the working batch, the first nb rows of every array; hd(a) = those rows of a; wf = the family
    # whose data rows follow the state's (a working copy: `fam` stays as it is), fw = its first nb problems.  Without compaction nb = B,
    # hd(a) is all of a and fw is fam.  `vals_cur` needs no reordering: prepare rewrites every problem's values in front of each use
    # (the -I segment is the same for all).
    nb = B
    hd = lambda a: a[:nb]
    wf = fw = fam
    L_nb = B             # the handle's active batch
    hF_full = hc_full = None

    def prepare(vals, hF, Jv_, Jcv_, delta_):
        nonlocal hF_full, hc_full
        if hF is not None and hF.shape[0] < L_nb:   # a handle that could not shrink reads a Hessian row for every problem it was created with
            if hF_full is None:
                hF_full = Z(B, hF.shape[1])
            hF_full[:hF.shape[0]].copy_(hF)
            hF = hF_full
        hc = hc0
        if nonlinear:   # sum_k lam_k Hess c_k at the current point and multipliers, fresh for every problem (prepare negates it)
            hc = fw.hess_cons_vals(hd(x), hd(lam)).contiguous()
            if hc.shape[0] < L_nb:   # (as hF above)
                if hc_full is None:
                    hc_full = Z(B, hc.shape[1])
                hc_full[:hc.shape[0]].copy_(hc)
                hc = hc_full
        hipldl.prepare_newton_system_dev(L, nnzhF, nnzhc, nnzjF, nnzjc, ptr(hF) if hF is not None else 0, ptr(hc) if p else 0, ptr(Jv_),
                                         ptr(Jcv_) if p else 0, ptr(delta_) if p else 0, ptr(vals), st)

    def resid_vectors(Jv_, Jcv_, r_, lam_, F_, c_, rhs_out, nrm_out):
        """[dual; primal] = [Jx'r - Jc'lam; F - r; c] and the two infinity norms; the Jacobian values come from the model's arrays
        (cnl_residual_vectors_jac_dev: no prepare pass in front — round 6; rounds 2-5 copied them into `vals` first)"""
        hipldl.residual_vectors_jac_dev(L, nnzjF, nnzjc, ptr(Jv_), ptr(Jcv_) if p else 0, ptr(r_), ptr(lam_) if p else 0, ptr(F_), ptr(c_) if p else 0,
                                        ptr(rhs_out), ptr(nrm_out), st)

    def multipliers(Jv_, Jcv_, r_, ones_if_zero):
        lam_ = Z(B, P)
        if p:
            hipldl.cgls_multipliers_jac_dev(L, nnzjF, nnzjc, ptr(Jv_), ptr(Jcv_), ptr(r_), ptr(lam_), 0, None, None, 0, ones_if_zero, 0, st)
        return lam_

    W = lambda mask, a, b: t.where(mask if a.dim() == 1 else mask[:, None], a, b)
    smax = 100.0
    dual_scaling = lambda l_: fdiv(t.clamp(fdiv(rsum(l_.abs()), p), min=smax), smax) if p > 0 else t.ones(B, **f64)
    ninf = lambda a: a.abs().max(dim=1).values if a.shape[1] else Z(B)
    cnorm2 = lambda c_: fsqrt(rdot(c_, c_)) if p else Z(B)

    # ---- state (every array is updated IN PLACE from here on: the kernels hold its address) -------------------------
    if x is None:
        x = fam.d["x0"].clone()
    else:
        x = t.as_tensor(np.ascontiguousarray(x, dtype=dt), **f64).clone()
        if tuple(x.shape) != (B, n):
            raise ValueError(f"x: [{B}, {n}] start points expected, got {tuple(x.shape)}")
    Fx = fam.residual(x).contiguous()
    fx = (0.5 * rdot(Fx, Fx)).contiguous()
    Jv = fam.jac_vals(x).contiguous()
    Jcv = fam.jacc_vals(x)          # linear constraints: one array serves the current and the trial point
    # (a linear family hands out its own array; with compaction the state's rows change places, so the state gets a copy)
    Jcv = (Jcv.clone() if compact or nonlinear else Jcv.contiguous()) if p else Z(B, 1)
    cx = fam.cons(x).contiguous()
    r = Fx.clone()
    delta = t.ones(B, **f64)
    if use_initial_multiplier:   # :512-518: no least-squares estimate, no ones-if-zero rule
        lam0 = np.zeros((B, p), dt) if lam is None else np.ascontiguousarray(lam, dtype=dt)
        if lam0.shape != (B, p):
            raise ValueError(f"lam: [{B}, {p}] start multipliers expected, got {lam0.shape}")
        lam = Z(B, P)
        lam[:, :p] = t.as_tensor(lam0, **f64)
    else:
        lam = multipliers(Jv, Jcv, r, True)
    rhs_cur, nrm0 = Z(B, N), Z(B, 2)
    resid_vectors(Jv, Jcv, r, lam, Fx, cx, rhs_cur, nrm0)
    normdual, normprimal = nrm0[:, 0].clone(), nrm0[:, 1].clone()
    epsF = (Fatol + Frtol * 2 * fsqrt(fx)).contiguous()
    epstol = (atol + rtol * normdual).contiguous()
    epsc = fsqrt(epstol).contiguous()

    rv_rhs, rv_nrm = Z(B, N), Z(B, 2)

    def small_res_check(mask):
        """src/CaNNOLeS.jl:873-897 for the problems of `mask`: r = F, least-squares multipliers, dual, primal = [0; c] (in place; the
        working rows only — the handle's passes take whole arrays, whose other rows are not used)"""
        mask = hd(mask)
        r2 = r.clone()
        hd(r2).copy_(W(mask, hd(Fx), hd(r)))
        lam2 = multipliers(Jv, Jcv, r2, False)
        hd(lam).copy_(W(mask, hd(lam2), hd(lam)))
        resid_vectors(Jv, Jcv, r2, lam, r2, cx, rv_rhs, rv_nrm)   # F - r = 0 for the masked problems
        hd(rhs_cur).copy_(W(mask, hd(rv_rhs), hd(rhs_cur)))
        hd(normdual).copy_(W(mask, hd(rv_nrm)[:, 0], hd(normdual)))
        hd(normprimal).copy_(W(mask, ninf(hd(cx)[:, :p]) if p else Z(nb), hd(normprimal)))
        hd(r).copy_(hd(r2))

    small_residual = (2 * fsqrt(fx) <= epsF) & (cnorm2(cx) <= epsc)
    first_order = t.maximum(normdual / dual_scaling(lam), normprimal) <= epstol
    chk0 = small_residual & ~first_order
    if bool(chk0.any()):
        small_res_check(chk0)
        first_order = t.maximum(normdual / dual_scaling(lam), normprimal) <= epstol
    UNKNOWN, FIRST, SMALL, EXC, TIRED, STALL, MAX_ITER, MAX_TIME = 0, 1, 2, 3, 4, 5, 6, 7
    # the evaluation at the start point; `tired` (:559) may hold already with a tiny limit.  (it = 0 never exceeds a max_iter >= 0)
    neval = t.full((B,), epp, dtype=t.int64, device=dev)
    start_rest = TIRED if 0 <= max_eval < epp else UNKNOWN
    status = t.where(first_order, FIRST, t.where(small_residual, SMALL, start_rest)).to(t.int32).contiguous()
    eta = t.full((B,), 1.0 if p else 0.0, **f64)
    epsk = t.full((B,), 1e3, **f64)
    rho_old = Z(B)
    it, inner = ZI(t.int32, B), ZI(t.int64, B)
    # :Newton_vanishing: the H_F values each problem's system holds (zero until its first refresh), this step's refresh mask, the skips
    hess_upd = t.zeros(B, dtype=t.bool, device=dev)
    hF_cur, hess_skipped = (Z(B, nnzhF), ZI(t.int64, B)) if vanishing else (None, None)
    nfact, nlin, nbk = ZI(t.int64, B), ZI(t.int64, B), ZI(t.int64, B)
    phase0 = t.ones(B, dtype=t.bool, device=dev)
    combined, combined_hat = Z(B), Z(B)
    ndh, nph = normdual.clone(), normprimal.clone()
    d = Z(B, N)
    xt, rt, lamt, Ft, ct = x.clone(), r.clone(), lam.clone(), Fx.clone(), cx.clone()
    Jt = Jv.clone()
    # nonlinear constraints: Jcv belongs to the current point (the line search's dual part, the rejected-extrapolation branch, the
    # small-residual check, the start-up multipliers), Jct to the trial point; cnl_outer_trial_done_dev copies Jct to Jcv on acceptance
    Jct = Jcv.clone() if nonlinear else Jcv
    rhs_t, nrm_t = Z(B, N), Z(B, 2)
    d_new, rho_new, ro_tmp = Z(B, N), Z(B), Z(B)
    nf_new, ok_new = ZI(t.int32, B), ZI(t.int32, B)
    xt_e, rt_e, lamt_e, dlam_e = Z(B, n), Z(B, m), Z(B, P), Z(B, P)
    xl, Fl, cl, lam_ls = Z(B, n), Z(B, m), Z(B, P), Z(B, P)
    alpha, Dphi, phix = Z(B), Z(B), Z(B)
    masks = {k: t.zeros(B, dtype=t.bool, device=dev) for k in ("act", "need", "brk", "ext", "lsm", "rej", "chk", "done_in", "tired", "small_res", "bt")}
    # the step's flag words and, behind them, the two counts of cnl_outer_compact_dev: one block, one pinned copy per read
    flags_counts = ZI(t.int32, 10)
    flags, counts = flags_counts[:8], flags_counts[8:]
    flags_h = t.zeros(10, dtype=t.int32).pin_memory()
    S = hipldl.cnl_outer_state_f32() if f32 else hipldl.cnl_outer_state()
    for k, v in dict(B=B, n=n, m=m, p=p, P=P, N=N, nnzjF=nnzjF, nnzjc=nnzjc, max_inner=max_inner, dmin=dmin, rhomax=rhomax,
                     delta_dec=delta_dec, smax=smax, gammaA=gammaA, eps2=eps ** 2).items():
        setattr(S, k, v)
    arrays = dict(status=status, it=it, flags=flags, nf_new=nf_new, ok_new=ok_new, inner=inner, nfact=nfact, nlin=nlin, phase0=phase0,
                  normdual=normdual, normprimal=normprimal, combined=combined, combined_hat=combined_hat, delta=delta, ndh=ndh, nph=nph, fx=fx,
                  epsk=epsk, epstol=epstol, epsF=epsF, epsc=epsc, rho_old=rho_old, d=d, d_new=d_new, ro_tmp=ro_tmp, rho_new=rho_new,
                  x=x, r=r, Fx=Fx, cx=cx, Jv=Jv, Jcv=Jcv, lam=lam, rhs_cur=rhs_cur, xt=xt, rt=rt, Ft=Ft, ct=ct, Jt=Jt, Jct=Jct, lamt=lamt,
                  rhs_t=rhs_t, nrm_t=nrm_t, xt_e=xt_e, rt_e=rt_e, lamt_e=lamt_e, ls_g=rv_rhs, xl=xl, Fl=Fl, cl=cl, lam_ls=lam_ls, alpha=alpha,
                  Dphi=Dphi, phix=phix, eta=eta, nbk=nbk, **masks)
    for k, v in arrays.items():
        assert v.is_contiguous(), k
        setattr(S, k, v.data_ptr())
    Sref = C.byref(S)
    ctl = hipldl.outer_ctl(neval.data_ptr(), epp, always_accept_extrapolation, max_iter, max_eval, hess_upd.data_ptr())
    Cref = C.byref(ctl)
    chk_ = hipldl._check
    sfx = "_f32_dev" if f32 else "_dev"
    k_begin, k_newton_done, k_extrapolated, k_trial_done, k_end, k_ls_begin, k_ls_test, k_ls_step, k_ls_take, k_hess_mask = (
        getattr(lib, "cnl_outer_" + k + sfx) for k in ("begin_ex", "newton_done", "extrapolated", "trial_done_ex", "end_ex", "ls_begin", "ls_test_ex",
                                                       "ls_step", "ls_take", "hess_mask"))

    def read_flags():
        flags_h.copy_(flags_counts, non_blocking=True)
        t.cuda.current_stream(dev).synchronize()
        return flags_h.tolist()

    prof = {} if PROFILE else None

    def tick(name, t0):
        if prof is not None:
            t.cuda.synchronize(dev)
            prof[name] = prof.get(name, 0.0) + (_time.perf_counter() - t0)
        return _time.perf_counter()

    compactions = problem_steps = 0
    handle_shrunk, can_shrink, pending = False, True, False
    if compact:
        if compact_min_finished is not None and int(compact_min_finished) < 1:
            raise ValueError("compact_min_finished >= 1")
        wf = fam.head(B)
        wf.d = {k: v.clone() for k, v in fam.per_problem_tensors().items()}
        fw = wf
        extras = [(v.data_ptr(), v.shape[1] * v.element_size()) for v in wf.d.values() if v.shape[1] > 0]
        extras.append((neval.data_ptr(), 8))   # (per-problem arrays of the control block and of :Newton_vanishing move with the state)
        if vanishing:
            extras += [(hF_cur.data_ptr(), nnzhF * hF_cur.element_size()), (hess_skipped.data_ptr(), 8)]
        assert all(v.is_contiguous() and v.shape[0] == B for v in wf.d.values())
        orig = t.arange(B, dtype=t.int32, device=dev)
        pair_work = ZI(t.int32, B + 2)
    t.cuda.synchronize(dev)
    t_loop0 = _time.perf_counter()
    steps = 0
    # host synchronisations per global step: one for the branch flags of cnl_outer_begin_dev, one for (rejected, small-residual) behind
    # cnl_outer_trial_done_dev, and one per round of backtracking when a line search runs
    while steps < max_steps:
        tk = _time.perf_counter()
        chk_(k_begin(Sref, Cref, st))   # (behind a compaction still over the rows of the step before: the ones that left are finished)
        fl = read_flags()
        any_act, any_need, any_ext, any_ls = fl[:4]
        if not any_act:
            break
        moved, pending = pending and fl[9] < nb, False
        if moved:   # the active problems are the first fl[8] = fl[9] rows now
            nb = int(fl[9])
            compactions += 1
            S.B = nb
            fw = wf.head(nb)
            if can_shrink:
                try:
                    hipldl.set_active_batch(L, nb)
                    L_nb, handle_shrunk = nb, True
                except hipldl.CnlError as err:
                    if err.code != 5:   # CNL_ERR_STATE: this handle cannot work on a prefix (staged, split, dense) — it keeps its batch
                        raise
                    can_shrink = False
        steps += 1
        problem_steps += nb
        tk = tick("begin", tk)
        # ---- Newton step (skipped on the iteration right after a rejected extrapolation), :627-652
        if any_need:
            if nnzhF == 0:          # Gauss-Newton: no H_F segment, no Hessian callback
                prepare(vals_cur, None, Jv, Jcv, delta)
            elif vanishing:         # the problems due a system refresh their H_F values where dot(Fx, Fx) > 1e-8 and keep them otherwise
                chk_(k_hess_mask(Sref, Cref, st))
                due = hd(masks["need"])
                hd(hF_cur).copy_(t.where((due & hd(hess_upd))[:, None], fw.hess_vals(hd(x), hd(r)), hd(hF_cur)))
                hd(hess_skipped).add_((due & ~hd(hess_upd)).to(t.int64))
                prepare(vals_cur, hF_cur, Jv, Jcv, delta)
            else:
                prepare(vals_cur, fw.hess_vals(hd(x), hd(r)), Jv, Jcv, delta)
            hd(ro_tmp).copy_(hd(rho_old))
            hipldl.newton_system_dev(L, ptr(vals_cur), ptr(rhs_cur), ptr(d_new), ptr(ro_tmp), ptr(rho_new), ptr(nf_new), ptr(ok_new), params, st)
        chk_(k_newton_done(Sref, 1 if any_need else 0, st))
        dx = d[:, :n]
        tk = tick("newton", tk)
        # ---- extrapolation step, :654-668
        if any_ext:   # (a superset test: problems that broke above are masked out by `ext`)
            hipldl.trial_point_dev(L, ptr(x), ptr(r), ptr(lam) if p else 0, ptr(d), 1e4, ptr(xt_e), ptr(rt_e), ptr(lamt_e) if p else 0,
                                   ptr(dlam_e) if p else 0, st)
            chk_(k_extrapolated(Sref, st))
        tk = tick("extrapolation", tk)
        # ---- Armijo line search on the merit function, :1054-1112
        if any_ls:
            resid_vectors(Jv, Jcv, Fx, lam_ls, Fx, cx, rv_rhs, rv_nrm)      # dual part: Jx'Fx - Jc'(lam - c/delta), lam_ls by cnl_outer_newton_done_dev
            chk_(k_ls_begin(Sref, st))
            hd(Fl).copy_(fw.residual(hd(xl)))
            hd(cl).copy_(fw.cons(hd(xl)))
            chk_(k_ls_test(Sref, 1, Cref, st))
            while read_flags()[6]:
                chk_(k_ls_step(Sref, st))
                hd(Fl).copy_(fw.residual(hd(xl)))       # (rows of problems that do not backtrack are recomputed from an unchanged xl: same values)
                hd(cl).copy_(fw.cons(hd(xl)))
                chk_(k_ls_test(Sref, 0, Cref, st))
            chk_(k_ls_take(Sref, st))
        tk = tick("line_search", tk)
        hd(Ft).copy_(fw.residual(hd(xt)))
        hd(ct).copy_(fw.cons(hd(xt)))
        # ---- optimality measures at the trial point, :722-732; acceptance and the state update, :733-800
        hd(Jt).copy_(fw.jac_vals(hd(xt)))
        if nonlinear:
            hd(Jct).copy_(fw.jacc_vals(hd(xt)))
        resid_vectors(Jt, Jct, rt, lamt, Ft, ct, rhs_t, nrm_t)
        tk = tick("trial_eval", tk)
        chk_(k_trial_done(Sref, Cref, st))
        any_rej, any_chk = read_flags()[4:6]
        tk = tick("trial_done", tk)
        if any_rej:   # dual at (x, r, lam) again; primal keeps the trial's value, as in the reference (:742-747)
            resid_vectors(Jv, Jcv, r, lam, Fx, cx, rv_rhs, rv_nrm)
            hd(rhs_cur)[:, :n] = t.where(hd(masks["rej"])[:, None], hd(rv_rhs)[:, :n], hd(rhs_cur)[:, :n])
        if any_chk:
            small_res_check(masks["chk"])
        chk_(k_end(Sref, Cref, st))
        if max_time is not None and _time.perf_counter() - t_start > max_time:
            status.masked_fill_(status == UNKNOWN, MAX_TIME)   # (the clock is the caller's: code 7 is never written by a kernel)
            break
        if compact and nb > 1:
            # the problems that just finished leave the working rows (once enough of them have); the counts come back with the next
            # step's flags
            hipldl.outer_compact_dev(S, extras, compact_min_finished if compact_min_finished is not None else max(32, nb // 8), orig, counts,
                                     pair_work, st)
            pending = True
        tk = tick("rej_chk_end", tk)
    t.cuda.synchronize(dev)
    loop_seconds = _time.perf_counter() - t_loop0
    names = hipldl.OUTER_STATUS_NAMES
    if compact:   # row b of every array holds problem orig[b]: back to the original order
        where = orig.cpu().numpy().astype(np.int64)
        assert np.array_equal(np.sort(where), np.arange(B))

        def host(a):
            a = a.cpu().numpy()
            out_ = np.empty_like(a)
            out_[where] = a
            return out_
    else:
        host = lambda a: a.cpu().numpy()
    out = {"solution": host(x), "multipliers": host(lam[:, :p]), "status": [names[int(v)] for v in host(status)],
           "iter": host(it), "nfact": host(nfact), "nlinsolve": host(nlin), "nbk": host(nbk), "neval": host(neval),
           "objective": host(fx), "dtype": str(dt), "r": host(r), "normdual": host(normdual),
           "normprimal": host(normprimal), "epstol": host(epstol), "steps": steps, "kernel": "band" if L.config.get("band") else L.config["kernel"], "vals_layout": "interleaved" if L.config.get("batch_layout") else "problem-major",
           "loop_seconds": loop_seconds,   # the global steps alone (the symbolic analysis of the pattern and the start-up evaluations are not in it)
           "jct_shared": S.Jct == S.Jcv,   # one constraint-Jacobian array for the current and the trial point (linear constraints)
           "cgls_wide": L.config["cgls_wide"]}
    if vanishing:
        out["hess_skipped"] = host(hess_skipped)
    if compact:
        out.update(compactions=compactions, problem_steps=problem_steps, handle_shrunk=handle_shrunk)
    if prof is not None:
        out["profile_ms_per_step"] = {k: 1e3 * v / max(steps, 1) for k, v in prof.items()}
    L.close()
    return out


def solve_batch_device_framework(fam, params=None, max_steps=400, max_inner=10000, atol=None, rtol=None, Fatol=None, Frtol=None, delta_dec=0.1,
                       device_index=0, dtype=None):
    """The loop as rounds 2-3 ran it: masks and masked state updates as ~150 framework launches per global step.  Kept as the
    executable restatement solve_batch_device is compared with (tests/test_gpu_parity.py).
    All B problems of `fam` in lockstep on the device.  Returns a dict of numpy arrays: solution [B, n], multipliers,
    status (list of strings), iter, nfact, nlinsolve, nbk, objective, and `steps` (global steps = batched Newton rounds)."""
    from . import hipldl
    t = fam.torch
    dev = fam.device
    dt, f32 = _element_type(fam, dtype)
    tdt = t.float32 if f32 else t.float64
    eps = float(np.finfo(dt).eps)
    atol = np.sqrt(eps) if atol is None else atol
    rtol = np.sqrt(eps) if rtol is None else rtol
    Fatol = np.sqrt(eps) if Fatol is None else Fatol
    Frtol = eps if Frtol is None else Frtol
    params = hipldl.default_params(dt) if params is None else np.ascontiguousarray(params, dtype=dt)
    dmin, rhomax, gammaA = float(params[1]), float(params[6]), float(params[8])
    s, B = fam.s, fam.B
    n, m, p = s.nvar, s.nequ, s.ncon
    N = n + m + p
    P = max(p, 1)
    if p > 0 and not getattr(fam, "linear_constraints", True):
        raise ValueError("solve_batch_device_framework restates the loop for linear constraints (H_c = 0, one constraint Jacobian): "
                         "a family with nonlinear constraints runs in solve_batch_device")
    rows, cols, (nnzhF, nnzhc, nnzjF, nnzjc) = kkt_pattern_of(fam)
    nnz = len(rows)
    L = hipldl.HIPLDLStruct(N, rows, cols, None, n, m, p, batch=B, device=device_index, dtype=dt)
    f64 = dict(dtype=tdt, device=dev)   # (the run's element type)
    rdot, rsum, fdiv, fsqrt = _element_ops(t, tdt, dev, f32)
    huge = float("inf") if f32 else 1e60   # T(1e60), src/CaNNOLeS.jl:638, 647
    Z = lambda *sh: t.zeros(sh, **f64)
    o_I = nnzhF + nnzhc + nnzjF + nnzjc

    def new_vals():
        v = t.ones((B, nnz), **f64)
        v[:, o_I:o_I + m] = -1.0     # the -I block is set once (src/CaNNOLeS.jl:306); prepare never writes it
        return v

    vals_cur, vals_t = new_vals(), new_vals()
    hc0 = Z(B, max(nnzhc, 1))
    st = t.cuda.current_stream(dev).cuda_stream
    ptr = lambda a: a.data_ptr()

    def prepare(vals, hF, Jv, Jcv, delta):
        hipldl.prepare_newton_system_dev(L, nnzhF, nnzhc, nnzjF, nnzjc, ptr(hF) if hF is not None else 0, ptr(hc0) if p else 0, ptr(Jv),
                                         ptr(Jcv) if p else 0, ptr(delta) if p else 0, ptr(vals), st)

    rv_rhs, rv_nrm = Z(B, N), Z(B, 2)

    def resid_vectors(vals, r_, lam_, F_, c_):
        """[dual; primal] = [Jx'r - Jc'lam; F - r; c] and the two infinity norms, from the J segments of `vals`"""
        rv_nrm.zero_()
        hipldl.residual_vectors_dev(L, ptr(vals), ptr(r_), ptr(lam_) if p else 0, ptr(F_), ptr(c_) if p else 0, ptr(rv_rhs), ptr(rv_nrm), st)
        return rv_rhs.clone(), rv_nrm[:, 0].clone(), rv_nrm[:, 1].clone()

    def multipliers(vals, r_, ones_if_zero):
        lam_ = Z(B, P)
        if p:
            hipldl.cgls_multipliers_dev(L, ptr(vals), ptr(r_), ptr(lam_), 0, None, None, 0, ones_if_zero, 0, st)
        return lam_

    W = lambda mask, a, b: t.where(mask if a.dim() == 1 else mask[:, None], a, b)
    smax = 100.0
    dual_scaling = lambda l_: fdiv(t.clamp(fdiv(rsum(l_.abs()), p), min=smax), smax) if p > 0 else t.ones(B, **f64)
    ninf = lambda a: a.abs().max(dim=1).values if a.shape[1] else Z(B)

    # ---- start, src/CaNNOLeS.jl:470-560
    x = fam.d["x0"].clone()
    Fx = fam.residual(x)
    fx = 0.5 * rdot(Fx, Fx)
    Jv, Jcv = fam.jac_vals(x), fam.jacc_vals(x)
    cx = fam.cons(x)
    r = Fx.clone()
    delta = t.ones(B, **f64)
    prepare(vals_cur, None, Jv, Jcv, delta)
    lam = multipliers(vals_cur, r, True)
    rhs_cur, normdual, normprimal = resid_vectors(vals_cur, r, lam, Fx, cx)
    epsF = Fatol + Frtol * 2 * fsqrt(fx)
    epstol = atol + rtol * normdual
    epsc = fsqrt(epstol)
    cnorm2 = lambda c_: fsqrt(rdot(c_, c_)) if p else Z(B)

    def small_res_check(mask, lam, rhs_cur, normdual, normprimal, r):
        """src/CaNNOLeS.jl:873-897 for the problems of `mask`: r = F, least-squares multipliers, dual, primal = [0; c]"""
        r2 = W(mask, Fx, r)
        prepare(vals_cur, None, Jv, Jcv, delta)
        lam2 = multipliers(vals_cur, r2, False)
        lam_n = W(mask, lam2, lam)
        rhs2, nd2, _ = resid_vectors(vals_cur, r2, lam_n, r2, cx)   # F - r = 0 for the masked problems
        rhs_n = W(mask, rhs2, rhs_cur)
        return lam_n, rhs_n, W(mask, nd2, normdual), W(mask, ninf(cx[:, :p]) if p else Z(B), normprimal), r2

    small_residual = (2 * fsqrt(fx) <= epsF) & (cnorm2(cx) <= epsc)
    first_order = t.maximum(normdual / dual_scaling(lam), normprimal) <= epstol
    chk = small_residual & ~first_order
    if bool(chk.any()):
        lam, rhs_cur, normdual, normprimal, r = small_res_check(chk, lam, rhs_cur, normdual, normprimal, r)
        first_order = t.maximum(normdual / dual_scaling(lam), normprimal) <= epstol
    UNKNOWN, FIRST, SMALL, EXC, TIRED, STALL = 0, 1, 2, 3, 4, 5
    status = t.where(first_order, FIRST, t.where(small_residual, SMALL, UNKNOWN)).to(t.int32)
    eta = t.full((B,), 1.0 if p else 0.0, **f64)
    epsk = t.full((B,), 1e3, **f64)
    rho_old = Z(B)
    it = t.zeros(B, dtype=t.int32, device=dev)
    inner = t.zeros(B, dtype=t.int64, device=dev)
    nfact = t.zeros(B, dtype=t.int64, device=dev)
    nlin = t.zeros(B, dtype=t.int64, device=dev)
    nbk = t.zeros(B, dtype=t.int64, device=dev)
    phase0 = t.ones(B, dtype=t.bool, device=dev)
    combined, combined_hat = Z(B), Z(B)
    ndh, nph = normdual.clone(), normprimal.clone()
    d = Z(B, N)
    xt, rt, lamt, Ft, ct = x.clone(), r.clone(), lam.clone(), Fx.clone(), cx.clone()
    d_new, rho_new = Z(B, N), Z(B)
    nf_new = t.zeros(B, dtype=t.int32, device=dev)
    ok_new = t.zeros(B, dtype=t.int32, device=dev)
    xt_e, rt_e, lamt_e, dlam_e = Z(B, n), Z(B, m), Z(B, P), Z(B, P)
    phi = lambda F_, c_, l_, et: 0.5 * rdot(F_, F_) - (rdot(l_, c_) if p else 0.0) + (et * rdot(c_, c_) / 2 if p else 0.0)
    steps = 0
    # host synchronisations per global step: one for the branch flags below, one for (rejected, small-residual) further down,
    # and one per round of backtracking when a line search runs
    while steps < max_steps:
        act = status == UNKNOWN
        if not bool(act.any()):
            break
        steps += 1
        # ---- start of an outer iteration, src/CaNNOLeS.jl:612-626
        so = act & phase0
        combined = W(so, normdual + normprimal, combined)
        delta = W(so, t.clamp(t.minimum(delta_dec * delta, combined), min=dmin), delta)
        inner = t.where(so, 0, inner)
        combined_hat = W(so, t.full_like(combined, float("inf")), combined_hat)
        ndh, nph = W(so, normdual, ndh), W(so, normprimal, nph)
        phase0 = phase0 & ~so
        # ---- Newton step (skipped on the iteration right after a rejected extrapolation), :627-652
        need = act & (inner != 1)
        brk = t.zeros(B, dtype=t.bool, device=dev)
        any_need, any_ext, any_ls = t.stack([need.any(), (act & (inner == 0)).any(), (act & (inner > 0)).any()]).tolist()
        if any_need:
            prepare(vals_cur, fam.hess_vals(x, r), Jv, Jcv, delta)
            ro_tmp = rho_old.clone()
            hipldl.newton_system_dev(L, ptr(vals_cur), ptr(rhs_cur), ptr(d_new), ptr(ro_tmp), ptr(rho_new), ptr(nf_new), ptr(ok_new), params, st)
            d = W(need, d_new, d)
            rho_old = W(need, ro_tmp, rho_old)
            nfact = nfact + t.where(need, nf_new.to(t.int64), 0)
            nlin = nlin + need.to(t.int64)
            # `broken`: the inner loop is left at once; the end-of-iteration tests below still run for it (:638-652)
            brk = need & ((rho_new > rhomax) | (ok_new == 0) | ~t.isfinite(d_new).all(dim=1) | (fx >= huge))
            act = act & ~brk
        dx = d[:, :n]
        ext, lsm = act & (inner == 0), act & (inner > 0)
        # ---- extrapolation step, :654-668
        if any_ext:   # (a superset test: problems that broke above are masked out by `ext`)
            epsk = W(ext, t.maximum(t.minimum(1e3 * delta, fdiv(99 * epsk, 100)), fdiv(9 * epsk, 10)), epsk)
            hipldl.trial_point_dev(L, ptr(x), ptr(r), ptr(lam) if p else 0, ptr(d), 1e4, ptr(xt_e), ptr(rt_e), ptr(lamt_e) if p else 0,
                                   ptr(dlam_e) if p else 0, st)
            xt, rt, lamt = W(ext, xt_e, xt), W(ext, rt_e, rt), W(ext, lamt_e, lamt)
        # ---- Armijo line search on the merit function, :1054-1112
        if any_ls:
            lam_ls = lam - fdiv(cx, delta[:, None]) if p else lam
            prepare(vals_cur, None, Jv, Jcv, delta)
            g, _, _ = resid_vectors(vals_cur, Fx, lam_ls, Fx, cx)      # dual part: Jx'Fx - Jc'(lam - c/delta)
            Dphi = rdot(g[:, :n], dx)
            if p:
                eta = W(lsm, fdiv(1.0, delta), eta)
            phix = phi(Fx, cx, lam, eta)
            alpha = t.ones(B, **f64)
            xl = x + dx
            Fl, cl = fam.residual(xl), fam.cons(xl)
            bt = lsm & ~(phi(Fl, cl, lam, eta) <= phix + gammaA * alpha * Dphi)
            while bool(bt.any()):
                nbk = nbk + bt.to(t.int64)
                alpha = W(bt, alpha / 4, alpha)
                xl = W(bt, x + alpha[:, None] * dx, xl)
                F2, c2 = fam.residual(xl), fam.cons(xl)
                Fl, cl = W(bt, F2, Fl), W(bt, c2, cl)
                bt = bt & ~(phi(Fl, cl, lam, eta) <= phix + gammaA * alpha * Dphi) & (alpha >= eps ** 2)
            xt, rt = W(lsm, xl, xt), W(lsm, Fl, rt)
            lamt = W(lsm, lam_ls, lamt)
        Ft, ct = fam.residual(xt), fam.cons(xt)
        # ---- optimality measures at the trial point, :722-732
        Jt, Jct = fam.jac_vals(xt), fam.jacc_vals(xt)
        prepare(vals_t, None, Jt, Jct, delta)
        rhs_t, nd_t, np_t = resid_vectors(vals_t, rt, lamt, Ft, ct)
        ndh, nph = W(act, nd_t, ndh), W(act, np_t, nph)
        combined_hat = W(act, ndh + nph, combined_hat)
        good = combined_hat <= 0.99 * combined + epsk
        acc_state = act & ((inner > 0) | good)
        x, r, Fx, cx = W(acc_state, xt, x), W(acc_state, rt, r), W(acc_state, Ft, Fx), W(acc_state, ct, cx)
        Jv, Jcv = W(acc_state, Jt, Jv), W(acc_state, Jct, Jcv)
        fx = W(acc_state, 0.5 * rdot(Ft, Ft), fx)
        acc_lam = act & good
        lam = W(acc_lam, lamt, lam)
        rhs_cur = W(act, rhs_t, rhs_cur)
        rej = act & ~good
        delta_next = delta
        if p:
            dr_ = act & (inner > 0) & (ndh <= 0.99 * normdual + epsk / 2) & (nph > 0.99 * normprimal + epsk / 2)
            delta_next = W(dr_, t.clamp(fdiv(delta, 10), min=dmin), delta)
        inner = inner + act.to(t.int64)
        tired = inner > max_inner
        # ---- end of the inner loop -> end of the outer iteration, :765-800 (tests first: one synchronisation for both branches)
        done_in = (act & (good | tired)) | brk
        normdual, normprimal = W(done_in, ndh, normdual), W(done_in, nph, normprimal)
        first_order = t.maximum(normdual / dual_scaling(lam), normprimal) <= epstol
        small_residual = (2 * fsqrt(fx) <= epsF) & (cnorm2(cx) <= epsc)
        chk = done_in & small_residual & ~first_order
        any_rej, any_chk = t.stack([rej.any(), chk.any()]).tolist()
        if any_rej:   # dual at (x, r, lam) again; primal keeps the trial's value, as in the reference (:742-747)
            prepare(vals_cur, None, Jv, Jcv, delta)
            rhs_r, _, _ = resid_vectors(vals_cur, r, lam, Fx, cx)
            rhs_cur = t.cat([W(rej, rhs_r[:, :n], rhs_cur[:, :n]), rhs_cur[:, n:]], dim=1)
        delta = delta_next
        if any_chk:
            lam, rhs_cur, normdual, normprimal, r = small_res_check(chk, lam, rhs_cur, normdual, normprimal, r)
            first_order = t.maximum(normdual / dual_scaling(lam), normprimal) <= epstol
        it = it + done_in.to(t.int32)
        new_status = t.where(first_order, FIRST, t.where(small_residual, SMALL, t.where(brk, EXC, t.where(tired, STALL, UNKNOWN))))   # inner > max_inner: `stalled` (src/CaNNOLeS.jl:846)
        status = t.where(done_in, new_status.to(t.int32), status)
        phase0 = phase0 | done_in
    t.cuda.synchronize(dev)
    names = {UNKNOWN: "unknown", FIRST: "first_order", SMALL: "small_residual", EXC: "exception", TIRED: "max_eval", STALL: "stalled"}
    out = {"solution": x.cpu().numpy(), "multipliers": lam[:, :p].cpu().numpy(), "status": [names[int(v)] for v in status.cpu().numpy()],
           "iter": it.cpu().numpy(), "nfact": nfact.cpu().numpy(), "nlinsolve": nlin.cpu().numpy(), "nbk": nbk.cpu().numpy(),
           "objective": fx.cpu().numpy(), "dtype": str(dt), "r": r.cpu().numpy(), "normdual": normdual.cpu().numpy(),
           "normprimal": normprimal.cpu().numpy(), "epstol": epstol.cpu().numpy(), "steps": steps, "kernel": L.config["kernel"]}
    L.close()
    return out
