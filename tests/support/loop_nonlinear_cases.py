"""What the CPU and the GPU tests of the lockstep loop with nonlinear constraints share (test infrastructure): the family's parameters,
chosen on the CPU (tests/test_loop_nonlinear_cpu.py asserts what they are chosen for), the scalar runs of outer_loop.solve with the CPU
oracle on the counting wrapper, computed once per case, and the two crippled models that show what the comparison can see."""
import numpy as np

from tests.support.counting_model import CountingModel

# BandQuadConFamily(band_structure(40, 2), 12, SEED, **KIND): the F3 kind of tests/test_loop_keywords_gpu.py and constraint curvatures
# of +-0.5.  Problems 0 and 9 reject an extrapolation and backtrack in the line search behind it, and every problem climbs the rho
# ladder.
# F32_SEED, for the Float32 run: the host mirror computes in Float64, so its decisions bind a Float32 run only where they do not hang on
# the last bits.  The seed is the first from 40 on at which, on the data rounded to Float32 and under the Float32 run's tolerances
# (f32_run), three problems reject an extrapolation and backtrack, every problem climbs the ladder, AND every problem's status and
# counters stay what they are under each of the perturbations of F32_PERTURBATIONS, which are of the size of a Float32 run's own
# rounding: every model callback takes and returns Float32 values (Float32Callbacks), and every Newton system is solved for values
# and a right-hand side changed by eps32 relative — rounded to Float32, or multiplied by 1 + 2 eps32 u, u uniform in [-1, 1], four
# draws — with the step rounded to Float32: a backward-stable Float32 factorisation is the exact solve of such a system, so this
# carries the conditioning of the system into the step, which rounding the callbacks alone does not.  Asserted on the CPU
# (float32_stable).  Seeds 48, 53 and 59 have the three problems and fail it (48: problem 5; 53: problems 4 and 7); a Float32 run on
# the device leaves the mirror's counters on exactly those problems of seeds 48 and 53.
N, P, BL, SEED, F32_SEED = 40, 2, 12, 53, 84
KIND = dict(curvature=1.5, start=1.0, noise=0.5, con_curvature=0.5)
DECISIONS = ("iter", "nlinsolve", "nfact", "nbk", "neval")
# the larger shape that needs the wide CGLS instance: 1 025 constraints, the smallest number above the LDS instance's 1 024
# (band_structure needs n % p == 0)
WIDE_N, WIDE_P, WIDE_B, WIDE_SEED = 2050, 1025, 2, 7
WIDE_KIND = dict(curvature=0.1, start=0.1, con_curvature=0.1)
WIDE_MAX_ITER = 1     # on both sides: the host mirror's factorisations of order 5 125 take a second each (two iterations: about 4 s)
# the other methods run a milder residual (Gauss-Newton does not end on the F3 kind within max_eval): two problems reject an
# extrapolation and backtrack under either method, and with noise = 0 four problems skip a refresh of H_F under Newton_vanishing
# (family keywords, `seed` among them: chosen per method)
METHOD_KINDS = {"Newton": KIND, "Newton_noFHess": dict(curvature=0.3, start=1.0, noise=0.01, con_curvature=0.5, seed=44),
                "Newton_vanishing": dict(curvature=0.3, start=1.0, noise=0.0, con_curvature=0.5, seed=44)}
# 300 variables, 4 constraints, 12 problems: the default handle of this batch runs staged and refuses cnl_set_active_batch
STAGED_N, STAGED_P, STAGED_SEED = 300, 4, 304
_runs = {}


def family(device="cpu", dtype=np.float64, seed=SEED, **over):
    import torch
    from cannoles_jl_amd import device_loop as DL, synthetic as syn
    return DL.BandQuadConFamily(syn.band_structure(N, P), BL, seed, torch=torch, device=device, dtype=dtype, **dict(KIND, **over))


def staged_family(device="cpu"):
    import torch
    from cannoles_jl_amd import device_loop as DL, synthetic as syn
    return DL.BandQuadConFamily(syn.band_structure(STAGED_N, STAGED_P), BL, STAGED_SEED, torch=torch, device=device, **KIND)


def f32_run(hipldl):
    """keywords under which outer_loop.solve (Float64 arithmetic) takes a Float32 run's tolerances and ParamCaNNOLeS(Float32)"""
    eps32 = float(np.finfo(np.float32).eps)
    return dict(params=hipldl.default_params(np.float32).astype(np.float64), atol=np.sqrt(eps32), rtol=np.sqrt(eps32), Fatol=np.sqrt(eps32),
                Frtol=eps32)


def wide_family(device="cpu"):
    import torch
    from cannoles_jl_amd import device_loop as DL, synthetic as syn
    return DL.BandQuadConFamily(syn.band_structure(WIDE_N, WIDE_P), WIDE_B, WIDE_SEED, torch=torch, device=device, **WIDE_KIND)


class NoConstraintHessian:
    """the model with hess_coord_cons forced to zero: what a loop that hands `prepare` a zero H_c solves"""

    def __init__(self, model):
        self._model = model

    def __getattr__(self, name):
        return getattr(self._model, name)

    def hess_coord_cons(self, x, lam):
        return np.zeros(len(self._model.h_rows))


class StaleConstraintJacobian:
    """the model whose constraint Jacobian is never evaluated again: jac(xt) is jac(x), so by induction the start point's — what a loop
    with one constraint-Jacobian array, evaluated once, computes with"""

    def __init__(self, model):
        self._model = model
        self._J = None

    def __getattr__(self, name):
        return getattr(self._model, name)

    def jac(self, x):
        if self._J is None:
            self._J = self._model.jac(x)
        return self._J


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


class Float32Callbacks:
    """the model with every callback's arguments and results rounded to Float32: a perturbation of the size of a Float32 run's rounding"""

    def __init__(self, model):
        self._model = model

    def __getattr__(self, name):
        return getattr(self._model, name)

    def residual(self, x):
        return _f32(self._model.residual(_f32(x)))

    def cons(self, x):
        return _f32(self._model.cons(_f32(x)))

    def jac_residual(self, x):
        return _f32(self._model.jac_residual(_f32(x)))

    def jac(self, x):
        return _f32(self._model.jac(_f32(x)))

    def hess_coord_residual(self, x, r):
        return _f32(self._model.hess_coord_residual(_f32(x), _f32(r)))

    def hess_coord_cons(self, x, lam):
        return _f32(self._model.hess_coord_cons(_f32(x), _f32(lam)))


F32_PERTURBATIONS = ("round", 1, 2, 3, 4)     # the systems rounded to Float32; four seeded draws of the random perturbation


def float32_newton(which):
    """the oracle's newton_system on a system perturbed by eps32 relative (see F32_SEED), its step rounded to Float32"""
    from tests.test_oracle_pinning import oracle_newton
    eps32 = float(np.finfo(np.float32).eps)
    rng = None if which == "round" else np.random.default_rng(which)

    def newton(LDLT, nvar, nequ, ncon, rhs, vals, rho_old, params):
        if rng is None:
            rhs2, vals2 = _f32(rhs), _f32(vals)
        else:
            rhs2 = rhs * (1 + 2 * eps32 * rng.uniform(-1, 1, rhs.shape))
            vals2 = vals * (1 + 2 * eps32 * rng.uniform(-1, 1, vals.shape))
        d, ok, rho, rho_old, nf = oracle_newton(LDLT, nvar, nequ, ncon, rhs2, vals2, rho_old, params)
        return _f32(d), ok, rho, rho_old, nf

    return newton


def float32_stable(fam, key, ones, **kw):
    """the problems whose status or counters change under one of F32_PERTURBATIONS (empty: what F32_SEED is chosen for)"""
    moved = set()
    for which in F32_PERTURBATIONS:
        pert = scalar_runs(fam, (key, "perturbed", which), wrap=Float32Callbacks, newton=float32_newton(which), max_iter=100, **kw)
        moved |= {b for b in range(len(ones)) if any(ones[b][k] != pert[b][k] for k in ("status",) + DECISIONS)}
    return sorted(moved)


def scalar_run(model, params=None, newton=None, **kw):
    """outer_loop.solve with the CPU oracle on a counting wrapper of `model`; adds `neval` and `rejected`, the number of rejected
    extrapolations: every trial point but a rejected extrapolation's successor (inner = 1) has a Newton system in front, so
    rejected = trial points - nlinsolve, trial points = evaluated points - the start point - the backtracking candidates"""
    from cannoles_jl_amd import outer_loop
    from oracle import oracle as O
    from tests.test_oracle_pinning import oracle_newton, oracle_solver
    cm = CountingModel(model)
    epp = 2 if model.ncon else 1
    one = outer_loop.solve(cm, oracle_solver, newton or oracle_newton, O.default_params() if params is None else params, **kw)
    one["neval"] = cm.neval
    one["rejected"] = cm.neval // epp - 1 - one["nbk"] - one["nlinsolve"]
    return one


def scalar_runs(fam, key, wrap=None, nb=None, **kw):
    if key not in _runs:
        _runs[key] = [scalar_run(wrap(fam.host_model(b)) if wrap else fam.host_model(b), **kw) for b in range(fam.B if nb is None else nb)]
    return _runs[key]


def col(ones, k):
    return [o[k] for o in ones]


def assert_chosen_for(ones):
    """what SEED and KIND are chosen for, asserted on the scalar runs (the GPU tests call this before they touch the device)"""
    assert set(col(ones, "status")) <= {"first_order", "small_residual"}, col(ones, "status")
    assert any(o["rejected"] > 0 for o in ones), "no problem rejects an extrapolation"
    assert any(o["nbk"] > 0 for o in ones), "no line search backtracks"
    assert any(o["nfact"] > o["nlinsolve"] for o in ones), "no problem climbs the rho ladder"
