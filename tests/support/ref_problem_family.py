"""The reference's own constrained test problems with NONLINEAR constraints as families for the lockstep loop (test infrastructure):
(F_linear, c_quad), (F_Rosen, c_quad), (F_larger(3), c_quad) of tests/test_oracle_pinning.CONSTRAINED and HS6.  Every callback is a torch
closed form on [B, n] arrays, written out by hand on the dense structures tests/support/outer_loop.SymNLS uses (Hessians: lower triangle,
column-major; Jacobians: every entry, row-major); `host_model(b)` is the SymNLS model of problem b, whose sympy derivatives
tests/test_loop_nonlinear_cpu.py holds these closed forms against.  A batch is one problem from B start points: row 0 the reference's,
the others small seeded perturbations of it."""
import numpy as np

from tests import test_oracle_pinning as P
from tests.support.outer_loop import SymNLS


def _dense_structure(n, m, p, name):
    from cannoles_jl_amd import synthetic as syn
    il, jl = np.tril_indices(n)
    o = np.lexsort((il, jl))
    h = (il[o] + 1, jl[o] + 1)
    jr, jc = np.nonzero(np.ones((m, n)))
    cr, cc = np.nonzero(np.ones((p, n)))
    return syn.Structure(n, m, p, h, h, (jr + 1, jc + 1), (cr + 1, cc + 1), name=name)


def _cols(t, *cols):
    return t.stack(cols, dim=1)


# ---- residuals: (F, J_F values, sum_i r_i Hess F_i values) -----------------------------------------------------------------------------------
def _F_linear(t):
    def F(X):
        return _cols(t, X[:, 0] - 2, X[:, 1] - 3)

    def J(X):
        one, zero = t.ones_like(X[:, 0]), t.zeros_like(X[:, 0])
        return _cols(t, one, zero, zero, one)

    def H(X, R):
        return t.zeros((X.shape[0], 3), dtype=X.dtype, device=X.device)

    return F, J, H, 2


def _F_rosen(t):
    def F(X):
        return _cols(t, X[:, 0] - 1, 10 * (X[:, 1] - X[:, 0] ** 2))

    def J(X):
        one, zero = t.ones_like(X[:, 0]), t.zeros_like(X[:, 0])
        return _cols(t, one, zero, -20 * X[:, 0], 10 * one)

    def H(X, R):
        zero = t.zeros_like(X[:, 0])
        return _cols(t, -20 * R[:, 1], zero, zero)

    return F, J, H, 2


def _F_larger3(t):
    def F(X):
        return _cols(t, 10 * (X[:, 1] - X[:, 0] ** 2), 10 * (X[:, 2] - X[:, 1] ** 2), X[:, 0] - 1, X[:, 1] - 1)

    def J(X):
        one, zero = t.ones_like(X[:, 0]), t.zeros_like(X[:, 0])
        return _cols(t, -20 * X[:, 0], 10 * one, zero, zero, -20 * X[:, 1], 10 * one, one, zero, zero, zero, one, zero)

    def H(X, R):   # (1,1) (2,1) (3,1) (2,2) (3,2) (3,3)
        zero = t.zeros_like(X[:, 0])
        return _cols(t, -20 * R[:, 0], zero, zero, -20 * R[:, 1], zero, zero)

    return F, J, H, 4


def _F_hs6(t):
    def F(X):
        return _cols(t, X[:, 0] - 1)

    def J(X):
        return _cols(t, t.ones_like(X[:, 0]), t.zeros_like(X[:, 0]))

    def H(X, R):
        return t.zeros((X.shape[0], 3), dtype=X.dtype, device=X.device)

    return F, J, H, 1


# ---- constraints: (c, J_c values, sum_k lam_k Hess c_k values) -------------------------------------------------------------------------------
def _c_quad2(t):
    def c(X):
        return _cols(t, X[:, 0] ** 2 + X[:, 1] ** 2 - 5, X[:, 0] * X[:, 1] - 2)

    def J(X):
        return _cols(t, 2 * X[:, 0], 2 * X[:, 1], X[:, 1], X[:, 0])

    def H(X, LAM):
        return _cols(t, 2 * LAM[:, 0], LAM[:, 1], 2 * LAM[:, 0])

    return c, J, H, 2


def _c_quad3(t):
    def c(X):
        return _cols(t, X[:, 0] ** 2 + X[:, 1] ** 2 + X[:, 2] ** 2 - 5, X[:, 0] * X[:, 1] * X[:, 2] - 2)

    def J(X):
        return _cols(t, 2 * X[:, 0], 2 * X[:, 1], 2 * X[:, 2], X[:, 1] * X[:, 2], X[:, 0] * X[:, 2], X[:, 0] * X[:, 1])

    def H(X, LAM):
        l0, l1 = 2 * LAM[:, 0], LAM[:, 1]
        return _cols(t, l0, l1 * X[:, 2], l1 * X[:, 1], l0, l1 * X[:, 0], l0)

    return c, J, H, 2


def _c_hs6(t):
    def c(X):
        return _cols(t, 10 * (X[:, 1] - X[:, 0] ** 2))

    def J(X):
        return _cols(t, -20 * X[:, 0], 10 * t.ones_like(X[:, 0]))

    def H(X, LAM):
        zero = t.zeros_like(X[:, 0])
        return _cols(t, -20 * LAM[:, 0], zero, zero)

    return c, J, H, 1


_hs6_F = lambda x: [x[0] - 1]                      # noqa: E731   (tests/test_oracle_pinning.test_hs6_resolve_and_small_residual)
_hs6_c = lambda x: [10 * (x[1] - x[0] ** 2)]       # noqa: E731

# name -> (torch residual, torch constraints, the sympy-side functions, the reference's start point, its answer, the atol of its test)
PROBLEMS = {
    "linear-quad": (_F_linear, _c_quad2, P.F_linear, P.c_quad) + tuple(P.CONSTRAINED[3][2:]),
    "rosen-quad": (_F_rosen, _c_quad2, P.F_Rosen, P.c_quad) + tuple(P.CONSTRAINED[4][2:]),
    "larger3-quad": (_F_larger3, _c_quad3, P.F_larger(3), P.c_quad) + tuple(P.CONSTRAINED[5][2:]),
    "hs6": (_F_hs6, _c_hs6, _hs6_F, _hs6_c, [-1.2, 1.0], [1.0, 1.0]),
    "hs6-far": (_F_hs6, _c_hs6, _hs6_F, _hs6_c, [10.0, 10.0], [1.0, 1.0]),
}
assert P.CONSTRAINED[3][:2] == (P.F_linear, P.c_quad) and P.CONSTRAINED[4][:2] == (P.F_Rosen, P.c_quad) and P.CONSTRAINED[5][1] is P.c_quad
REF_ATOL = 1e-4       # test/runtests.jl of the reference: the known answers are held at atol = 1e-4
PERTURBATION = 0.02   # rows 1 .. B - 1 start within this of the reference's start point


class RefProblemFamily:
    """One of PROBLEMS from B start points, with the members solve_batch_device reads of a family"""
    linear_constraints = False
    dtype = np.dtype(np.float64)

    def __init__(self, name, B, seed, torch, device):
        mkF, mkc, self._symF, self._symc, x0, self.answer = PROBLEMS[name]
        self.name, self.B, self.torch, self.device = name, int(B), torch, device
        self.residual, self.jac_vals, self.hess_vals, m = mkF(torch)
        self.cons, self.jacc_vals, self.hess_cons_vals, p = mkc(torch)
        self.s = _dense_structure(len(x0), m, p, name)
        rng = np.random.default_rng(seed)
        X0 = np.tile(np.asarray(x0, float), (self.B, 1))
        X0[1:] += PERTURBATION * rng.uniform(-1, 1, (self.B - 1, len(x0)))
        self.h = {"x0": X0}
        self.d = {"x0": torch.as_tensor(X0, dtype=torch.float64, device=device)}

    def per_problem_tensors(self):
        return dict(self.d)

    def head(self, nb):
        sub = object.__new__(type(self))
        sub.__dict__.update(self.__dict__)
        sub.B = int(nb)
        sub.h = {k: v[:nb] for k, v in self.h.items()}
        sub.d = {k: v[:nb] for k, v in self.d.items()}
        return sub

    def host_model(self, b):
        return SymNLS(self._symF, self.h["x0"][b], self._symc)
