"""PlanSimF32 (plan_sim_f32.py) on a CONDENSED plan: the CPU model of a Float32 general handle with tuning float32_condense = 1
(test infrastructure).

The three float passes of csrc/kernels_aux.hip around the multifrontal kernel, restated in numpy float32:
  condense     slot s = the sum, in LIST ORDER, of its contributions c_ptr[s] .. c_ptr[s + 1): a plain one adds x(c_a), a product
               one subtracts (x(c_a) * x(c_b)) / x(c_d) — product, quotient and every partial sum rounded to float32, nothing
               accumulated in a wider type (x(i) = vals[i] below nnz, rhs[i - nnz] above);
  cond_inertia the condensed pivots d_r against eig_tol narrowed to float32;
  expand       kept components copied, d_r_out = -((rhs_r + sum_k J_rk d2_xk) / d_r) with the row's products rounded one by one and
               summed in row order onto rhs_r.
Between them PlanSimF32's factor and backward sweep run on the condensed system.  The kernels agree with this model up to the fused
multiply-add of expand's long-row loop and the backward sweep's reduction order, which the tolerances of the tests absorb; the
summation ORDER of a slot is the rule this file pins.
"""
import numpy as np

from tests.support.plan_sim import PlanSim
from tests.support.plan_sim_f32 import PlanSimF32

F32 = np.float32


class PlanSimF32Cond(PlanSimF32):
    def __init__(self, plan):
        PlanSim.__init__(self, plan)
        assert self.ncond, "the plan is not condensed (Options(condense=1) on a pattern with residual nodes)"
        self.nslot = len(self.c_ptr) - 1
        self.c_len = np.diff(self.c_ptr)

    def condense(self, vals, rhs):
        """[K2 slots | rho tail | condensed rhs] in float32, every slot summed in list order"""
        x = np.concatenate([np.asarray(vals, F32), np.asarray(rhs, F32)])
        assert x.dtype == F32
        plain = self.c_b < 0
        with np.errstate(all="ignore"):
            prod = x[self.c_a] * x[np.maximum(self.c_b, 0)]           # float32 product
            quot = prod / x[np.maximum(self.c_d, 0)]                   # float32 quotient (correctly rounded)
        assert prod.dtype == F32 and quot.dtype == F32
        out = np.zeros(self.nslot, F32)
        for k in range(int(self.c_len.max(initial=0))):                # the k-th contribution of every slot that has one
            on = np.nonzero(self.c_len > k)[0]
            c = self.c_ptr[on] + k
            out[on] = np.where(plain[c], out[on] + x[self.c_a[c]], out[on] - quot[c])
        assert out.dtype == F32
        return out

    def cond_inertia(self, vals, eig_tol):
        dr = np.asarray(vals, F32)[self.r_dsrc]
        tol = F32(eig_tol)
        return int((dr > tol).sum()), int((np.abs(dr) <= tol).sum())

    def expand(self, vals, rhs, d2):
        vals, rhs, d2 = np.asarray(vals, F32), np.asarray(rhs, F32), np.asarray(d2, F32)
        d = np.zeros(self.Nout, F32)
        d[self.orig_of] = d2
        for q in range(len(self.r_orig)):
            s_ = rhs[self.r_orig[q]]
            for k in range(self.r_ptr[q], self.r_ptr[q + 1]):
                s_ = F32(s_ + F32(vals[self.r_jsrc[k]] * d2[self.r_jx[k]]))
            d[self.r_orig[q]] = -F32(s_ / vals[self.r_dsrc[q]])
        return d

    def newton_system(self, vals, rhs, nvar, nequ, ncon, rho_old, params):
        """float32 in, float32 out: (d, ok, rho, rho_old, nfact).  `vals` (a float32 array) gets its rho slots rewritten where the
        ladder ran, as the reference mutates them (src/CaNNOLeS.jl:1031, 1038); d stays zero where the factorisation failed."""
        p = np.asarray(params, F32)
        vals32, rhs32 = np.asarray(vals, F32), np.asarray(rhs, F32)
        cb = self.condense(vals32, rhs32)
        nmat = self.nslot - self.N                                      # K2 slots and the rho tail
        xpos, xzer = self.cond_inertia(vals32, p[0])
        cv, crhs = cb[:nmat].copy(), cb[nmat:]
        eig_tol, kdec, kinc, klarge, rho0, rhomax, rhomin = p[0], p[2], p[3], p[4], p[5], p[6], p[7]

        def attempt(rho=None):
            L, npos, nzer = self.factor(cv, crhs, nvar, eig_tol, rho)
            return L, (npos + xpos == nvar and nzer + xzer == 0)

        ro = F32(rho_old)
        rho = wrote = F32(0)
        L, ok = attempt()
        nfact = 1
        if not ok:
            rho = rho0 if ro == 0 else max(rhomin, F32(kdec * ro))
            wrote = rho
            L, ok = attempt(rho)
            nfact += 1
            while not ok and rho <= rhomax:
                rho = F32(klarge * rho) if ro == 0 else F32(kinc * rho)
                if rho <= rhomax:
                    wrote = rho
                    L, ok = attempt(rho)
                    nfact += 1
            if rho <= rhomax:
                ro = rho
            if isinstance(vals, np.ndarray) and vals.dtype == F32:
                vals[len(vals) - nvar:] = wrote
        d = self.expand(vals32, rhs32, self.backward(L)) if ok else np.zeros(self.Nout, F32)
        return d, bool(ok), F32(rho), F32(ro), nfact
