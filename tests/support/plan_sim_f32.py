"""PlanSim (plan_sim.py) with every store rounded to float32 (test infrastructure).

The same schedule, on float32 arrays: work area, factor panels, x stack and d are float32, every product, quotient and sum is a
float32 operation, and the ladder runs on float32 scalars.  It is the CPU model of the general multifrontal kernel's Float32
instantiation (csrc/kernels.hip with T = float) up to the fused multiply-adds and the reduction order of the backward dot
products, which the tolerances of the tests absorb.  Plans without condensation only (the plan of a Float32 general handle).
"""
import numpy as np

from tests.support.plan_sim import PlanSim, tri

F32 = np.float32


class PlanSimF32(PlanSim):
    def __init__(self, plan):
        super().__init__(plan)
        assert not self.ncond, "the Float32 general kernel runs plans without condensation"

    def factor(self, vals, rhs, nvar, eig_tol, rho=None):
        f = self.fr
        eig_tol = F32(eig_tol)
        W = np.full(self.info["fwd_peak"] + 8, np.nan, F32)
        L = np.full(self.info["lsize"], np.nan, F32)
        src_all = np.concatenate([np.asarray(vals, F32), np.zeros(self.N, F32) if rhs is None else np.asarray(rhs, F32)])
        if rho is not None:
            src_all[self.nnz - nvar:self.nnz] = F32(rho)
        npos = nzer = 0
        for s in range(self.ns):
            nupd, npiv = f["nupd"][s], f["npiv"][s]
            fs = 1 + nupd + npiv
            tf, tu = tri(fs), tri(1 + nupd)
            F = W[f["foff"][s]:f["foff"][s] + tf]
            F[:] = 0.0
            for r in range(f["seg_begin"][s], f["seg_end"][s]):
                e0, e1 = self.seg_ptr[r], self.seg_ptr[r + 1]
                F[self.asm_pos[e0:e1]] += src_all[self.asm_src[e0:e1]]
            for c in self.child_idx[f["child_begin"][s]:f["child_end"][s]]:
                nu = f["nupd"][c]
                tuc = tri(1 + nu)
                U = W[f["ubase"][c]:f["ubase"][c] + tuc]
                rel = self.rel_idx[f["rel_begin"][c]:f["rel_begin"][c] + 1 + nu]
                F[tri(rel[self.ti[:tuc]]) + rel[self.tj[:tuc]]] += U
            idep = fs - f["indep"][s]
            for i in range(fs - 1, nupd, -1):
                ulim = idep if i >= idep else i
                row = F[tri(i):tri(i) + i + 1]
                dp = row[i]
                npos += dp > eig_tol
                nzer += abs(dp) <= eig_tol
                w = row[:ulim].copy()
                with np.errstate(all="ignore"):
                    l = w / dp
                row[:ulim] = l
                tul = tri(ulim)
                with np.errstate(all="ignore"):
                    F[:tul] -= l[self.ti[:tul]] * w[self.tj[:tul]]
            assert F.dtype == F32
            L[self.lptr[s]:self.lptr[s] + tf - tu] = F[tu:tf]
            if f["ubase"][s] != f["foff"][s]:
                W[f["ubase"][s]:f["ubase"][s] + tu] = F[:tu].copy()
        return L, int(npos), int(nzer)

    def backward(self, L):
        f = self.fr
        assert L.dtype == F32
        X = np.full(self.info["bwd_peak"] + 8, np.nan, F32)
        d = np.zeros(self.N, F32)
        for s in range(self.ns - 1, -1, -1):
            nupd, npiv = f["nupd"][s], f["npiv"][s]
            fs = 1 + nupd + npiv
            tu = tri(1 + nupd)
            panel = L[self.lptr[s]:self.lptr[s] + tri(fs) - tu]
            xo = f["xoff"][s]
            if f["parent"][s] >= 0:
                rel = self.rel_idx[f["rel_begin"][s]:f["rel_begin"][s] + 1 + nupd]
                xp = f["xoff"][f["parent"][s]]
                X[xo + 1:xo + 1 + nupd] = X[xp + rel[1:]].copy()
            for i in range(nupd + 1, fs):
                row = panel[tri(i) - tu:tri(i) - tu + i + 1]
                acc = F32(0)
                for j in range(1, i):   # float32 products and sums, one after the other
                    acc = F32(acc + F32(row[j] * X[xo + j]))
                xi = F32(row[0] - acc)
                X[xo + i] = xi
                d[self.perm[f["first_piv"][s] + (fs - 1 - i)]] = -xi
        return d

    def newton_system(self, vals, rhs, nvar, nequ, ncon, rho_old, params):
        """float32 in, float32 out: (d, ok, rho, rho_old, nfact) with rho / rho_old as float32 scalars"""
        p32 = np.asarray(params, F32)
        d, ok, rho, ro, nf = self._newton_inner(np.asarray(vals, F32), np.asarray(rhs, F32), nvar, F32(rho_old), p32, 0, 0)
        return d, ok, F32(rho), F32(ro), nf
