"""A plain restatement of the `_ex` entry points of csrc/outer_step.hip (cnl_outer_begin_ex_dev, cnl_outer_trial_done_ex_dev,
cnl_outer_ls_test_ex_dev, cnl_outer_end_ex_dev) and of cnl_outer_hess_mask_dev, one problem at a time, written from the contract of
`cnl_outer_ctl` in include/cannoles_hip.h and from cannoles.jl_amd/outer_loop.py.  The state `S` is that of tests/support/outer_step_sim.py
(whose helpers and conventions are used: arithmetic in T, reductions summed exactly and rounded once); the control block is a dict

    ctl = dict(always_accept_extrapolation, max_iter, max_eval, evals_per_point, neval [rows] int64, hess_upd [rows] uint8 or None)

and ctl = None stands for the plain call.  Every function works in place on the first S["B"] rows."""
import numpy as np

from tests.support import outer_step_sim as base
from tests.support.outer_step_sim import dual_scaling, merit, rdot, rsum, tmax, tmin


def new_ctl(rows, evals_per_point, always_accept_extrapolation=0, max_iter=-1, max_eval=-1, with_mask=True):
    return dict(always_accept_extrapolation=int(always_accept_extrapolation), max_iter=int(max_iter), max_eval=int(max_eval),
                evals_per_point=int(evals_per_point), neval=np.zeros(rows, np.int64), hess_upd=np.zeros(rows, np.uint8) if with_mask else None)


def copy_ctl(ctl):
    return None if ctl is None else {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ctl.items()}


def _always(ctl):
    return bool(ctl and ctl["always_accept_extrapolation"])


def _over_eval(ctl, b):
    return bool(ctl and ctl["max_eval"] >= 0 and ctl["neval"][b] > ctl["max_eval"])


def begin_ex(S, ctl):
    """:612-627: as begin, with need = act and (inner != 1 or always_accept_extrapolation)"""
    T = S["T"]
    S["flags"][:] = 0
    with np.errstate(all="ignore"):
        for b in range(S["B"]):
            act = S["status"][b] == 0
            inner = int(S["inner"][b])
            if act and S["phase0"][b]:
                nd, npr = S["normdual"][b], S["normprimal"][b]
                comb = nd + npr
                S["combined"][b] = comb
                S["delta"][b] = tmax(tmin(S["delta_dec"] * S["delta"][b], comb), S["dmin"])
                inner = 0
                S["inner"][b] = 0
                S["combined_hat"][b] = T(np.inf)
                S["ndh"][b], S["nph"][b] = nd, npr
                S["phase0"][b] = 0
            need = act and (inner != 1 or _always(ctl))
            S["act"][b], S["need"][b], S["brk"][b] = act, need, 0
            if act:
                S["flags"][0] = 1
            if need:
                S["flags"][1] = 1
            if act and inner == 0:
                S["flags"][2] = 1
            if act and inner > 0:
                S["flags"][3] = 1


def trial_done_ex(S, ctl):
    """:722-800: as trial_done; the state is accepted also where always_accept_extrapolation (:735); the problems of `ext` count the
    evaluation of their trial point; tired = inner > max_inner or neval > max_eval >= 0"""
    T, n, m, p, P, N = S["T"], S["n"], S["m"], S["p"], S["P"], S["N"]
    with np.errstate(all="ignore"):
        for b in range(S["B"]):
            act, brk = S["act"][b] != 0, S["brk"][b] != 0
            inner0 = int(S["inner"][b])
            ss = rdot(T, S["Ft"][b, :m], S["Ft"][b, :m])
            ndh, nph, chat = S["ndh"][b], S["nph"][b], S["combined_hat"][b]
            if act:
                ndh, nph = S["nrm_t"][b, 0], S["nrm_t"][b, 1]
                chat = ndh + nph
            S["ndh"][b], S["nph"][b], S["combined_hat"][b] = ndh, nph, chat
            epsk = S["epsk"][b]
            good = bool(chat <= T(0.99) * S["combined"][b] + epsk)
            acc_state = act and (inner0 > 0 or _always(ctl) or good)
            acc_lam = act and good
            if ctl is not None and S["ext"][b]:
                ctl["neval"][b] += ctl["evals_per_point"]
            if acc_state:
                S["fx"][b] = T(0.5) * ss
            delta = S["delta"][b]
            delta_next = delta
            if p > 0:
                dr = act and inner0 > 0 and bool(ndh <= T(0.99) * S["normdual"][b] + epsk / T(2)) \
                    and bool(nph > T(0.99) * S["normprimal"][b] + epsk / T(2))
                if dr:
                    delta_next = tmax(delta / T(10), S["dmin"])
            inner = inner0 + (1 if act else 0)
            S["inner"][b] = inner
            tired = inner > S["max_inner"] or _over_eval(ctl, b)
            done_in = (act and (good or tired)) or brk
            if done_in:
                S["normdual"][b], S["normprimal"][b] = ndh, nph
            S["delta"][b] = delta_next
            rej = act and not good
            S["rej"][b], S["done_in"][b], S["tired"][b] = rej, done_in, tired
            if rej:
                S["flags"][4] = 1
            if acc_state:
                S["x"][b, :n] = S["xt"][b, :n]
                S["r"][b, :m] = S["rt"][b, :m]
                S["Fx"][b, :m] = S["Ft"][b, :m]
                S["cx"][b, :P] = S["ct"][b, :P]
                S["Jv"][b, :S["nnzjF"]] = S["Jt"][b, :S["nnzjF"]]
                if S["nnzjc"] > 0 and S["Jcv"] is not S["Jct"]:
                    S["Jcv"][b, :S["nnzjc"]] = S["Jct"][b, :S["nnzjc"]]
            if acc_lam:
                S["lam"][b, :P] = S["lamt"][b, :P]
            if act:
                S["rhs_cur"][b, :N] = S["rhs_t"][b, :N]
            sc = rsum(T, [float(v) * float(v) for v in S["cx"][b, :p]])
            first_order = bool(tmax(S["normdual"][b] / dual_scaling(S, b), S["normprimal"][b]) <= S["epstol"][b])
            small_res = bool(T(2) * np.sqrt(S["fx"][b]) <= S["epsF"][b]) and bool(np.sqrt(sc) <= S["epsc"][b])
            S["small_res"][b] = small_res
            chk = done_in and small_res and not first_order
            S["chk"][b] = chk
            if chk:
                S["flags"][5] = 1


def ls_test_ex(S, first, ctl):
    """as ls_test; every candidate of the call (lsm when first, else bt) counts the evaluation of its xl"""
    S["flags"][6] = 0
    with np.errstate(all="ignore"):
        for b in range(S["B"]):
            cand = S["lsm"][b] != 0 if first else S["bt"][b] != 0
            if not cand:
                if first:
                    S["bt"][b] = 0
                continue
            if ctl is not None:
                ctl["neval"][b] += ctl["evals_per_point"]
            phil = merit(S, b, S["Fl"], S["cl"], S["eta"][b])
            alpha = S["alpha"][b]
            bt = not bool(phil <= S["phix"][b] + S["gammaA"] * alpha * S["Dphi"][b])
            if not first:
                bt = bt and bool(alpha >= S["eps2"])
            S["bt"][b] = bt
            if bt:
                S["flags"][6] = 1


def end_ex(S, ctl):
    """:800-857 where done_in, the status chain of outer_loop.solve: first_order 1, small_residual 2, exception 3, max_eval 4 (neval >
    max_eval >= 0), max_iter 6 (it > max_iter >= 0, it already incremented), stalled 5 (`tired`), else 0"""
    with np.errstate(all="ignore"):
        for b in range(S["B"]):
            if not S["done_in"][b]:
                continue
            first_order = bool(tmax(S["normdual"][b] / dual_scaling(S, b), S["normprimal"][b]) <= S["epstol"][b])
            S["it"][b] += 1
            over_iter = bool(ctl and ctl["max_iter"] >= 0 and S["it"][b] > ctl["max_iter"])
            S["status"][b] = (1 if first_order else 2 if S["small_res"][b] else 3 if S["brk"][b] else 4 if _over_eval(ctl, b) else 6 if over_iter
                              else 5 if S["tired"][b] else 0)
            S["phase0"][b] = 1


def hess_mask(S, ctl):
    """hessian_approx.jl:55-60: hess_upd = dot(Fx, Fx) > 1e-8 — the dot product summed exactly, rounded to T once, compared with the double"""
    m = S["m"]
    for b in range(S["B"]):
        ctl["hess_upd"][b] = float(rdot(S["T"], S["Fx"][b, :m], S["Fx"][b, :m])) > 1e-8


PLAIN = dict(begin_ex=base.begin, trial_done_ex=base.trial_done, ls_test_ex=base.ls_test, end_ex=base.end)
