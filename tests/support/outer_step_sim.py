"""A plain restatement of the nine step kernels of csrc/outer_step.hip (cnl_outer_begin_dev ... cnl_outer_end_dev and their `_f32_dev`
twins), one problem at a time, for the tests to compare the kernels with.

Written from the contract in include/cannoles_hip.h and the project's scalar loop cannoles.jl_amd/outer_loop.py (the reference's lines
are cited as there: src/CaNNOLeS.jl).  A state `S` is a dict: the scalar members of `cnl_outer_state` (B, n, m, p, P, N, nnzjF, nnzjc,
max_inner as int; dmin, rhomax, delta_dec, smax, gammaA, eps2 as scalars of the element type), "T" (np.float64 or np.float32) and one
numpy array per array member — [rows] for a per-problem scalar, [rows, width] for a row array, [8] for flags; rows >= B.  Jcv / Jct
may be None (nnzjc == 0) or the same array; lam_ls may be None for the entries that do not need it.  Every function works in place on
the first B rows and touches nothing else.

Element type: every operation is on numpy scalars of T, so each is rounded separately in T; every literal is rounded to T first.
Reductions (|Ft|^2, the three merit sums, g'dx, the non-finite count, sum |lam|, sum c^2): every term widened to a Python float, summed
with math.fsum, rounded to T once.  Minimum / maximum propagate NaN."""
import math

import numpy as np

INT32 = ("status", "it", "flags", "nf_new", "ok_new")
INT64 = ("inner", "nfact", "nlin", "nbk")
MASKS = ("phase0", "act", "need", "brk", "ext", "lsm", "rej", "chk", "done_in", "tired", "small_res", "bt")
SIZES = ("B", "n", "m", "p", "P", "N", "nnzjF", "nnzjc", "max_inner")
ELEM_SCALARS = ("dmin", "rhomax", "delta_dec", "smax", "gammaA", "eps2")


def huge(T):
    """T(1e60), src/CaNNOLeS.jl:638, 647: Inf32 for Float32"""
    return T(1e60) if T is np.float64 else T(np.inf)


def tmax(a, b):
    return type(a)(np.nan) if (a != a or b != b) else (a if a > b else b)


def tmin(a, b):
    return type(a)(np.nan) if (a != a or b != b) else (a if a < b else b)


def rsum(T, terms):
    """the reductions' rule: wide terms, one exact sum, one rounding to T"""
    with np.errstate(all="ignore"):
        return T(math.fsum(terms))


def rdot(T, a, b):
    return rsum(T, [float(u) * float(v) for u, v in zip(a, b)])


def width(S, k):
    """entries per row of array member k"""
    if k in ("d", "d_new", "rhs_cur", "rhs_t", "ls_g"):
        return S["N"]
    if k in ("x", "xt", "xt_e", "xl"):
        return S["n"]
    if k in ("r", "Fx", "rt", "Ft", "rt_e", "Fl"):
        return S["m"]
    if k in ("cx", "lam", "ct", "lamt", "lamt_e", "cl", "lam_ls"):
        return S["P"]
    if k in ("Jv", "Jt"):
        return S["nnzjF"]
    if k in ("Jcv", "Jct"):
        return S["nnzjc"]
    return 2 if k == "nrm_t" else 1


def dual_scaling(S, b):
    """max(smax, sum |lam| / p) / smax, 1 without constraints (outer_loop.solve: dual_scaling)"""
    T, p = S["T"], S["p"]
    if p == 0:
        return T(1)
    sl = rsum(T, [abs(float(v)) for v in S["lam"][b, :p]])
    return tmax(sl / T(p), S["smax"]) / S["smax"]


def begin(S):
    """src/CaNNOLeS.jl:612-626: start of an outer iteration where phase0; act, need; flags[0..3]; all eight flag words start at 0"""
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
            need = act and inner != 1   # the iteration behind a rejected extrapolation keeps d (:627)
            S["act"][b], S["need"][b], S["brk"][b] = act, need, 0
            if act:
                S["flags"][0] = 1
            if need:
                S["flags"][1] = 1
            if act and inner == 0:
                S["flags"][2] = 1
            if act and inner > 0:
                S["flags"][3] = 1


def newton_done(S, did_newton):
    """:633-659: the Newton call's outputs where `need`, `broken`, lam_ls, ext / lsm, eps_k where ext"""
    T, p, N = S["T"], S["p"], S["N"]
    with np.errstate(all="ignore"):
        for b in range(S["B"]):
            act = S["act"][b] != 0
            if did_newton:
                need = S["need"][b] != 0
                bad = rsum(np.float64, [0.0 if math.isfinite(float(v)) else 1.0 for v in S["d_new"][b, :N]])
                if need:
                    S["d"][b, :N] = S["d_new"][b, :N]
                    S["rho_old"][b] = S["ro_tmp"][b]
                    S["nfact"][b] += int(S["nf_new"][b])
                    S["nlin"][b] += 1
                brk = bool(need and (S["rho_new"][b] > S["rhomax"] or S["ok_new"][b] == 0 or bad != 0.0 or S["fx"][b] >= huge(T)))   # :638-652
                S["brk"][b] = brk
                if brk:
                    act = False
                    S["act"][b] = 0
            if S.get("lam_ls") is not None:   # lam - c / delta (:1066), for every problem
                dl = S["delta"][b]
                for k in range(S["P"]):
                    S["lam_ls"][b, k] = S["lam"][b, k] - S["cx"][b, k] / dl if p > 0 else S["lam"][b, k]
            inner = int(S["inner"][b])
            ext, lsm = act and inner == 0, act and inner > 0
            S["ext"][b], S["lsm"][b] = ext, lsm
            if ext:   # :659
                e = S["epsk"][b]
                S["epsk"][b] = tmax(tmin(T(1e3) * S["delta"][b], T(99) * e / T(100)), T(9) * e / T(10))


def extrapolated(S):
    """:661-668: the extrapolation's trial point where ext"""
    n, m, P = S["n"], S["m"], S["P"]
    for b in range(S["B"]):
        if S["ext"][b]:
            S["xt"][b, :n] = S["xt_e"][b, :n]
            S["rt"][b, :m] = S["rt_e"][b, :m]
            S["lamt"][b, :P] = S["lamt_e"][b, :P]


def trial_done(S):
    """:722-800: measures at the trial point, acceptance, the state update, delta, inner, the end-of-inner-loop tests; flags[4], [5]"""
    T, n, m, p, P, N = S["T"], S["n"], S["m"], S["p"], S["P"], S["N"]
    with np.errstate(all="ignore"):
        for b in range(S["B"]):
            act, brk = S["act"][b] != 0, S["brk"][b] != 0
            inner0 = int(S["inner"][b])
            ss = rdot(T, S["Ft"][b, :m], S["Ft"][b, :m])
            ndh, nph, chat = S["ndh"][b], S["nph"][b], S["combined_hat"][b]
            if act:   # :722-732
                ndh, nph = S["nrm_t"][b, 0], S["nrm_t"][b, 1]
                chat = ndh + nph
            S["ndh"][b], S["nph"][b], S["combined_hat"][b] = ndh, nph, chat
            epsk = S["epsk"][b]
            good = bool(chat <= T(0.99) * S["combined"][b] + epsk)   # :733
            acc_state = act and (inner0 > 0 or good)
            acc_lam = act and good
            if acc_state:
                S["fx"][b] = T(0.5) * ss
            delta = S["delta"][b]
            delta_next = delta
            if p > 0:   # :758-763
                dr = act and inner0 > 0 and bool(ndh <= T(0.99) * S["normdual"][b] + epsk / T(2)) \
                    and bool(nph > T(0.99) * S["normprimal"][b] + epsk / T(2))
                if dr:
                    delta_next = tmax(delta / T(10), S["dmin"])
            inner = inner0 + (1 if act else 0)
            S["inner"][b] = inner
            tired = inner > S["max_inner"]
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
            # :765-800
            sc = rsum(T, [float(v) * float(v) for v in S["cx"][b, :p]])
            first_order = bool(tmax(S["normdual"][b] / dual_scaling(S, b), S["normprimal"][b]) <= S["epstol"][b])
            small_res = bool(T(2) * np.sqrt(S["fx"][b]) <= S["epsF"][b]) and bool(np.sqrt(sc) <= S["epsc"][b])
            S["small_res"][b] = small_res
            chk = done_in and small_res and not first_order
            S["chk"][b] = chk
            if chk:
                S["flags"][5] = 1


def merit(S, b, F, c, eta):
    """phi = |F|^2 / 2 - lam'c + eta |c|^2 / 2, :1054-1064"""
    T, m, p = S["T"], S["m"], S["p"]
    phi = T(0.5) * rdot(T, F[b, :m], F[b, :m])
    if p > 0:
        phi = phi - rdot(T, S["lam"][b, :p], c[b, :p])
        phi = phi + eta * rdot(T, c[b, :p], c[b, :p]) / T(2)
    return phi


def ls_begin(S):
    """:1065-1075: Dphi = g'dx, eta = 1 / delta where lsm (p > 0), phi(x), alpha = 1, xl = x + dx — written for every problem"""
    T, n, p = S["T"], S["n"], S["p"]
    with np.errstate(all="ignore"):
        for b in range(S["B"]):
            dp = rdot(T, S["ls_g"][b, :n], S["d"][b, :n])
            eta = S["eta"][b]
            if p > 0 and S["lsm"][b]:
                eta = T(1) / S["delta"][b]
            phix = merit(S, b, S["Fx"], S["cx"], eta)
            S["Dphi"][b], S["eta"][b], S["phix"][b], S["alpha"][b] = dp, eta, phix, T(1)
            for k in range(n):
                S["xl"][b, k] = S["x"][b, k] + S["d"][b, k]


def ls_test(S, first):
    """the Armijo test (:1080-1098) of the lsm problems (first) or of those still backtracking; flags[6] = any bt"""
    S["flags"][6] = 0
    with np.errstate(all="ignore"):
        for b in range(S["B"]):
            cand = S["lsm"][b] != 0 if first else S["bt"][b] != 0
            if not cand:
                if first:
                    S["bt"][b] = 0
                continue
            phil = merit(S, b, S["Fl"], S["cl"], S["eta"][b])
            alpha = S["alpha"][b]
            bt = not bool(phil <= S["phix"][b] + S["gammaA"] * alpha * S["Dphi"][b])
            if not first:
                bt = bt and bool(alpha >= S["eps2"])   # :1106
            S["bt"][b] = bt
            if bt:
                S["flags"][6] = 1


def ls_step(S):
    """:1098-1105 where bt: alpha / 4, xl = x + alpha dx, nbk + 1"""
    T, n = S["T"], S["n"]
    with np.errstate(all="ignore"):
        for b in range(S["B"]):
            if not S["bt"][b]:
                continue
            alpha = S["alpha"][b] / T(4)
            for k in range(n):
                S["xl"][b, k] = S["x"][b, k] + alpha * S["d"][b, k]
            S["alpha"][b] = alpha
            S["nbk"][b] += 1


def ls_take(S):
    """the accepted point of the line search becomes the trial point where lsm"""
    n, m, P = S["n"], S["m"], S["P"]
    for b in range(S["B"]):
        if S["lsm"][b]:
            S["xt"][b, :n] = S["xl"][b, :n]
            S["rt"][b, :m] = S["Fl"][b, :m]
            S["lamt"][b, :P] = S["lam_ls"][b, :P]


def end(S):
    """:800-857 where done_in: the status (first_order, small_residual, exception, stalled in that order; inner > max_inner is `stalled`,
    :846), it + 1, phase0"""
    with np.errstate(all="ignore"):
        for b in range(S["B"]):
            if not S["done_in"][b]:
                continue
            first_order = bool(tmax(S["normdual"][b] / dual_scaling(S, b), S["normprimal"][b]) <= S["epstol"][b])
            S["it"][b] += 1
            S["status"][b] = 1 if first_order else 2 if S["small_res"][b] else 3 if S["brk"][b] else 5 if S["tired"][b] else 0
            S["phase0"][b] = 1


def new_state(T, B, n, m, p, nnzjF=1, nnzjc=None, rows=None, max_inner=10, dmin=1e-8, rhomax=1e10, delta_dec=0.1, smax=100.0, gammaA=1e-2,
              eps2=None, share_jc=False):
    """a zero state of B problems in `rows` (default B) rows"""
    rows = B if rows is None else rows
    nnzjc = (3 if p else 0) if nnzjc is None else nnzjc
    S = dict(T=T, B=B, n=n, m=m, p=p, P=max(p, 1), N=n + m + p, nnzjF=nnzjF, nnzjc=nnzjc, max_inner=max_inner, dmin=T(dmin), rhomax=T(rhomax),
             delta_dec=T(delta_dec), smax=T(smax), gammaA=T(gammaA), eps2=T(float(np.finfo(T).eps) ** 2 if eps2 is None else eps2))
    for k in ARRAYS:
        if k == "flags":
            S[k] = np.zeros(8, np.int32)
        elif k in ("Jcv", "Jct") and nnzjc == 0:
            S[k] = None
        elif k == "Jct" and share_jc:
            S[k] = S["Jcv"]
        else:
            dt = np.int32 if k in INT32 else np.int64 if k in INT64 else np.uint8 if k in MASKS else T
            w = width(S, k)
            S[k] = np.zeros(rows if w == 1 and k not in ROW_ARRAYS else (rows, w), dt)
    return S


ROW_ARRAYS = ("d", "d_new", "rhs_cur", "rhs_t", "ls_g", "x", "xt", "xt_e", "xl", "r", "Fx", "rt", "Ft", "rt_e", "Fl", "cx", "lam", "ct", "lamt", "lamt_e",
              "cl", "lam_ls", "Jv", "Jt", "Jcv", "Jct", "nrm_t")
ARRAYS = ("status", "it", "flags", "nf_new", "ok_new", "inner", "nfact", "nlin",
          "phase0", "act", "need", "brk", "ext", "lsm", "rej", "chk", "done_in", "tired", "small_res",
          "normdual", "normprimal", "combined", "combined_hat", "delta", "ndh", "nph", "fx", "epsk", "epstol", "epsF", "epsc", "rho_old",
          "d", "d_new", "ro_tmp", "rho_new", "x", "r", "Fx", "cx", "Jv", "Jcv", "lam", "rhs_cur",
          "xt", "rt", "Ft", "ct", "Jt", "Jct", "lamt", "rhs_t", "nrm_t", "xt_e", "rt_e", "lamt_e",
          "ls_g", "xl", "Fl", "cl", "lam_ls", "alpha", "Dphi", "phix", "eta", "nbk", "bt")


def copy_state(S):
    """a deep copy that keeps Jcv / Jct aliased where they are"""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in S.items()}
    if S.get("Jct") is not None and S["Jct"] is S["Jcv"]:
        out["Jct"] = out["Jcv"]
    return out
