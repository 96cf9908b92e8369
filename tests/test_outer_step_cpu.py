"""tests/support/outer_step_sim.py — the plain restatement the GPU tests compare the step kernels of csrc/outer_step.hip with — pinned
without a GPU: one hand-computed case per rule (the expected numbers are written out), and a whole trajectory: the simulator's nine
functions, driven in the order device_loop.solve_batch_device calls the kernels with the host model callbacks and the CPU oracle's
newton_system, must reproduce outer_loop.solve problem by problem."""
import numpy as np
import pytest

from tests.support import outer_step_sim as sim

F64, F32 = np.float64, np.float32


def _state(T=F64, B=1, **kw):
    """B problems with n = m = 2, p = 1 (or as given), active, mid-iteration, every threshold far away unless a test moves it"""
    kw.setdefault("p", 1)
    S = sim.new_state(T, B, 2, 2, kw.pop("p"), **kw)
    S["delta"][:] = 1
    S["epsk"][:] = 1000
    S["epstol"][:] = -1          # never first_order
    S["epsF"][:] = -1            # never small_residual
    S["epsc"][:] = -1
    S["act"][:] = 1
    S["ok_new"][:] = 1
    return S


@pytest.mark.parametrize("T", [F64, F32])
def test_delta_rule_of_begin_on_both_sides_of_each_clamp(T):
    """delta = max(min(delta_dec delta, combined), dmin) with delta_dec = 0.5, delta = 0.5 (product 0.25):
    combined 1 -> 0.25; combined 0.125 -> 0.125; combined 0.25 -> 0.25; dmin 0.5 -> 0.5; dmin 0.25 -> 0.25; combined NaN -> NaN"""
    cases = [(0.75, 0.25, 2.0 ** -20, 0.25), (0.0625, 0.0625, 2.0 ** -20, 0.125), (0.125, 0.125, 2.0 ** -20, 0.25), (0.75, 0.25, 0.5, 0.5),
             (0.75, 0.25, 0.25, 0.25), (0.0625, 0.0625, 0.25, 0.25), (np.nan, 0.25, 2.0 ** -20, np.nan)]
    for nd, npr, dmin, want in cases:
        S = _state(T, delta_dec=0.5, dmin=dmin)
        S["delta"][0], S["phase0"][0], S["normdual"][0], S["normprimal"][0], S["inner"][0] = 0.5, 1, nd, npr, 7
        S["flags"][:] = 9
        sim.begin(S)
        assert S["delta"].dtype == T and (S["delta"][0] == T(want) or (want != want and S["delta"][0] != S["delta"][0])), (nd, npr, dmin)
        assert (S["combined"][0] == T(nd) + T(npr)) or nd != nd
        assert S["inner"][0] == 0 and S["phase0"][0] == 0 and S["combined_hat"][0] == np.inf and S["ndh"][0] == T(nd) or nd != nd
        assert S["flags"].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    # not in phase0: nothing of the iteration start; inner = 1 needs no Newton system; inner = 2 does; a finished problem is not active
    for inner, status, want in [(1, 0, (1, 0, [1, 0, 0, 1])), (2, 0, (1, 1, [1, 1, 0, 1])), (0, 0, (1, 1, [1, 1, 1, 0])), (0, 1, (0, 0, [0, 0, 0, 0]))]:
        S = _state(T)
        S["delta"][0], S["inner"][0], S["status"][0], S["brk"][0], S["phase0"][0] = 0.5, inner, status, 1, status
        sim.begin(S)
        assert (S["act"][0], S["need"][0], S["flags"][:4].tolist()) == want and S["delta"][0] == 0.5 and S["brk"][0] == 0 and S["inner"][0] == inner
        assert S["phase0"][0] == status


@pytest.mark.parametrize("T", [F64, F32])
def test_eps_k_rule_on_both_sides_of_each_clamp(T):
    """eps_k = max(min(1e3 delta, 99 e / 100), 9 e / 10) with e = 1000 (990 and 900): delta 1 -> 990; 0.9375 -> 937.5; 0.5 -> 900;
    0.90625 -> 906.25 and 0.984375 -> 984.375 (just inside either clamp); NaN delta -> NaN; only where ext"""
    for delta, want in [(1.0, 990.0), (0.9375, 937.5), (0.5, 900.0), (0.90625, 906.25), (0.984375, 984.375), (np.nan, np.nan)]:
        S = _state(T)
        S["delta"][0] = delta
        sim.newton_done(S, 0)
        assert S["ext"][0] == 1 and S["lsm"][0] == 0
        assert S["epsk"][0] == T(want) or (want != want and S["epsk"][0] != S["epsk"][0]), delta
    S = _state(T)
    S["inner"][0] = 1
    sim.newton_done(S, 0)
    assert (S["ext"][0], S["lsm"][0], S["epsk"][0]) == (0, 1, 1000)
    S = _state(T)
    S["act"][0] = 0
    sim.newton_done(S, 0)
    assert (S["ext"][0], S["lsm"][0], S["epsk"][0]) == (0, 0, 1000)


@pytest.mark.parametrize("T", [F64, F32])
def test_broken_causes_counters_and_lam_ls(T):
    ulp_up = lambda v: np.nextafter(T(v), T(np.inf))
    big = [1e60, np.nextafter(1e60, 0)] if T is F64 else [np.inf, 3e38]
    cases = {"none": ({}, 0), "rho one ulp above": (dict(rho_new=ulp_up(1e10)), 1), "rho equal": (dict(rho_new=T(1e10)), 0), "not ok": (dict(ok_new=0), 1),
             "fx huge": (dict(fx=T(big[0])), 1), "fx below huge": (dict(fx=T(big[1])), 0)}
    for name, (over, want) in cases.items():
        for need in (1, 0):
            S = _state(T)
            S["need"][0], S["nf_new"][0], S["ro_tmp"][0], S["d_new"][0], S["nfact"][0], S["nlin"][0] = need, 3, 0.25, [1, 2, 3, 4, 5], 10, 20
            S["lam"][0], S["cx"][0], S["delta"][0] = 3.0, 1.0, 0.5
            for k, v in over.items():
                S[k][0] = v
            sim.newton_done(S, 1)
            assert S["brk"][0] == (want and need), (name, need)
            assert S["act"][0] == (0 if want and need else 1) and S["ext"][0] == S["act"][0]
            assert (S["nfact"][0], S["nlin"][0], S["rho_old"][0]) == ((13, 21, 0.25) if need else (10, 20, 0.0)), name   # counted also when broken
            assert S["d"][0].tolist() == ([1, 2, 3, 4, 5] if need else [0] * 5)
            assert S["lam_ls"][0, 0] == 1.0   # 3 - 1 / 0.5
    for k, v in [(4, np.inf), (0, np.nan), (2, -np.inf)]:
        for need in (1, 0):
            S = _state(T)
            S["need"][0] = need
            S["d_new"][0, k] = v
            sim.newton_done(S, 1)
            assert S["brk"][0] == need and S["act"][0] == 1 - need
    S = _state(T, p=0)
    S["lam"][0], S["cx"][0], S["lam_ls"][0], S["brk"][0] = 3.0, 1.0, 7.0, 1
    sim.newton_done(S, 0)
    assert S["lam_ls"][0, 0] == 3.0 and S["brk"][0] == 1   # p == 0: lam_ls = lam; no Newton call: brk stays
    S["lam_ls"] = None
    sim.newton_done(S, 1)
    assert S["brk"][0] == 0


def _trial(T, act=1, brk=0, inner=0, chat=(1.0, 1.0), combined=100.0, epsk=1.0, **over):
    S = _state(T, **{k: over.pop(k) for k in ("p", "max_inner", "dmin") if k in over})
    S["act"][0], S["brk"][0], S["inner"][0], S["combined"][0], S["epsk"][0] = act, brk, inner, combined, epsk
    S["nrm_t"][0] = chat
    S["normdual"][0], S["normprimal"][0], S["ndh"][0], S["nph"][0], S["combined_hat"][0] = 50, 60, 7, 8, 15
    S["xt"][0], S["rt"][0], S["Ft"][0], S["ct"][0], S["lamt"][0], S["Jt"][0], S["rhs_t"][0] = [1, 2], [3, 4], [3, 4], 5, 6, 7, 8
    if S["nnzjc"]:
        S["Jct"][0] = 9
    for k, v in over.items():
        S[k][0] = v
    sim.trial_done(S)
    return S


@pytest.mark.parametrize("T", [F64, F32])
def test_acceptance_table_of_trial_done(T):
    """good = chat <= T(0.99) combined + epsk with combined = 100, epsk = 1 (threshold 100): chat = 2 is good, chat = 200 is not.
    inner == 0: state and multipliers accepted only if good.  inner > 0: the state always, the multipliers if good."""
    for inner in (0, 3):
        for chat, good in (((1.0, 1.0), True), ((150.0, 50.0), False)):
            S = _trial(T, inner=inner, chat=chat)
            acc_state = inner > 0 or good
            assert S["x"][0].tolist() == ([1, 2] if acc_state else [0, 0]) and S["r"][0].tolist() == ([3, 4] if acc_state else [0, 0])
            assert S["Fx"][0].tolist() == ([3, 4] if acc_state else [0, 0]) and S["cx"][0, 0] == (5 if acc_state else 0)
            assert S["Jv"][0, 0] == (7 if acc_state else 0) and S["Jcv"][0, 0] == (9 if acc_state else 0)
            assert S["fx"][0] == (12.5 if acc_state else 0)                    # (9 + 16) / 2
            assert S["lam"][0, 0] == (6 if good else 0)
            assert (S["rej"][0], S["done_in"][0], S["inner"][0], S["tired"][0]) == (not good, good, inner + 1, 0)
            assert S["rhs_cur"][0].tolist() == [8] * 5 and S["flags"][4] == (not good)
            assert (S["ndh"][0], S["nph"][0], S["combined_hat"][0]) == (chat[0], chat[1], chat[0] + chat[1])
            assert (S["normdual"][0], S["normprimal"][0]) == ((chat[0], chat[1]) if good else (50, 60))
    # not active: nothing is accepted, inner stays; broken: the iteration ends with the old measures
    for brk in (0, 1):
        S = _trial(T, act=0, brk=brk, inner=2)
        assert S["x"][0].tolist() == [0, 0] and S["lam"][0, 0] == 0 and S["rhs_cur"][0].tolist() == [0] * 5 and S["fx"][0] == 0
        assert (S["rej"][0], S["done_in"][0], S["inner"][0]) == (0, brk, 2)
        assert (S["ndh"][0], S["nph"][0], S["combined_hat"][0]) == (7, 8, 15)
        assert (S["normdual"][0], S["normprimal"][0]) == ((7, 8) if brk else (50, 60))
    # the threshold itself, one ulp either side
    thr = T(0.99) * T(100) + T(1)
    for nd, good in ((thr, True), (np.nextafter(thr, T(np.inf)), False), (np.nextafter(thr, T(0)), True)):
        S = _trial(T, chat=(nd, 0.0))
        assert S["done_in"][0] == good and S["rej"][0] == (not good)
    # the inner-iteration limit: inner reaches max_inner (not tired), max_inner + 1 (tired: done though rejected)
    for inner, tired in ((4, 0), (5, 1)):
        S = _trial(T, inner=inner, chat=(150.0, 50.0), max_inner=5)
        assert (S["inner"][0], S["tired"][0], S["done_in"][0], S["rej"][0]) == (inner + 1, tired, tired, 1)


@pytest.mark.parametrize("T", [F64, F32])
def test_delta_over_ten_rule(T):
    """dr = inner > 0, ndh <= T(0.99) normdual + epsk / 2 and nph > T(0.99) normprimal + epsk / 2 (p > 0): with normdual = 50,
    normprimal = 60, epsk = 1 the thresholds are T(0.99) 50 + 0.5 and T(0.99) 60 + 0.5"""
    td, tp = T(0.99) * T(50) + T(0.5), T(0.99) * T(60) + T(0.5)
    up, dn = (lambda v: np.nextafter(v, T(np.inf))), (lambda v: np.nextafter(v, T(0)))
    for nd, npr, inner, p, want in [(td, up(tp), 1, 1, True), (up(td), up(tp), 1, 1, False), (td, tp, 1, 1, False), (dn(td), T(70), 2, 1, True),
                                    (td, up(tp), 0, 1, False), (td, up(tp), 1, 0, False)]:
        S = _trial(T, inner=inner, chat=(nd, npr), p=p, delta=T(0.5))
        assert S["delta"][0] == (T(0.5) / T(10) if want else T(0.5)), (nd, npr, inner, p)
    S = _trial(T, inner=1, chat=(td, T(70)), delta=T(0.5), dmin=0.25)
    assert S["delta"][0] == 0.25                                              # the floor
    S = _trial(T, act=0, inner=1, chat=(td, T(70)), delta=T(0.5), ndh=td, nph=T(70))
    assert S["delta"][0] == 0.5                                               # not active


@pytest.mark.parametrize("T", [F64, F32])
def test_end_of_inner_loop_tests(T):
    """first_order = max(normdual / ds, normprimal) <= epstol with ds = max(sum|lam| / p, smax) / smax; small_res = 2 sqrt(fx) <= epsF and
    sqrt(sum c^2) <= epsc; chk = done_in, small_res and not first_order"""
    # accepted: normdual = 8, normprimal = 1, lam = lamt = 400 -> ds = 4 -> measure 2; fx = 12.5 -> 2 sqrt(fx) = 7.07.., c = 5
    for epstol, fo in ((2.0, True), (1.96875, False), (np.nan, False)):
        for epsF, epsc, sr in ((8.0, 5.0, True), (4.0, 5.0, False), (8.0, 4.96875, False)):
            S = _trial(T, chat=(8.0, 1.0), lamt=400.0, epstol=epstol, epsF=epsF, epsc=epsc)
            assert S["small_res"][0] == sr and S["chk"][0] == (sr and not fo) and S["flags"][5] == (sr and not fo), (epstol, epsF, epsc)
    for epstol, fo in ((8.0, True), (7.96875, False)):         # sum|lam| / p below smax: ds = 1, measure 8
        S = _trial(T, chat=(8.0, 1.0), lamt=50.0, epstol=epstol, epsF=8.0, epsc=5.0)
        assert S["small_res"][0] == 1 and S["chk"][0] == (not fo)
    S = _trial(T, chat=(150.0, 50.0), epsF=8.0, epsc=8.0)      # small_res but the iteration goes on: no check
    assert S["small_res"][0] == 1 and S["chk"][0] == 0 and S["done_in"][0] == 0
    S = _trial(T, chat=(8.0, 1.0), p=0, epstol=8.0, epsF=8.0, epsc=0.0, lam=1e6)   # p == 0: ds = 1, no constraint part
    assert S["small_res"][0] == 1 and S["chk"][0] == 0
    S = _trial(T, chat=(8.0, 1.0), p=0, epstol=7.96875, epsF=8.0, epsc=0.0)
    assert S["chk"][0] == 1


@pytest.mark.parametrize("T", [F64, F32])
def test_armijo_test_first_and_later_rounds(T):
    """bt = not (phi(xl) <= phix + gammaA alpha Dphi); in a backtracking round also alpha >= eps2.  p = 1: phi = |F|^2 / 2 - lam c + eta c^2 / 2;
    Fl = (3, 4), cl = 2, lam = 1.5, eta = 4: phi = 12.5 - 3 + 8 = 17.5.  gammaA = 0.25, alpha = 0.5, Dphi = -4: phix - 0.5."""
    def run(first, phix, alpha=0.5, Dphi=-4.0, lsm=1, bt=1):
        S = _state(T, gammaA=0.25, eps2=2.0 ** -10)
        S["Fl"][0], S["cl"][0], S["lam"][0], S["eta"][0] = [3, 4], 2, 1.5, 4
        S["phix"][0], S["alpha"][0], S["Dphi"][0], S["lsm"][0], S["bt"][0], S["flags"][6] = phix, alpha, Dphi, lsm, bt, 1
        sim.ls_test(S, first)
        assert S["flags"][6] == S["bt"][0]
        return int(S["bt"][0])
    for first in (1, 0):
        assert run(first, 18.0) == 0                                          # satisfied at equality
        assert run(first, np.nextafter(T(18.0), T(0))) == 1                   # failed by one ulp
    assert run(1, 0.0, lsm=0) == 0 and run(0, 0.0, bt=0, lsm=1) == 0          # not a candidate
    assert run(0, 0.0, lsm=0, bt=1) == 1                                      # a later round looks at bt alone
    # alpha against eps2 = 2^-10, Armijo failed: the first test ignores it; a later round stops below it
    for alpha, later in ((2.0 ** -10, 1), (2.0 ** -11, 0), (2.0 ** -9, 1)):
        assert run(1, 0.0, alpha=alpha) == 1 and run(0, 0.0, alpha=alpha) == later
    assert run(0, 17.0, Dphi=4.0, alpha=2.0 ** -11) == 0                      # Dphi > 0 ends through eps2 only
    # ls_begin: Dphi = g'dx over the first n entries, eta = 1 / delta where lsm, phi(x), alpha = 1, xl = x + dx
    for lsm in (1, 0):
        S = _state(T)
        S["ls_g"][0], S["d"][0], S["x"][0], S["Fx"][0], S["cx"][0], S["lam"][0] = [1, 2, 100, 100, 100], [3, -4, 9, 9, 9], [10, 20], [3, 4], 2, 1.5
        S["delta"][0], S["eta"][0], S["lsm"][0] = 0.25, 1.0, lsm
        sim.ls_begin(S)
        assert (S["Dphi"][0], S["alpha"][0], S["eta"][0]) == (-5, 1, 4 if lsm else 1) and S["xl"][0].tolist() == [13, 16]
        assert S["phix"][0] == (17.5 if lsm else 11.5)
    S = _state(T)
    S["x"][0], S["d"][0], S["alpha"][0], S["bt"][0], S["nbk"][0] = [10, 20], [4, -8, 9, 9, 9], 1, 1, 5
    sim.ls_step(S)
    assert (S["alpha"][0], S["nbk"][0]) == (0.25, 6) and S["xl"][0].tolist() == [11, 18]
    S["bt"][0] = 0
    sim.ls_step(S)
    assert (S["alpha"][0], S["nbk"][0]) == (0.25, 6)


@pytest.mark.parametrize("T", [F64, F32])
def test_status_chain_of_end(T):
    """first_order > small_residual > exception > stalled, for every combination; nothing without done_in"""
    for done_in in (1, 0):
        for code in range(16):
            fo, sr, brk, tired = code >> 3 & 1, code >> 2 & 1, code >> 1 & 1, code & 1
            S = _state(T)
            S["normdual"][0], S["normprimal"][0], S["epstol"][0] = 8, 1, (8 if fo else 7.96875)
            S["small_res"][0], S["brk"][0], S["tired"][0], S["done_in"][0], S["it"][0], S["status"][0] = sr, brk, tired, done_in, 4, 0
            sim.end(S)
            want = 1 if fo else 2 if sr else 3 if brk else 5 if tired else 0
            assert (S["status"][0], S["it"][0], S["phase0"][0]) == ((want, 5, 1) if done_in else (0, 4, 0)), (done_in, code)
    S = _state(T)
    S["normdual"][0], S["normprimal"][0], S["epstol"][0], S["lam"][0], S["done_in"][0] = 8, 1, 2, 400, 1   # ds = 4
    sim.end(S)
    assert S["status"][0] == 1


def test_masked_copies_and_reductions_round_once():
    S = _state(F64, B=2)
    S["ext"][:], S["lsm"][:] = [1, 0], [0, 1]
    S["xt_e"][:], S["rt_e"][:], S["lamt_e"][:], S["xl"][:], S["Fl"][:], S["lam_ls"][:] = 1, 2, 3, 4, 5, 6
    sim.extrapolated(S)
    assert S["xt"].tolist() == [[1, 1], [0, 0]] and S["rt"].tolist() == [[2, 2], [0, 0]] and S["lamt"].tolist() == [[3], [0]]
    sim.ls_take(S)
    assert S["xt"].tolist() == [[1, 1], [4, 4]] and S["rt"].tolist() == [[2, 2], [5, 5]] and S["lamt"].tolist() == [[3], [6]]
    # a Float32 sum is the exact sum rounded once: 2^24 + 1 + 1 = 2^24 + 2 (a float32 running sum would stay at 2^24)
    assert sim.rsum(F32, [2.0 ** 24, 1.0, 1.0]) == F32(2.0 ** 24 + 2) and sim.rdot(F32, [F32(4096), F32(1)], [F32(4096), F32(2)]) == F32(2.0 ** 24 + 2)
    assert sim.huge(F32) == np.inf and sim.huge(F64) == 1e60
    assert sim.tmax(F64(np.nan), F64(1)) != sim.tmax(F64(np.nan), F64(1)) and sim.tmin(F32(1), F32(np.nan)) != sim.tmin(F32(1), F32(np.nan))
    assert sim.tmax(F32(1), F32(2)) == 2 and sim.tmin(F32(1), F32(2)) == 1


# ---- the trajectory ------------------------------------------------------------------------------------------------------------------------

def drive_simulator(fam, idx, prm, max_inner=10000):
    """the lockstep loop of device_loop.solve_batch_device on the problems `idx` of `fam` with the simulator in place of the kernels, the
    host model callbacks in place of the device ones and the CPU oracle for the Newton systems (Float64)"""
    from cannoles_jl_amd import device_loop as DL, outer_loop
    from tests.test_oracle_pinning import oracle_newton, oracle_solver
    s = fam.s
    n, m, p = s.nvar, s.nequ, s.ncon
    rows, cols, (nnzhF, nnzhc, nnzjF, nnzjc) = DL.kkt_pattern_of(fam)
    M = [fam.host_model(b) for b in idx]
    B, N = len(idx), n + m + p
    eps = np.finfo(float).eps
    S = sim.new_state(F64, B, n, m, p, nnzjF=nnzjF, nnzjc=nnzjc, max_inner=max_inner, dmin=prm[1], rhomax=prm[6], gammaA=prm[8], share_jc=True)
    o_jF = nnzhF + nnzhc
    o_jc, o_I = o_jF + nnzjF, o_jF + nnzjF + nnzjc
    vals = np.ones(len(rows))
    vals[o_I:o_I + m] = -1.0
    LDLT = [oracle_solver(N, rows, cols, vals, n, m, p) for _ in idx]
    J = lambda b, x: (M[b].jac_residual(x), M[b].jac(x) if p else np.zeros((0, n)))
    cons = lambda b, x: M[b].cons(x) if p else np.zeros(0)

    def rhs_of(b, x, r, lam, F, c):   # [dual; primal] and their infinity norms (cnl_residual_vectors_dev)
        Jx, Jc = J(b, x)
        v = np.concatenate([Jx.T @ r - Jc.T @ lam, F - r, c])
        return v, np.abs(v[:n]).max(), np.abs(v[n:]).max()

    for b in range(B):   # the start, outer_loop.solve up to its loop
        x = M[b].x0.copy()
        S["x"][b], S["Fx"][b] = x, M[b].residual(x)
        S["r"][b], S["cx"][b, :p], S["fx"][b] = S["Fx"][b], cons(b, x), S["Fx"][b] @ S["Fx"][b] / 2
        Jx, Jc = J(b, x)
        if p:
            lam = outer_loop.cgls(Jc.T, Jx.T @ S["r"][b])
            S["lam"][b, :p] = 1.0 if np.linalg.norm(lam) == 0 else lam
        S["rhs_cur"][b], S["normdual"][b], S["normprimal"][b] = rhs_of(b, x, S["r"][b], S["lam"][b, :p], S["Fx"][b], S["cx"][b, :p])
        S["epsF"][b], S["epstol"][b] = np.sqrt(eps) + eps * 2 * np.sqrt(S["fx"][b]), np.sqrt(eps) + np.sqrt(eps) * S["normdual"][b]
        S["epsc"][b] = np.sqrt(S["epstol"][b])
        first_order = max(S["normdual"][b] / sim.dual_scaling(S, b), S["normprimal"][b]) <= S["epstol"][b]
        small = 2 * np.sqrt(S["fx"][b]) <= S["epsF"][b] and np.linalg.norm(S["cx"][b, :p]) <= S["epsc"][b]
        assert not (small and not first_order)   # (the start's small-residual check is not restated: these families do not take it)
        S["status"][b] = 1 if first_order else 2 if small else 0
    S["delta"][:], S["epsk"][:], S["eta"][:], S["phase0"][:] = 1.0, 1e3, (1.0 if p else 0.0), 1
    steps = 0
    while steps < 400:
        sim.begin(S)
        any_act, any_need, any_ext, any_ls = S["flags"][:4]
        if not any_act:
            break
        steps += 1
        for b in np.flatnonzero(S["need"][:B]) if any_need else []:   # prepare_newton_system!, :947-981, and newton_system!
            Jx, Jc = J(b, S["x"][b])
            vals[:nnzhF] = M[b].hess_coord_residual(S["x"][b], S["r"][b])
            vals[o_jF:o_jc] = Jx[M[b].jF_rows - 1, M[b].jF_cols - 1]
            if p:
                vals[nnzhF:o_jF] = -M[b].hess_coord_cons(S["x"][b], S["lam"][b, :p])
                vals[o_jc:o_I] = Jc[M[b].jc_rows - 1, M[b].jc_cols - 1]
                vals[o_I + m:o_I + m + p] = -S["delta"][b]
            vals[o_I + m + p:] = 0.0
            S["d_new"][b], S["ok_new"][b], S["rho_new"][b], S["ro_tmp"][b], S["nf_new"][b] = oracle_newton(
                LDLT[b], n, m, p, S["rhs_cur"][b].copy(), vals, S["rho_old"][b], prm)
        sim.newton_done(S, 1 if any_need else 0)
        if any_ext:
            for b in range(B):   # cnl_trial_point_dev, :661-668
                dlam = -S["d"][b, n + m:]
                if np.linalg.norm(dlam) > 1e4:
                    dlam = dlam * 1e4 / np.linalg.norm(dlam)
                S["xt_e"][b], S["rt_e"][b], S["lamt_e"][b, :p] = S["x"][b] + S["d"][b, :n], S["r"][b] + S["d"][b, n:n + m], S["lam"][b, :p] + dlam
            sim.extrapolated(S)
        if any_ls:
            def model_at_xl():
                for b in range(B):
                    S["Fl"][b], S["cl"][b, :p] = M[b].residual(S["xl"][b]), cons(b, S["xl"][b])
            for b in range(B):
                S["ls_g"][b] = rhs_of(b, S["x"][b], S["Fx"][b], S["lam_ls"][b, :p], S["Fx"][b], S["cx"][b, :p])[0]
            sim.ls_begin(S)
            model_at_xl()
            sim.ls_test(S, 1)
            while S["flags"][6]:
                sim.ls_step(S)
                model_at_xl()
                sim.ls_test(S, 0)
            sim.ls_take(S)
        for b in range(B):
            S["Ft"][b], S["ct"][b, :p] = M[b].residual(S["xt"][b]), cons(b, S["xt"][b])
            S["rhs_t"][b], S["nrm_t"][b, 0], S["nrm_t"][b, 1] = rhs_of(b, S["xt"][b], S["rt"][b], S["lamt"][b, :p], S["Ft"][b], S["ct"][b, :p])
        sim.trial_done(S)
        for b in np.flatnonzero(S["rej"][:B]) if S["flags"][4] else []:   # dual at (x, r, lam) again, :742-747
            S["rhs_cur"][b, :n] = rhs_of(b, S["x"][b], S["r"][b], S["lam"][b, :p], S["Fx"][b], S["cx"][b, :p])[0][:n]
        for b in np.flatnonzero(S["chk"][:B]) if S["flags"][5] else []:   # :873-897
            S["r"][b] = S["Fx"][b]
            Jx, Jc = J(b, S["x"][b])
            if p:
                S["lam"][b, :p] = outer_loop.cgls(Jc.T, Jx.T @ S["r"][b])
            S["rhs_cur"][b], S["normdual"][b], _ = rhs_of(b, S["x"][b], S["r"][b], S["lam"][b, :p], S["r"][b], S["cx"][b, :p])
            S["normprimal"][b] = np.abs(S["cx"][b, :p]).max() if p else 0.0
        sim.end(S)
    names = {0: "unknown", 1: "first_order", 2: "small_residual", 3: "exception", 4: "max_eval", 5: "stalled"}
    return dict(status=[names[int(v)] for v in S["status"]], iter=S["it"], nlinsolve=S["nlin"], nfact=S["nfact"], nbk=S["nbk"], solution=S["x"],
                steps=steps)


TRAJECTORY = dict(curvature=1.5, start=1.0, noise=0.5)   # the family of test_f3_device_resident_lockstep_outer_loop
ROUGH = dict(curvature=3.0, start=2.0, noise=0.5)


def _family(shape, kind, B=12):
    import torch
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import device_loop as DL, synthetic as syn
    n, p = shape
    return DL.BandQuadFamily(syn.band_structure(n, p), B, seed=n + p, torch=torch, device="cpu", **kind)


@pytest.mark.parametrize("case", ["default", "max_inner=1", "rho_max=100"])
def test_simulator_trajectory_reproduces_the_scalar_loop(params, case):
    """four problems of the (300, 4) family in lockstep through the simulator against outer_loop.solve one by one: status, iter, nlinsolve,
    nfact, nbk, the solution to 1e-9 (the tolerance between two Float64 forms of the loop in test_f3_device_resident_lockstep_outer_loop);
    also with the inner-iteration limit at 1 on the rough family (`stalled`) and with rho_max = 100 (`exception`)"""
    from cannoles_jl_amd import outer_loop
    from tests.test_oracle_pinning import oracle_newton, oracle_solver
    fam = _family((300, 4), ROUGH if case == "max_inner=1" else TRAJECTORY)
    prm = np.array(params, dtype=np.float64)
    kw = {}
    idx = [0, 1, 2, 3]
    if case == "max_inner=1":
        kw, idx = dict(max_inner=1), [1, 2, 5, 7]
    if case == "rho_max=100":
        prm[6], idx = 100.0, [3, 4, 5, 9]
    got = drive_simulator(fam, idx, prm, **kw)
    ones = [outer_loop.solve(fam.host_model(b), oracle_solver, oracle_newton, prm, **kw) for b in idx]
    print(f"{case}: problems {idx}: simulator {got['status']}, scalar loop {[o['status'] for o in ones]}, steps = {got['steps']}")
    for k, one in enumerate(ones):
        assert got["status"][k] == one["status"], k
        assert (got["iter"][k], got["nlinsolve"][k], got["nfact"][k], got["nbk"][k]) == (one["iter"], one["nlinsolve"], one["nfact"], one["nbk"]), k
        assert np.allclose(got["solution"][k], one["solution"], atol=1e-9, rtol=1e-9), k
    if case == "default":
        assert got["status"] == ["first_order"] * 4
    if case == "max_inner=1":
        assert sorted(set(got["status"])) == ["first_order", "stalled"]
    if case == "rho_max=100":
        assert sorted(set(got["status"])) == ["exception", "first_order"]
