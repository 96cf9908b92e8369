"""The keywords of the reference's `solve!` in the lockstep loop, on the GPU (-m gpu).

Per kernel: the `_ex` entry points of csrc/outer_step.hip and cnl_outer_hess_mask_dev, both element types, against the numpy restatement
tests/support/outer_ctl_sim.py — every array of the state, `flags`, the control block's `neval` and `hess_upd`, the rows beyond st.B
included, bit for bit (the state machinery, exact mode and comparison are those of tests/test_outer_step_gpu.py).  Shapes: B = 3 and
B = 257 (the second workgroup of the thread-per-problem kernels), n = m = 3, p in {0, 2}.

The loop: solve_batch_device on BandQuadFamily(band_structure(40, p), 12, seed = 40 + p) against outer_loop.solve with the CPU oracle,
problem by problem, on a model wrapper that counts evaluations; status, iter, nlinsolve, nfact, nbk and neval are equal per problem, and
compact = True, compact_min_finished = 1 is bit-equal to compact = False.  Each test asserts what the scalar loop does before it runs the
device."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests.support import outer_ctl_sim as xsim
from tests.support import outer_step_sim as sim
from tests.support.counting_model import CountingModel
from tests.test_outer_step_gpu import EXTRA, F32, F64, _base, _batches, _compare, _Device, _put, _same_bits, _trial_state, types

pytestmark = pytest.mark.gpu

SHAPE_NM = (3, 3)
batches = pytest.mark.parametrize("B", [3, 257])
cons = pytest.mark.parametrize("p", [0, 2])


# ---- the control block on the device -------------------------------------------------------------------------------------------------------

class _DeviceEx(_Device):
    """the state of _Device and a device copy of the control block's arrays (None: the `_ex` calls get ctl = NULL)"""

    def __init__(self, H, ctl):
        super().__init__(H)
        self.ctl_host, self.ctl = ctl, None
        if ctl is not None:
            self.neval = self.torch.from_numpy(ctl["neval"].copy()).to(self.dev)
            self.hess = self.torch.from_numpy(ctl["hess_upd"].copy()).to(self.dev) if ctl["hess_upd"] is not None else None
            self.ctl = self.hipldl.outer_ctl(self.neval.data_ptr(), ctl["evals_per_point"], ctl["always_accept_extrapolation"], ctl["max_iter"],
                                             ctl["max_eval"], self.hess.data_ptr() if self.hess is not None else None)

    def call_ex(self, name, *args):
        fn = getattr(self.hipldl.lib(), "cnl_outer_" + name + ("_f32_dev" if self.f32 else "_dev"))
        self.hipldl._check(fn(C.byref(self.st), *args, C.byref(self.ctl) if self.ctl is not None else None, self.stream))

    def download_ctl(self):
        self.torch.cuda.synchronize(self.dev)
        return dict(neval=self.neval.cpu().numpy(), hess_upd=self.hess.cpu().numpy() if self.hess is not None else None)


def _check_ex(H, ctl, calls):
    """the `_ex` kernels of `calls` on device copies of (H, ctl) against the simulator on other copies; returns the simulator's (state, ctl)"""
    W, wctl = sim.copy_state(H), xsim.copy_ctl(ctl)
    D = _DeviceEx(H, ctl)
    for name, *args in calls:
        getattr(xsim, name)(W, *args, wctl)
        D.call_ex(name, *args)
    _compare(D.download(), W, H["B"])
    if ctl is not None:
        got = D.download_ctl()
        assert np.array_equal(got["neval"], wctl["neval"]), ("neval", got["neval"][:8], wctl["neval"][:8])
        if wctl["hess_upd"] is not None:
            assert np.array_equal(got["hess_upd"], wctl["hess_upd"]), ("hess_upd", got["hess_upd"][:8], wctl["hess_upd"][:8])
    return W, wctl


def _ctl(B, p, seed=0, **kw):
    """a control block for B problems in B + EXTRA rows: neval anything in 0 .. 9, sentinels behind"""
    ctl = xsim.new_ctl(B + EXTRA, 2 if p else 1, **kw)
    rng = np.random.default_rng([seed, B, p])
    ctl["neval"][:B], ctl["neval"][B:] = rng.integers(0, 10, B), -77
    ctl["hess_upd"][:B], ctl["hess_upd"][B:] = rng.integers(0, 2, B), 201
    return ctl


# ---- begin_ex ------------------------------------------------------------------------------------------------------------------------------

@types
@cons
@batches
def test_begin_ex_need_with_always_accept(built, B, p, f32):
    """inner in {0, 1, 2} x status 0 / 1 x phase0 0 / 1, always_accept_extrapolation both ways: need = act and (inner != 1 or always), so
    the problem right behind a rejected extrapolation gets a Newton system only with always_accept; the counter and the mask stay"""
    T = F32 if f32 else F64
    scen = [dict(status=s, phase0=f, inner=i) for s, f, i in itertools.product((0, 1), (0, 1), (0, 1, 2))]
    for always in (0, 1):
        seen = set()
        for j, assign in enumerate(_batches(len(scen), B)):
            H = _base(T, B, SHAPE_NM + (p,), seed=j, dmin=2.0 ** -6)
            for b, s in enumerate(assign):
                _put(H, b, scen[s])
            ctl = _ctl(B, p, seed=j, always_accept_extrapolation=always, max_iter=3, max_eval=5)
            W, wctl = _check_ex(H, ctl, [("begin_ex",)])
            assert np.array_equal(wctl["neval"], ctl["neval"]) and np.array_equal(wctl["hess_upd"], ctl["hess_upd"])
            for b, s in enumerate(assign):
                sc = scen[s]
                act = sc["status"] == 0
                inner = 0 if act and sc["phase0"] else sc["inner"]
                assert W["act"][b] == act and W["need"][b] == (act and (inner != 1 or always == 1)), (sc, always)
                seen.add(s)
            assert W["flags"][1] == (W["need"][:B] != 0).any()
        assert seen == set(range(len(scen)))


# ---- trial_done_ex -------------------------------------------------------------------------------------------------------------------------

MAX_EVAL = 20


def _trial_ex_scenarios():
    """(name, state inputs, neval after the call relative to max_eval).  Defaults of _trial_state: active, inner = 0, good (measures (1, 1/2)
    against the threshold T(0.99) 8 + 1), max_inner = 5.  ext = act and inner == 0, as cnl_outer_newton_done_dev leaves it."""
    bad = (64.0, 8.0)
    sc = []
    for after in (-1, 0, 1):
        sc += [(f"extrapolation rejected, neval {after:+d}", dict(ext=1, nrm_t=bad), after),
               (f"extrapolation accepted, neval {after:+d}", dict(ext=1), after),
               (f"line search, not good, neval {after:+d}", dict(inner=2, ext=0, nrm_t=bad), after),
               (f"line search, good, neval {after:+d}", dict(inner=2, ext=0), after),
               (f"finished, neval {after:+d}", dict(act=0, ext=0), after),
               (f"broken in this step, neval {after:+d}", dict(act=0, brk=1, ext=0), after)]
    return sc


@types
@cons
@batches
def test_trial_done_ex_acceptance_and_the_evaluation_limit(built, B, p, f32):
    """always_accept_extrapolation takes the state (x, r, Fx, cx, Jv, fx) of a rejected extrapolation but not its multipliers, and the
    problem is still `rej`; neval += evals_per_point on the ext rows only; tired exactly where neval after the call is above max_eval
    (rows at max_eval - 1, max_eval and max_eval + 1), and then done_in also where not good; max_eval = -1: never tired"""
    T = F32 if f32 else F64
    scen = _trial_ex_scenarios()
    epp = 2 if p else 1
    for always, max_eval in itertools.product((0, 1), (MAX_EVAL, -1)):
        seen = set()
        for j, assign in enumerate(_batches(len(scen), B)):
            H = _trial_state(T, SHAPE_NM + (p,), 5, False, j, assign, [(n_, over, None) for n_, over, _ in scen])
            ctl = _ctl(B, p, seed=j, always_accept_extrapolation=always, max_eval=max_eval, max_iter=0)
            for b, s in enumerate(assign):
                ext = scen[s][1].get("ext", 0)
                ctl["neval"][b] = MAX_EVAL + scen[s][2] - (epp if ext else 0)
            W, wctl = _check_ex(H, ctl, [("trial_done_ex",)])
            for b, s in enumerate(assign):
                name, over, after = scen[s]
                act, ext, inner0, good = over.get("act", 1), over.get("ext", 0), over.get("inner", 0), "nrm_t" not in over
                assert wctl["neval"][b] == MAX_EVAL + after and wctl["neval"][b] == ctl["neval"][b] + (epp if ext else 0), name
                tired = max_eval >= 0 and after > 0
                assert W["tired"][b] == tired and W["inner"][b] == inner0 + act, (name, max_eval)
                if act:
                    assert W["rej"][b] == (not good) and W["done_in"][b] == (good or tired), (name, max_eval)
                acc_state = act and (inner0 > 0 or always == 1 or good)
                for k, kt in (("x", "xt"), ("r", "rt"), ("Fx", "Ft"), ("cx", "ct"), ("Jv", "Jt")):
                    assert _same_bits(W[k][b], H[kt][b] if acc_state else H[k][b]).all(), (name, always, k)
                assert _same_bits(W["lam"][b], H["lamt"][b] if act and good else H["lam"][b]).all(), (name, always)
                seen.add(s)
        assert seen == set(range(len(scen)))


# ---- ls_test_ex ----------------------------------------------------------------------------------------------------------------------------

@types
@cons
@batches
def test_ls_test_ex_counts_the_candidates_only(built, B, p, f32):
    """first = 1: neval += evals_per_point on the lsm rows; first = 0: on the bt rows; every other row keeps its count.  lsm and bt are
    independent patterns (period 2 and 3), the Armijo decisions are the simulator's"""
    T = F32 if f32 else F64
    epp = 2 if p else 1
    for first in (1, 0):
        H = _base(T, B, SHAPE_NM + (p,), seed=first, gammaA=0.25, eps2=2.0 ** -20)
        H["lsm"][:B], H["bt"][:B] = np.arange(B) % 2, np.arange(B) % 3 == 0
        ctl = _ctl(B, p, seed=first, max_eval=4)
        W, wctl = _check_ex(H, ctl, [("ls_test_ex", first)])
        cand = (H["lsm"][:B] if first else H["bt"][:B]) != 0
        assert cand.any() and not cand.all()
        assert np.array_equal(wctl["neval"][:B], ctl["neval"][:B] + epp * cand) and np.array_equal(wctl["neval"][B:], ctl["neval"][B:])


# ---- end_ex --------------------------------------------------------------------------------------------------------------------------------

CAUSES = ("first_order", "small_res", "brk", "over_eval", "over_iter", "tired")
CHAIN = dict(first_order=1, small_res=2, brk=3, over_eval=4, over_iter=6, tired=5)   # in the order they are tested


def _end_ex_state(T, B, p, seed, assign, scen, max_iter, max_eval):
    """normdual = 4, normprimal = 1/2, sum |lam| / p <= 8 < smax (ds = 1): epstol = 4 is first_order at equality, one ulp less is not;
    over_eval: neval = max_eval + 1 against max_eval; over_iter: it = max_iter before the call (max_iter + 1 after) against max_iter - 1
    (it == max_iter after the call: goes on)"""
    H = _base(T, B, SHAPE_NM + (p,), seed=seed)
    H["status"][:B], H["normdual"][:B], H["normprimal"][:B] = 0, 4.0, 0.5
    ctl = _ctl(B, p, seed=seed, max_iter=max_iter, max_eval=max_eval)
    for b, s in enumerate(assign):
        sc = scen[s]
        _put(H, b, dict(done_in=sc["done_in"], small_res=sc["small_res"], brk=sc["brk"], tired=sc["tired"],
                        epstol=T(4) if sc["first_order"] else np.nextafter(T(4), T(0)), it=8 if sc["over_iter"] else 7))
        ctl["neval"][b] = 21 if sc["over_eval"] else 20
    return H, ctl


@types
@cons
@batches
def test_end_ex_status_chain(built, B, p, f32):
    """all 64 combinations of the six causes with done_in (so every pair set at once, and every larger set): the status is the first that
    holds of first_order 1, small_residual 2, exception 3, max_eval 4, max_iter 6, stalled 5, else 0; it + 1; neval == max_eval and
    it == max_iter (after the increment) stop nothing; max_iter = -1 and max_eval = -1 switch 6 and 4 off; done_in = 0 moves nothing"""
    T = F32 if f32 else F64
    scen = [dict(done_in=1, **{c: code >> i & 1 for i, c in enumerate(CAUSES)}) for code in range(64)]
    scen += [dict(done_in=0, **{c: 1 for c in CAUSES}), dict(done_in=0, **{c: 0 for c in CAUSES})]
    for max_iter, max_eval in ((8, 20), (-1, 20), (8, -1), (-1, -1)):
        seen = set()
        for j, assign in enumerate(_batches(len(scen), B)):
            H, ctl = _end_ex_state(T, B, p, j, assign, scen, max_iter, max_eval)
            W, wctl = _check_ex(H, ctl, [("end_ex",)])
            assert np.array_equal(wctl["neval"], ctl["neval"])
            for b, s in enumerate(assign):
                sc = scen[s]
                on = dict(sc, over_eval=sc["over_eval"] and max_eval >= 0, over_iter=sc["over_iter"] and max_iter >= 0)
                want = next((CHAIN[c] for c in CAUSES if on[c]), 0)
                if sc["done_in"]:
                    assert (W["status"][b], W["it"][b], W["phase0"][b]) == (want, H["it"][b] + 1, 1), (sc, max_iter, max_eval, W["status"][b])
                else:
                    assert (W["status"][b], W["it"][b], W["phase0"][b]) == (0, H["it"][b], H["phase0"][b]), sc
                seen.add(s)
        assert seen == set(range(len(scen)))


# ---- the mask kernel -----------------------------------------------------------------------------------------------------------------------

# Rows of three values whose squares and their partial sums are exact in double in any order (checked below), so that dot(Fx, Fx) is a
# known double.  1e-8 is not a Float32 number: a Float32 dot product is above (nearest float above) or below it, never equal; the
# `between` row has a dot product above 1e-8 in double that rounds to the float below 1e-8 — the mask is 0, because the sum is rounded
# to T once and then compared.
_H = float.fromhex
MASK_ROWS = {
    F64: [("just above", ("0x1.a36e2a8p-14", "0x1.d148p-25", "0x1.7510p-27"), 1),
          ("equal", ("0x1.a36e2ep-14", "0x1.7698p-26", "0x1.7740p-28"), 0),
          ("just below", ("0x1.a36e2e8p-14", "0x1.8120p-27", "0x1.1140p-28"), 0)],
    F32: [("the float above 1e-8", ("0x1.a340p-14", "0x1.38p-19", "0x1.ep-20"), 1),
          ("between: above 1e-8 in double, rounds below", ("0x1.a36e2ap-14", "0x1.d98p-25", "0x1.4dap-26"), 0),
          ("just below", ("0x1.a36e20p-14", "0x1.17fp-24", "0x1.592p-25"), 0)],
}
COMMON_ROWS = [("zero", (0.0, 0.0, 0.0), 0), ("ordinary", (0.5, -2.0, 0.25), 1), ("1e-4 alone", (1e-4, 0.0, 0.0), None)]


def _mask_rows(T):
    rows = []
    for name, vals, want in MASK_ROWS[T] + COMMON_ROWS:
        v = np.array([_H(x) if isinstance(x, str) else x for x in vals], T)
        if isinstance(vals[0], str):
            assert all(float(u) == _H(x) for u, x in zip(v, vals)), name      # representable in T
            dots = {(a * a + b * b) + c * c for a, b, c in itertools.permutations([float(u) for u in v])}
            assert len(dots) == 1, name                                         # exact in any order
            dot = dots.pop()
            assert abs(dot - 1e-8) <= 2.0 ** -20 * 1e-8 and (float(T(dot)) > 1e-8) == bool(want), (name, dot)
            if "between" in name:
                assert dot > 1e-8 and float(T(dot)) < 1e-8
            if name == "equal":
                assert dot == 1e-8
        if want is None:
            want = int(float(sim.rdot(T, v, v)) > 1e-8)
        rows.append((name, v, want))
    return rows


@types
@cons
@batches
def test_hess_mask_at_the_threshold(built, B, p, f32):
    """hess_upd = dot(Fx, Fx) > 1e-8 with the dot product just above, equal to (Float64) and just below 1e-8; the state and neval stay"""
    T = F32 if f32 else F64
    rows = _mask_rows(T)
    H = _base(T, B, SHAPE_NM + (p,), seed=3)
    for b in range(B):
        H["Fx"][b] = np.roll(rows[b % len(rows)][1], b // len(rows) % 3)
    ctl = _ctl(B, p, seed=3)
    W, wctl = _check_ex(H, ctl, [("hess_mask",)])
    assert np.array_equal(wctl["neval"], ctl["neval"]) and (wctl["hess_upd"][B:] == 201).all()
    for b in range(B):
        assert wctl["hess_upd"][b] == rows[b % len(rows)][2], rows[b % len(rows)][0]
    for k in sim.ARRAYS:
        if H[k] is not None:
            assert _same_bits(W[k], H[k]).all(), k


# ---- NULL and an all-off block are the plain calls ---------------------------------------------------------------------------------------------

@types
@cons
@batches
def test_null_and_all_off_blocks_are_the_plain_calls(built, B, p, f32):
    """begin, trial_done, ls_test (first 1 and 0) and end: the `_ex` call with ctl = NULL, and with a block of always_accept = 0,
    max_iter = max_eval = -1, leave the state byte-equal to the plain call's (the all-off block still counts evaluations)"""
    T = F32 if f32 else F64
    for name, args in (("begin", ()), ("trial_done", ()), ("ls_test", (1,)), ("ls_test", (0,)), ("end", ())):
        H = _base(T, B, SHAPE_NM + (p,), seed=11, dmin=2.0 ** -6, max_inner=2, gammaA=0.25, eps2=2.0 ** -20)
        H["status"][:B] = np.arange(B) % 3 == 0
        plain = _Device(H)
        plain.call(name, *args)
        want = plain.download()
        want_sim = sim.copy_state(H)
        getattr(sim, name)(want_sim, *args)
        _compare(want, want_sim, B)
        for ctl in (None, _ctl(B, p, seed=11)):
            D = _DeviceEx(H, ctl)
            D.call_ex(name + "_ex", *args)
            got = D.download()
            for k in sim.ARRAYS:
                if H[k] is not None:
                    assert _same_bits(got[k], want[k]).all(), (name, args, "NULL" if ctl is None else "off", k)


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------

DEFAULT = dict(curvature=0.3, start=0.3, noise=0.01)
F3 = dict(curvature=1.5, start=1.0, noise=0.5)
ROUGH = dict(curvature=3.0, start=2.0, noise=0.5)
BL = 12
DECISIONS = ("iter", "nlinsolve", "nfact", "nbk", "neval")
EXACT = ("solution", "multipliers", "r", "objective", "normdual", "normprimal", "epstol", "iter", "nfact", "nlinsolve", "nbk", "neval")
_scalar = {}


def _mods():
    import torch
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import device_loop as DL, hipldl, synthetic as syn
    return torch, DL, hipldl, syn


def _family(p, kind, device="cuda:0", dtype=np.float64):
    torch, DL, hipldl, syn = _mods()
    return DL.BandQuadFamily(syn.band_structure(40, p), BL, seed=40 + p, torch=torch, device=device, dtype=dtype, **kind)


def _scalar_runs(fam, key, per_problem=None, **kw):
    """outer_loop.solve with the CPU oracle on a counting wrapper of each problem's host model (once per case); `per_problem(b)` gives
    keywords that differ by problem (start points)"""
    if key not in _scalar:
        from cannoles_jl_amd import outer_loop
        from oracle import oracle as O
        from tests.test_oracle_pinning import oracle_newton, oracle_solver
        out = []
        for b in range(BL):
            model = CountingModel(fam.host_model(b))
            one = outer_loop.solve(model, oracle_solver, oracle_newton, O.default_params(), **kw, **(per_problem(b) if per_problem else {}))
            one["neval"] = model.neval
            out.append(one)
        _scalar[key] = out
    return _scalar[key]


def _col(ones, k):
    return [o[k] for o in ones]


def _same_decisions(got, ones, tag):
    print(f"{tag}: device {got['status']}, " + ", ".join(f"{k} = {got[k].tolist()}" for k in DECISIONS))
    assert got["status"] == _col(ones, "status"), tag
    for k in DECISIONS:
        assert got[k].tolist() == _col(ones, k), (tag, k, got[k].tolist(), _col(ones, k))


def _device_and_packed(fam, tag, ones, **kw):
    """the device loop against the scalar runs, and compact = True, compact_min_finished = 1 bit-equal to it"""
    torch, DL, hipldl, syn = _mods()
    got = DL.solve_batch_device(fam, **kw)
    _same_decisions(got, ones, tag)
    packed = DL.solve_batch_device(fam, compact=True, compact_min_finished=1, **kw)
    for k in EXACT + (("hess_skipped",) if "hess_skipped" in got else ()):
        assert packed[k].dtype == got[k].dtype and np.array_equal(packed[k].view(np.uint8), got[k].view(np.uint8)), (tag, "compact", k)
    assert packed["status"] == got["status"] and packed["steps"] == got["steps"]
    return got, packed


def _close_solutions(got, ones, tag):
    """the tolerances of test_loop_rho_max_ends_exception"""
    for b in range(BL):
        assert np.allclose(got["solution"][b], ones[b]["solution"], atol=1e-7, rtol=1e-7), (tag, b)
        assert np.allclose(got["multipliers"][b], ones[b]["multipliers"], atol=1e-6, rtol=1e-6), (tag, b)
        assert abs(got["objective"][b] - ones[b]["objective"]) <= 1e-9 * max(1.0, ones[b]["objective"]), (tag, b)


def case_always_accept(p, device="cuda:0"):
    fam = _family(p, ROUGH, device)
    plain = _scalar_runs(fam, ("rough", p))
    ones = _scalar_runs(fam, ("rough always", p), always_accept_extrapolation=True)
    changed = [b for b in range(BL) if any(plain[b][k] != ones[b][k] for k in ("status",) + DECISIONS)]
    assert set(_col(ones, "status")) == {"first_order"} and changed == ([7, 8, 9] if p else [2, 6, 7]), changed
    assert not any(_col(ones, "nbk")) and any(_col(plain, "nbk"))   # an accepted extrapolation leaves nothing to search from
    if p:
        assert [(plain[b]["iter"], ones[b]["iter"]) for b in changed] == [(18, 16), (16, 26), (20, 26)]
    return fam, ones


@pytest.mark.parametrize("p", [4, 0])
def test_loop_always_accept_extrapolation(built, p):
    """rough family: with p = 4 problems 7, 8 and 9 change from the default (iter 16 / 26 / 26 against 18 / 16 / 20), with p = 0 problems
    2, 6 and 7; no problem backtracks any more"""
    fam, ones = case_always_accept(p)
    got, packed = _device_and_packed(fam, f"always_accept p = {p}", ones, always_accept_extrapolation=True)
    assert packed["compactions"] >= 1


def case_max_iter(device="cuda:0"):
    fam = _family(0, F3, device)
    plain = _scalar_runs(fam, ("F3", 0))
    assert _col(plain, "iter") == [11, 10, 13, 10, 7, 9, 7, 7, 9, 9, 14, 9]
    ones = _scalar_runs(fam, ("F3 max_iter", 0), max_iter=8)
    # an iteration count of 9 that ends first_order is first_order: max_iter stops the five problems that needed more than nine
    assert _col(ones, "status") == ["max_iter" if it > 9 else "first_order" for it in _col(plain, "iter")]
    assert all(o["iter"] == 9 for o in ones if o["status"] == "max_iter") and _col(ones, "status").count("max_iter") == 5
    return fam, ones


def test_loop_max_iter(built):
    """max_iter = 8 on the F3 family, p = 0: the scalar iteration counts are 11, 10, 13, 10, 7, 9, 7, 7, 9, 9, 14, 9, so the five problems
    above nine end `max_iter` with iter = 9 and the other seven first_order (three of them in their ninth iteration)"""
    fam, ones = case_max_iter()
    _device_and_packed(fam, "max_iter = 8", ones, max_iter=8)


def case_max_eval(which, device="cuda:0"):
    if which == 12:
        fam = _family(0, ROUGH, device)
        ones = _scalar_runs(fam, ("rough max_eval", 0), max_eval=12)
        st = _col(ones, "status")
        assert (st.count("first_order"), st.count("max_eval")) == (5, 7)
        assert all(st[b] == "max_eval" and ones[b]["nbk"] > 0 for b in (2, 7))
    else:
        fam = _family(4, F3, device)
        ones = _scalar_runs(fam, ("F3 max_eval", 4), max_eval=20)
        st = _col(ones, "status")
        assert (st.count("first_order"), st.count("max_eval")) == (7, 5)
    assert all(o["neval"] > which for o in ones if o["status"] == "max_eval")   # (a problem may also pass the limit and end first_order)
    return fam, ones


@pytest.mark.parametrize("which", [12, 20])
def test_loop_max_eval(built, which):
    """max_eval = 12, rough family, p = 0: five first_order and seven max_eval, problems 2 and 7 among the latter after backtracking;
    max_eval = 20, F3 family, p = 4 (two evaluations per point): seven first_order and five max_eval"""
    fam, ones = case_max_eval(which)
    _device_and_packed(fam, f"max_eval = {which}", ones, max_eval=which)


def test_loop_tiny_max_eval_ends_at_the_start(built):
    """max_eval = 0: `tired` holds after the start evaluation (src/CaNNOLeS.jl:559) — every problem ends max_eval without a global step"""
    torch, DL, hipldl, syn = _mods()
    fam = _family(4, DEFAULT)
    ones = _scalar_runs(fam, ("default max_eval 0", 4), max_eval=0)
    assert set(_col(ones, "status")) == {"max_eval"} and set(_col(ones, "iter")) == {0} and set(_col(ones, "neval")) == {2}
    got = DL.solve_batch_device(fam, max_eval=0)
    _same_decisions(got, ones, "max_eval = 0")
    assert got["steps"] == 0


def _raising(*a, **k):
    raise AssertionError("hess_vals called under Newton_noFHess")


def case_gauss_newton(p, device="cuda:0"):
    fam = _family(p, DEFAULT, device)
    ones = _scalar_runs(fam, ("default noFHess", p), method="Newton_noFHess")
    assert set(_col(ones, "status")) == {"first_order"} and set(_col(ones, "iter")) <= {3, 4}
    return fam, ones


@pytest.mark.parametrize("p", [0, 4])
def test_loop_gauss_newton(built, p):
    """method = Newton_noFHess on the default family: every problem first_order in 3-4 iterations, with a family whose hess_vals raises;
    the handle is built on the pattern without the H_F segment"""
    torch, DL, hipldl, syn = _mods()
    fam, ones = case_gauss_newton(p)
    fam.hess_vals = _raising
    got, _ = _device_and_packed(fam, f"Newton_noFHess p = {p}", ones, method="Newton_noFHess")
    _close_solutions(got, ones, "Newton_noFHess")
    del fam.hess_vals
    with pytest.raises(ValueError):
        DL.solve_batch_device(fam, method="LM")


def case_vanishing(p, device="cuda:0"):
    fam = _family(p, DEFAULT if p == 0 else dict(DEFAULT, noise=0.0), device)
    ones = _scalar_runs(fam, ("default vanishing", p), method="Newton_vanishing")
    assert set(_col(ones, "status")) == {"first_order"}
    assert _col(ones, "hess_skipped") == ([int(b in (5, 9, 10)) for b in range(BL)] if p == 0 else [1] * BL)
    return fam, ones


@pytest.mark.parametrize("p", [0, 4])
def test_loop_newton_vanishing(built, p):
    """method = Newton_vanishing on the default family: with p = 0 problems 5, 9 and 10 skip one H_F refresh, with p = 4 and noise = 0
    every problem skips one; hess_skipped as the scalar loop counts it, solutions to the tolerances of test_loop_rho_max_ends_exception"""
    fam, ones = case_vanishing(p)
    got, _ = _device_and_packed(fam, f"Newton_vanishing p = {p}", ones, method="Newton_vanishing")
    assert got["hess_skipped"].tolist() == _col(ones, "hess_skipped")
    _close_solutions(got, ones, "Newton_vanishing")


def case_start_point(device="cuda:0"):
    """start at the scalar solutions of the default run of the F3 family (p = 4), with those multipliers perturbed"""
    fam = _family(4, F3, device)
    first = _scalar_runs(fam, ("F3", 4))
    assert set(_col(first, "status")) == {"first_order"}
    X = np.stack(_col(first, "solution"))
    LAM = np.stack(_col(first, "multipliers")) * 1.5 + np.array([0.25, -0.5, 0.125, 1.0])
    ones = _scalar_runs(fam, ("F3 start", 4), per_problem=lambda b: dict(x=X[b], lam=LAM[b]), use_initial_multiplier=True)
    ignored = _scalar_runs(fam, ("F3 start, least-squares multipliers", 4), per_problem=lambda b: dict(x=X[b], lam=LAM[b]))
    # the perturbed multipliers are what keeps the loop going: from the least-squares multipliers at a solution it ends at once or after one step
    assert max(_col(ignored, "iter")) <= 1 and min(_col(ones, "iter")) >= 4 and set(_col(ones, "status")) == {"first_order"}
    return fam, ones, ignored, X, LAM


def test_loop_start_point_and_initial_multiplier(built):
    """x [B, n], lam [B, p], use_initial_multiplier: the decisions of the scalar loop per problem; without use_initial_multiplier `lam` is
    ignored: from the least-squares multipliers at a solution every problem ends at the start or after one iteration"""
    torch, DL, hipldl, syn = _mods()
    fam, ones, ignored, X, LAM = case_start_point()
    got, _ = _device_and_packed(fam, "x, lam, use_initial_multiplier", ones, x=X, lam=LAM, use_initial_multiplier=True)
    _close_solutions(got, ones, "start point")
    off = DL.solve_batch_device(fam, x=X, lam=LAM)
    _same_decisions(off, ignored, "x alone")
    assert off["steps"] <= 1
    for bad in (dict(x=X[:, :-1]), dict(x=X[:-1]), dict(lam=LAM[:, :-1], use_initial_multiplier=True)):
        with pytest.raises(ValueError):
            DL.solve_batch_device(fam, **bad)


def test_loop_max_time_zero_stops_after_one_step(built):
    """max_time = 0.0: one global step, then every unfinished problem has status max_time; what the step did is what max_steps = 1 does"""
    torch, DL, hipldl, syn = _mods()
    fam = _family(4, F3)
    one = DL.solve_batch_device(fam, max_steps=1)
    got = DL.solve_batch_device(fam, max_time=0.0)
    assert got["steps"] == 1 and "unknown" in one["status"]
    assert got["status"] == ["max_time" if s == "unknown" else s for s in one["status"]]
    for k in EXACT:
        assert np.array_equal(got[k], one[k]), k
    free = DL.solve_batch_device(fam, max_time=3600.0)
    assert "max_time" not in free["status"] and free["steps"] > 1


F32_CASES = {"max_iter": (0, F3, dict(max_iter=8)),
             "always_accept": (4, F3, dict(max_iter=8, always_accept_extrapolation=True)),
             "gauss_newton": (4, DEFAULT, dict(max_iter=8, method="Newton_noFHess")),
             "vanishing": (0, DEFAULT, dict(max_iter=8, method="Newton_vanishing")),
             "start_point": (4, DEFAULT, dict(max_iter=8, max_eval=1000, use_initial_multiplier=True))}


def _f32_keywords(fam, case, kw, idx=None):
    """the case's keywords for the problems `idx` of the family; start_point: x = x0 + 1/64 and multipliers 1/2, -1/4, ... per problem"""
    if case != "start_point":
        return kw
    idx = np.arange(BL) if idx is None else np.asarray(idx)
    x = (fam.h["x0"] + 2.0 ** -6).astype(np.float32)
    lam = (0.5 * (-0.5) ** np.arange(4)[None, :] * (1 + np.arange(BL)[:, None] % 3)).astype(np.float32)
    return dict(kw, x=x[idx], lam=lam[idx])


@pytest.mark.parametrize("case", list(F32_CASES))
def test_loop_float32(built, case):
    """dtype = float32: the keywords against sub-batches (each problem decides alone) and compact on / off; every problem ends
    first_order or max_iter within max_iter + 1 iterations.  Not compared with the Float64 scalar loop."""
    torch, DL, hipldl, syn = _mods()
    p, kind, kw = F32_CASES[case]
    fam = _family(p, kind, dtype=np.float32)
    got = DL.solve_batch_device(fam, **_f32_keywords(fam, case, kw))
    print(f"float32 {case}: {got['status']}, " + ", ".join(f"{k} = {got[k].tolist()}" for k in DECISIONS))
    assert got["dtype"] == "float32" and set(got["status"]) <= {"first_order", "max_iter"} and (got["iter"] <= kw["max_iter"] + 1).all()
    assert all(it == kw["max_iter"] + 1 for s, it in zip(got["status"], got["iter"]) if s == "max_iter")
    packed = DL.solve_batch_device(fam, compact=True, compact_min_finished=1, **_f32_keywords(fam, case, kw))
    for k in EXACT + (("hess_skipped",) if "hess_skipped" in got else ()):
        assert np.array_equal(packed[k].view(np.uint8), got[k].view(np.uint8)), (case, k)
    assert packed["status"] == got["status"] and packed["steps"] == got["steps"]
    eps32 = float(np.finfo(np.float32).eps)
    for idx in ([3], [0, 1, 2, 3, 4], [11, 6]):
        sub = DL.solve_batch_device(fam.take(idx), **_f32_keywords(fam, case, kw, idx))
        assert sub["status"] == [got["status"][b] for b in idx], idx
        for k in DECISIONS + (("hess_skipped",) if "hess_skipped" in got else ()):
            assert np.array_equal(sub[k], got[k][idx]), (idx, k)
        assert (np.abs(sub["solution"] - got["solution"][idx]) <= 16 * eps32 * np.maximum(1.0, np.abs(got["solution"][idx]))).all(), idx
