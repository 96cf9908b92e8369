"""The nine step kernels of csrc/outer_step.hip (cnl_outer_begin_dev ... cnl_outer_end_dev, and their `_f32_dev` twins) one by one against
the plain restatement tests/support/outer_step_sim.py, and the lockstep loop at statuses other than first_order.  -m gpu.

State.  Every member of the state is an array of its own, every second one starts one element off a 16-byte boundary, and every array has
EXTRA rows more than st.B, filled with a sentinel.  The inputs come from a seeded generator on the host; the device and the simulator get
copies of the same arrays.  Every array of the state — the rows of problems outside a kernel's mask and the rows >= st.B included, and
`flags` — is compared after the call.

Exact mode.  Every element array holds multiples of 2^-6 of magnitude <= 8: every sum of products of such values is exact in double in
any order, so the kernel's tree sum and the simulator's fsum round the same number to T once, and every other operation is one IEEE
operation in T on both sides (the kernels are compiled with fp contract off).  The comparison is bit for bit (two NaNs count as equal:
the payload of a NaN that an operation produces is not specified).  Division and square root: the library is built with hipcc's default
flags (csrc/Makefile: -O3, no fast-math option), under which -fhip-fp32-correctly-rounded-divide-sqrt is on, so the Float32 division
and sqrtf are correctly rounded, as the Float64 ones always are; no 1-ulp allowance is made for them.

Random mode.  Normally distributed element arrays.  A reduction's value output is compared with the simulator's within the bound of a
sum of K products in any order, K eps(double) sum|terms| + eps(T)/2 |sum| (the second term is absent for Float64); every threshold a
decision compares a reduction with is placed, after the sums are known on the host, at least 1000 times that bound away (asserted for
every row), so masks, counters, flags and statuses are compared exactly, and so is everything that is not a reduction's output."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests.support import outer_step_sim as sim

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
EXTRA = 3
SHAPES = [(1, 1, 0), (5, 7, 2), (64, 65, 1), (255, 257, 3), (600, 256, 300)]
BP = 9                                  # problems of a per-problem kernel's batch (one workgroup each)
THREAD_B = [1, 255, 256, 257, 300]      # begin / end: one thread per problem in blocks of 256
EPS64 = float(np.finfo(F64).eps)

types = pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
shapes = pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-m%d-p%d" % s)
layouts = pytest.mark.parametrize("nnzjF,share", [(1, True), (257, False), (257, True), (1, False)], ids=["jF1-aliased", "jF257-distinct", "jF257-aliased", "jF1-distinct"])


# ---- the state on the device ---------------------------------------------------------------------------------------------------------------

class _Device:
    """a device copy of the host state H: one buffer per array, every second one starting one element off a 16-byte boundary"""

    def __init__(self, H):
        import torch
        from cannoles_jl_amd import hipldl
        self.torch, self.hipldl, self.H = torch, hipldl, H
        self.dev = torch.device("cuda", 0)
        self.f32 = H["T"] is F32
        st = hipldl.cnl_outer_state_f32() if self.f32 else hipldl.cnl_outer_state()
        for k in sim.SIZES:
            setattr(st, k, int(H[k]))
        for k in sim.ELEM_SCALARS:
            setattr(st, k, float(H[k]))
        self.keep = {}
        for idx, k in enumerate(sim.ARRAYS):
            a = H[k]
            if a is None:
                setattr(st, k, None)
                continue
            if k == "Jct" and H["Jct"] is H["Jcv"]:
                self.keep[k] = self.keep["Jcv"]
            else:
                flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy())
                buf = torch.zeros(flat.numel() + 1, dtype=flat.dtype, device=self.dev)
                self.keep[k] = buf[idx % 2:idx % 2 + flat.numel()]
                self.keep[k].copy_(flat)
                assert self.keep[k].data_ptr() % 16 == (idx % 2) * flat.element_size()
            setattr(st, k, self.keep[k].data_ptr())
        self.st = st
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def call(self, name, *args):
        fn = getattr(self.hipldl.lib(), "cnl_outer_" + name + ("_f32_dev" if self.f32 else "_dev"))
        self.hipldl._check(fn(C.byref(self.st), *args, self.stream))

    def read(self, k):
        self.torch.cuda.synchronize(self.dev)
        return self.keep[k].cpu().numpy().reshape(self.H[k].shape)

    def download(self):
        return {k: self.read(k) for k in self.keep}


def _device_run(H, calls):
    D = _Device(H)
    for name, *args in calls:
        D.call(name, *args)
    return D.download()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return np.zeros(1, bool)
    if a.dtype.kind == "f":
        u = "u%d" % a.itemsize
        return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))
    return a == b


def _compare(got, want, B, only_rows=None, approx=None):
    """every array bit for bit in every row; `only_rows`: {array: row mask} for the arrays compared on some rows only (always with the
    rows >= B); `approx`: {array: per-row bound} for a reduction's value output (random mode), rows >= B still exact"""
    only_rows, approx = only_rows or {}, approx or {}
    for k in sim.ARRAYS:
        if want[k] is None:
            continue
        g, w = got[k], want[k]
        rows = np.ones(len(w), bool)
        if k in only_rows:
            rows = np.asarray(only_rows[k], bool).copy()
            rows[B:] = True
        if k in approx:
            diff = np.abs(g[:B].astype(np.float64) - w[:B].astype(np.float64))
            ok = (diff <= approx[k]) | _same_bits(g[:B], w[:B])
            assert ok[rows[:B]].all(), (k, np.flatnonzero(~ok & rows[:B])[:8].tolist(), diff[~ok][:4], np.asarray(approx[k])[~ok][:4])
            rows[:B] = False
        same = _same_bits(g, w)
        same = same.reshape(len(w), -1).all(axis=1) if k != "flags" else same
        if k == "flags":
            assert same.all(), (k, g.tolist(), w.tolist())
        else:
            bad = np.flatnonzero(~same & rows)
            assert bad.size == 0, (k, "rows", bad[:8].tolist(), "got", g[bad[:2]].tolist()[:2], "want", w[bad[:2]].tolist()[:2])


def _check(H, calls, only_rows=None, approx=None):
    """the kernels of `calls` on a device copy of H against the simulator on another copy; returns the simulator's state"""
    want = sim.copy_state(H)
    for name, *args in calls:
        getattr(sim, name)(want, *args)
    got = _device_run(H, calls)
    _compare(got, want, H["B"], only_rows, approx)
    return want


# ---- host states ---------------------------------------------------------------------------------------------------------------------------

def _base(T, B, shape, nnzjF=11, share=False, seed=0, normal=False, **scalars):
    """a state of B problems in B + EXTRA rows: element arrays on the 2^-6 grid (or normal), per-problem element scalars positive on the
    grid, masks and counters anything; the extra rows hold sentinels"""
    n, m, p = shape
    rng = np.random.default_rng([seed, B, n, m, p, nnzjF, int(T is F32)])
    S = sim.new_state(T, B, n, m, p, nnzjF=nnzjF, rows=B + EXTRA, share_jc=share, **scalars)
    for k in sim.ARRAYS:
        a = S[k]
        if a is None or (k == "Jct" and share):
            continue
        if k == "flags":
            a[:] = rng.integers(0, 2, 8)     # stale words of an earlier step
        elif k in sim.MASKS:
            a[:B], a[B:] = rng.integers(0, 2, B), 201
        elif k in sim.INT32 or k in sim.INT64:
            a[:B], a[B:] = rng.integers(0, 5, B), -9
        elif k in sim.ROW_ARRAYS:
            a[:B] = rng.normal(size=a[:B].shape) if normal else rng.integers(-512, 513, a[:B].shape) / 64.0
            a[B:] = -123.5
        else:
            a[:B], a[B:] = rng.integers(1, 513, B) / 64.0, -123.5
    return S


def _batches(K, B):
    """scenario of problem b in batch j = (j B + b) mod K: neighbours differ, and there are as many batches as it takes for every scenario
    to occur"""
    out = [[(j * B + b) % K for b in range(B)] for j in range(-(-K // B))]
    assert set(itertools.chain(*out)) == set(range(K))
    return out


def _put(S, b, over):
    for k, v in over.items():
        S[k][b] = v


def _expect(W, b, want, tag):
    for k, v in want.items():
        g = W[k][b]
        if isinstance(v, float) and v != v:
            assert g != g, (tag, k)
        else:
            assert np.all(g == v), (tag, k, g, v)


# ---- begin, end: one thread per problem ----------------------------------------------------------------------------------------------------

def _begin_scenarios(T):
    """status x phase0 x inner, and the four regimes of delta = max(min(delta_dec delta, combined), dmin) with delta_dec = T(0.1),
    dmin = 2^-6: 0 the product (T(0.1) 4 below combined = 3), 1 combined (2^-5), 2 the floor, 3 NaN from normdual"""
    regimes = [dict(delta=4.0, normdual=2.0, normprimal=1.0), dict(delta=4.0, normdual=2.0 ** -6, normprimal=2.0 ** -6),
               dict(delta=2.0 ** -6, normdual=2.0, normprimal=1.0), dict(delta=4.0, normdual=np.nan, normprimal=1.0)]
    results = [T(0.1) * T(4), T(2.0 ** -5), T(2.0 ** -6), float("nan")]
    sc = [dict(status=s, phase0=f, inner=i) for s, f, i in itertools.product((0, 1), (0, 1), (0, 1, 2))]
    sc += [dict(status=0, phase0=1, inner=i % 3) for i in range(4)]
    out = []
    for i, s in enumerate(sc):
        r = i % 4
        so = s["status"] == 0 and s["phase0"] == 1
        inner = 0 if so else s["inner"]
        act = s["status"] == 0
        want = dict(act=act, need=act and inner != 1, brk=0, inner=inner, phase0=0 if so else s["phase0"],
                    delta=results[r] if so else regimes[r]["delta"])
        if so and r != 3:
            want.update(combined=T(regimes[r]["normdual"]) + T(regimes[r]["normprimal"]), combined_hat=np.inf, ndh=regimes[r]["normdual"])
        out.append((dict(s, **regimes[r]), want))
    return out


@types
@pytest.mark.parametrize("p", [2, 0])
@pytest.mark.parametrize("B", THREAD_B)
def test_begin_every_branch_and_the_second_workgroup(built, B, p, f32):
    """cnl_outer_begin_dev on B problems (B + 3 rows), exact mode: status 0 / 1, phase0 0 / 1, inner 0 / 1 / 2, the regimes of the delta
    rule (NaN propagating from normdual included) — every array of the state bit for bit, the four flag words as the simulator has them
    (all eight words are zeroed first); one batch without an active problem leaves all flags 0"""
    T = F32 if f32 else F64
    scen = _begin_scenarios(T)
    seen = set()
    for j, assign in enumerate(_batches(len(scen), B)):
        H = _base(T, B, (5, 7, p), seed=j, dmin=2.0 ** -6)
        for b, s in enumerate(assign):
            _put(H, b, scen[s][0])
        W = _check(H, [("begin",)])
        for b, s in enumerate(assign):
            _expect(W, b, scen[s][1], ("begin", s))
            seen.add(s)
        act, inner = W["act"][:B] != 0, W["inner"][:B]
        assert W["flags"].tolist() == [act.any(), (W["need"][:B] != 0).any(), (act & (inner == 0)).any(), (act & (inner > 0)).any(), 0, 0, 0, 0]
    assert seen == set(range(len(scen)))
    H = _base(T, B, (5, 7, p), seed=99, dmin=2.0 ** -6)
    H["status"][:B] = 1 + np.arange(B) % 5
    H["flags"][:] = 1
    W = _check(H, [("begin",)])
    assert not W["flags"].any() and not W["act"][:B].any() and not W["need"][:B].any()


def _end_scenarios():
    """first_order x small_res x brk x tired with done_in, and four states without: normdual = 4, normprimal = 1/2, sum |lam| / p <= 8 <
    smax (ds = 1): epstol = 4 is first_order at equality, one ulp less is not"""
    sc = [dict(done_in=1, fo=c >> 3 & 1, small_res=c >> 2 & 1, brk=c >> 1 & 1, tired=c & 1) for c in range(16)]
    sc += [dict(done_in=0, fo=c >> 1 & 1, small_res=1, brk=c & 1, tired=1) for c in range(4)]
    return sc


@types
@pytest.mark.parametrize("p", [2, 0])
@pytest.mark.parametrize("B", THREAD_B)
def test_end_status_chain_and_the_second_workgroup(built, B, p, f32):
    """cnl_outer_end_dev, exact mode: all 16 combinations of first_order, small_res, brk and tired with done_in — status 1 > 2 > 3 > 5 > 0,
    it + 1, phase0 = 1 — and done_in = 0, where nothing moves; every array bit for bit"""
    T = F32 if f32 else F64
    scen = _end_scenarios()
    seen = set()
    for j, assign in enumerate(_batches(len(scen), B)):
        H = _base(T, B, (5, 7, p), seed=j)
        H["status"][:B], H["normdual"][:B], H["normprimal"][:B] = 0, 4.0, 0.5
        for b, s in enumerate(assign):
            sc = scen[s]
            _put(H, b, dict(done_in=sc["done_in"], small_res=sc["small_res"], brk=sc["brk"], tired=sc["tired"],
                            epstol=T(4) if sc["fo"] else np.nextafter(T(4), T(0))))
        W = _check(H, [("end",)])
        for b, s in enumerate(assign):
            sc = scen[s]
            status = 1 if sc["fo"] else 2 if sc["small_res"] else 3 if sc["brk"] else 5 if sc["tired"] else 0
            _expect(W, b, dict(status=status, it=H["it"][b] + 1, phase0=1) if sc["done_in"] else dict(status=0, it=H["it"][b], phase0=H["phase0"][b]),
                    ("end", s))
            seen.add(s)
    assert seen == set(range(len(scen)))


# ---- newton_done -----------------------------------------------------------------------------------------------------------------------------

def _newton_scenarios(T):
    """(name, inputs, broken with did_newton = 1, eps_k where ext); defaults: active, a Newton system was due, inner = 0, the system fine,
    delta = 1, eps_k = 1000"""
    up = np.nextafter(T(1e10), T(np.inf))
    hi, lo = (T(1e60), np.nextafter(T(1e60), T(0))) if T is F64 else (T(np.inf), T(3e38))
    return [("extrapolation, eps_k at 99 e / 100", {}, 0, 990.0),
            ("line search", dict(inner=2), 0, None),
            ("no Newton system", dict(need=0, inner=1), 0, None),
            ("rho_new one ulp above rhomax", dict(rho_new=up), 1, None),
            ("rho_new equal to rhomax", dict(rho_new=T(1e10)), 0, 990.0),
            ("ok_new = 0", dict(ok_new=0), 1, None),
            ("inf at the last index of d_new", dict(d_last=np.inf), 1, None),
            ("NaN at index 0 of d_new", dict(d_first=np.nan), 1, None),
            ("fx huge", dict(fx=hi), 1, None),
            ("fx just not huge", dict(fx=lo), 0, 990.0),
            ("non-finite d_new, no Newton system due", dict(need=0, inner=1, d_first=np.nan, d_last=np.inf), 0, None),
            ("finished", dict(act=0, need=0), 0, None),
            ("eps_k at 9 e / 10", dict(delta=0.5), 0, 900.0),
            ("eps_k at 1e3 delta", dict(delta=0.9375), 0, 937.5),
            ("broken in a line-search iteration", dict(inner=3, ok_new=0), 1, None)]


def _newton_state(T, shape, nnzjF, share, seed, assign, scen):
    B = len(assign)
    H = _base(T, B, shape, nnzjF=nnzjF, share=share, seed=seed, rhomax=1e10)
    H["act"][:B], H["need"][:B], H["inner"][:B], H["ok_new"][:B], H["delta"][:B], H["epsk"][:B] = 1, 1, 0, 1, 1.0, 1000.0
    for b, s in enumerate(assign):
        over = dict(scen[s][1])
        if "d_last" in over:
            H["d_new"][b, -1] = over.pop("d_last")
        if "d_first" in over:
            H["d_new"][b, 0] = over.pop("d_first")
        _put(H, b, over)
    return H


@types
@layouts
@shapes
def test_newton_done_every_cause_of_broken(built, shape, nnzjF, share, f32):
    """cnl_outer_newton_done_dev, exact mode, did_newton 1 and 0: each cause of `broken` alone (and its boundary: rho_new == rhomax and fx
    just below T(1e60) do not break), the counters, rho_old and d where need, act cleared; a non-finite d_new does not break a problem
    without `need`; ext / lsm by inner; the three regimes of the eps_k clamp; lam_ls = lam - c / delta (lam for p == 0), and one call with
    lam_ls = NULL — every array bit for bit"""
    T = F32 if f32 else F64
    scen = _newton_scenarios(T)
    seen = set()
    for j, assign in enumerate(_batches(len(scen), BP)):
        for did in (1, 0):
            H = _newton_state(T, shape, nnzjF, share, j, assign, scen)
            W = _check(H, [("newton_done", did)])
            for b, s in enumerate(assign):
                name, over, brk, epsk = scen[s]
                need, act0, inner = over.get("need", 1), over.get("act", 1), over.get("inner", 0)
                brk = brk if did else H["brk"][b]
                act = act0 and not (did and brk)
                took = did and need
                if act and inner == 0:
                    epsk = {1.0: 990.0, 0.5: 900.0, 0.9375: 937.5}[over.get("delta", 1.0)]
                _expect(W, b, dict(brk=brk, act=act, ext=act and inner == 0, lsm=act and inner > 0, nlin=H["nlin"][b] + (1 if took else 0),
                                   nfact=H["nfact"][b] + (H["nf_new"][b] if took else 0), rho_old=H["ro_tmp"][b] if took else H["rho_old"][b],
                                   epsk=epsk if act and inner == 0 else 1000.0), (name, did))
                assert _same_bits(W["d"][b], H["d_new"][b] if took else H["d"][b]).all(), name
                seen.add(s)
    assert seen == set(range(len(scen)))
    H = _newton_state(T, shape, nnzjF, share, 7, _batches(len(scen), BP)[0], scen)
    H["lam_ls"] = None
    _check(H, [("newton_done", 1)])


# ---- the masked copies and the backtracking step -------------------------------------------------------------------------------------------------

@types
@layouts
@shapes
def test_extrapolated_ls_take_and_ls_step_on_masked_rows(built, shape, nnzjF, share, f32):
    """cnl_outer_extrapolated_dev (where ext), cnl_outer_ls_take_dev (where lsm), cnl_outer_ls_step_dev (where bt: alpha / 4, xl = x +
    alpha dx, nbk + 1), exact mode, on batches whose masks alternate — every array bit for bit, the rows outside the mask untouched"""
    T = F32 if f32 else F64
    for name, mask in (("extrapolated", "ext"), ("ls_take", "lsm"), ("ls_step", "bt")):
        for phase in (0, 1):
            H = _base(T, BP, shape, nnzjF=nnzjF, share=share, seed=phase)
            H[mask][:BP] = (np.arange(BP) + phase) % 2
            W = _check(H, [(name,)])
            on = H[mask][:BP] != 0
            assert on.any() and not on.all()
            if name == "ls_step":
                assert (W["alpha"][:BP][on] == H["alpha"][:BP][on] / T(4)).all() and (W["nbk"][:BP] == H["nbk"][:BP] + on).all()
            if name == "extrapolated":
                assert _same_bits(W["xt"][:BP][on], H["xt_e"][:BP][on]).all() and _same_bits(W["lamt"][:BP][~on], H["lamt"][:BP][~on]).all()
            if name == "ls_take":
                assert _same_bits(W["rt"][:BP][on], H["Fl"][:BP][on]).all() and _same_bits(W["lamt"][:BP][on], H["lam_ls"][:BP][on]).all()


# ---- trial_done -----------------------------------------------------------------------------------------------------------------------------

def _trial_scenarios(T, p):
    """(name, inputs, expected).  Defaults: active, not broken, inner = 0, combined = 8, eps_k = 1 (threshold thr = T(0.99) 8 + 1), the
    measures at the trial point (1, 1/2) — good —, normdual = normprimal = 2, delta = 1, never first_order, never small_residual;
    state scalars smax = 2, max_inner = 5, dmin = 2^-6"""
    up, dn = (lambda v: np.nextafter(T(v), T(np.inf))), (lambda v: np.nextafter(T(v), T(-np.inf)))
    thr = T(0.99) * T(8) + T(1)
    thr_d = T(0.99) * T(2) + T(1) / T(2)     # dr: ndh <= T(0.99) normdual + epsk / 2 and nph > T(0.99) normprimal + epsk / 2
    sc = []
    for act, brk, inner, good in itertools.product((1, 0), (0, 1), (0, 2), (1, 0)):
        nrm = (1.0, 0.5) if good else (64.0, 8.0)
        # (not active: the old combined_hat stands in `good`, which then reaches nothing: rej and done_in need act or brk)
        want = dict(inner=inner + act, rej=act and not good, done_in=(act and good) or brk, tired=0, chk=0)
        sc.append((f"table act={act} brk={brk} inner={inner} good={good}", dict(act=act, brk=brk, inner=inner, nrm_t=nrm, combined_hat=1.0 if good else 64.0), want))
    sc += [("good at equality", dict(nrm_t=(thr, 0.0)), dict(done_in=1, rej=0)),
           ("one ulp above the threshold", dict(nrm_t=(up(thr), 0.0)), dict(done_in=0, rej=1)),
           ("one ulp below the threshold", dict(nrm_t=(dn(thr), 0.0)), dict(done_in=1, rej=0)),
           ("delta / 10 at both edges", dict(inner=2, nrm_t=(thr_d, up(thr_d))), dict(delta=T(1) / T(10) if p else 1.0)),
           ("no delta / 10: dual measure one ulp too large", dict(inner=2, nrm_t=(up(thr_d), 4.0)), dict(delta=1.0)),
           ("no delta / 10: primal measure at its threshold", dict(inner=2, nrm_t=(thr_d, thr_d)), dict(delta=1.0)),
           ("no delta / 10 in the extrapolation iteration", dict(inner=0, nrm_t=(thr_d, up(thr_d))), dict(delta=1.0)),
           ("delta / 10 below dmin", dict(inner=2, delta=2.0 ** -4, nrm_t=(thr_d, 4.0)), dict(delta=2.0 ** -6 if p else 2.0 ** -4)),
           ("inner reaches max_inner", dict(inner=4, nrm_t=(64.0, 8.0)), dict(inner=5, tired=0, done_in=0, rej=1)),
           ("inner reaches max_inner + 1", dict(inner=5, nrm_t=(64.0, 8.0)), dict(inner=6, tired=1, done_in=1, rej=1)),
           ("small_res, not first_order", dict(epsF=1e6, epsc=1e6), dict(small_res=1, chk=1, done_in=1)),
           ("small_res and first_order", dict(epsF=1e6, epsc=1e6, epstol=1e6), dict(small_res=1, chk=0, done_in=1)),
           ("small_res, the iteration goes on", dict(epsF=1e6, epsc=1e6, nrm_t=(64.0, 8.0)), dict(small_res=1, chk=0, done_in=0)),
           ("sum |lam| / p above smax: ds = 4", dict(epsF=1e6, epsc=1e6, nrm_t=(4.0, 0.5), epstol=1.5, lam=8.0, lamt=8.0), dict(chk=0 if p else 1)),
           ("sum |lam| / p below smax: ds = 1", dict(epsF=1e6, epsc=1e6, nrm_t=(4.0, 0.5), epstol=1.5, lam=1.0, lamt=1.0), dict(chk=1)),
           ("epstol = NaN", dict(epsF=1e6, epsc=1e6, epstol=np.nan), dict(small_res=1, chk=1))]
    return sc


def _trial_state(T, shape, nnzjF, share, seed, assign, scen, normal=False):
    B = len(assign)
    H = _base(T, B, shape, nnzjF=nnzjF, share=share, seed=seed, normal=normal, smax=2.0, max_inner=5, dmin=2.0 ** -6)
    H["act"][:B], H["brk"][:B], H["inner"][:B], H["combined"][:B], H["epsk"][:B], H["delta"][:B] = 1, 0, 0, 8.0, 1.0, 1.0
    H["nrm_t"][:B], H["normdual"][:B], H["normprimal"][:B], H["epstol"][:B], H["epsF"][:B], H["epsc"][:B] = (1.0, 0.5), 2.0, 2.0, -1.0, -1.0, -1.0
    for b, s in enumerate(assign):
        _put(H, b, scen[s][1])
    return H


def _trial_expect(H, W, assign, scen, seen):
    for b, s in enumerate(assign):
        name, over, want = scen[s]
        _expect(W, b, want, name)
        act, inner0 = over.get("act", 1), over.get("inner", 0)
        acc_state, acc_lam = act and (inner0 > 0 or not W["rej"][b]), act and not W["rej"][b]
        assert _same_bits(W["x"][b], H["xt"][b] if acc_state else H["x"][b]).all() and _same_bits(W["Jv"][b], H["Jt"][b] if acc_state else H["Jv"][b]).all(), name
        assert _same_bits(W["lam"][b], H["lamt"][b] if acc_lam else H["lam"][b]).all(), name
        assert _same_bits(W["rhs_cur"][b], H["rhs_t"][b] if act else H["rhs_cur"][b]).all(), name
        seen.add(s)


@types
@layouts
@shapes
def test_trial_done_acceptance_table_thresholds_and_end_of_inner_loop(built, shape, nnzjF, share, f32):
    """cnl_outer_trial_done_dev, exact mode: act x brk x (inner0 == 0 or > 0) x good; good at the threshold chat == T(0.99) combined + epsk
    (computed in T on the host), one ulp above, one ulp below; the delta / 10 rule at its edges and at the dmin floor; inner reaching
    max_inner and max_inner + 1; small_res with and without first_order (chk, flags[5]); p == 0 (ds = 1, no delta rule); sum |lam| / p
    above and below smax; epstol = NaN — every array bit for bit (Jcv / Jct aliased and distinct)"""
    T = F32 if f32 else F64
    scen = _trial_scenarios(T, shape[2])
    seen = set()
    for j, assign in enumerate(_batches(len(scen), BP)):
        H = _trial_state(T, shape, nnzjF, share, j, assign, scen)
        W = _check(H, [("trial_done",)])
        _trial_expect(H, W, assign, scen, seen)
        assert W["flags"][4] == max(H["flags"][4], W["rej"][:BP].any()) and W["flags"][5] == max(H["flags"][5], W["chk"][:BP].any())
    assert seen == set(range(len(scen)))


# ---- the line search ---------------------------------------------------------------------------------------------------------------------------

@types
@layouts
@shapes
def test_ls_begin(built, shape, nnzjF, share, f32):
    """cnl_outer_ls_begin_dev, exact mode: Dphi = g'dx, eta = 1 / delta on the lsm rows only (p > 0), phi(x), alpha = 1, xl = x + dx.  The
    kernel writes xl, alpha, Dphi and phix for every problem; the header describes them as line-search work arrays of the lsm problems,
    so these four are compared on the lsm rows only (and on the rows >= B); everything else in every row"""
    T = F32 if f32 else F64
    for phase in (0, 1):
        H = _base(T, BP, shape, nnzjF=nnzjF, share=share, seed=phase)
        H["lsm"][:BP] = (np.arange(BP) + phase) % 2
        H["delta"][:BP] = 2.0 ** -(np.arange(BP) % 3 + 1)
        lsm = H["lsm"] != 0
        lsm[BP:] = False
        W = _check(H, [("ls_begin",)], only_rows={k: lsm for k in ("xl", "alpha", "Dphi", "phix")})
        on = lsm[:BP]
        assert (W["alpha"][:BP][on] == 1).all()
        assert (W["eta"][:BP] == np.where(on & (shape[2] > 0), T(1) / H["delta"][:BP], H["eta"][:BP])).all()


def _phix_for(target, t):
    """phix with phix + t == target in T, None if rounding leaves none"""
    T = type(target)
    c = target - t
    for v in (c, np.nextafter(c, T(np.inf)), np.nextafter(c, T(-np.inf))):
        if v + t == target:
            return v
    return None


def _ls_test_state(T, shape, nnzjF, share, seed, assign, normal=False):
    """scenarios of the Armijo test phi(xl) <= phix + gammaA alpha Dphi with gammaA = 1/4, eps2 = 2^-20, eta = 2:
    (lsm, bt, alpha, Dphi sign, phix relative to the threshold) -> bt after the first test, bt after a later round"""
    B = len(assign)
    H = _base(T, B, shape, nnzjF=nnzjF, share=share, seed=seed, normal=normal, gammaA=0.25, eps2=2.0 ** -20)
    H["eta"][:B] = 2.0
    e2 = 2.0 ** -20
    scen = [("not a candidate", 0, 0, 1.0, -1, "fail", 0, 0), ("satisfied at equality", 1, 1, 0.5, -1, "equal", 0, 0),
            ("failed by one ulp", 1, 1, 0.5, -1, "ulp", 1, 1), ("clearly satisfied", 1, 1, 1.0, -1, "pass", 0, 0),
            ("failed, alpha above eps2", 1, 1, 2.0 ** -10, -1, "fail", 1, 1), ("failed, alpha at eps2", 1, 1, e2, -1, "fail", 1, 1),
            ("failed, alpha below eps2", 1, 1, e2 / 2, -1, "fail", 1, 0), ("Dphi > 0", 1, 1, 1.0, 1, "fail", 1, 1),
            ("Dphi > 0, alpha below eps2", 1, 1, e2 / 4, 1, "fail", 1, 0), ("in lsm, not backtracking", 1, 0, 1.0, -1, "fail", 1, 0),
            ("backtracking, not in lsm", 0, 1, 1.0, -1, "fail", 0, 1)]
    want = []
    with np.errstate(all="ignore"):
        for b, s in enumerate(assign):
            name, lsm, bt, alpha, sign, kind, w1, w0 = scen[s]
            Dphi = T(sign) * abs(H["Dphi"][b])
            phil = sim.merit(H, b, H["Fl"], H["cl"], H["eta"][b])
            t = H["gammaA"] * T(alpha) * Dphi
            big = abs(phil) + abs(t) + T(1)
            if kind in ("equal", "ulp"):
                target = phil if kind == "equal" else np.nextafter(phil, T(-np.inf))
                phix = _phix_for(target, t)
                if phix is None:     # no phix + t lands on the target: the threshold itself, without the product
                    Dphi, phix = T(0), target
            else:
                phix = phil - t + (big if kind == "pass" else -big)
            _put(H, b, dict(lsm=lsm, bt=bt, alpha=alpha, Dphi=Dphi, phix=phix))
            want.append((name, w1, w0, phil, big))
    return H, want, len(scen)


N_LS_SCEN = 11


@types
@layouts
@shapes
def test_ls_test_armijo_at_equality_and_the_eps2_stop(built, shape, nnzjF, share, f32):
    """cnl_outer_ls_test_dev, exact mode, first = 1 and first = 0: satisfied at equality and failed by one ulp; alpha at, below and above
    eps2 in a backtracking round (the first test does not look at alpha); Dphi > 0; the candidates are lsm (first) or bt (later), a
    problem that is not a candidate keeps everything but bt = 0 at the first test; flags[6] zeroed first — every array bit for bit"""
    T = F32 if f32 else F64
    seen = set()
    for j, assign in enumerate(_batches(N_LS_SCEN, BP)):
        H, want, K = _ls_test_state(T, shape, nnzjF, share, j, assign)
        assert K == N_LS_SCEN
        for first in (1, 0):
            W = _check(H, [("ls_test", first)])
            for b, (name, w1, w0, _, _) in enumerate(want):
                assert W["bt"][b] == (w1 if first else w0), (name, first)
            assert W["flags"][6] == W["bt"][:BP].any()
        seen.update(assign)
    assert seen == set(range(N_LS_SCEN))


@types
def test_whole_backtracking_sequence_stops_at_eps2(built, f32):
    """Dphi > 0: the Armijo test can never be satisfied, and the rounds ls_step / ls_test(0) must end through alpha < eps2 = eps(T)^2:
    alpha = 4^-k falls below it after 53 steps in Float64 and 24 in Float32.  nbk, alpha and the whole state against the simulator."""
    T = F32 if f32 else F64
    H = _base(T, 3, (5, 7, 2), seed=5)
    H["lsm"][:3], H["bt"][:3], H["alpha"][:3], H["nbk"][:3] = [0, 1, 0], 0, 1.0, [3, 4, 5]
    H["Dphi"][1], H["phix"][1] = 1.0, sim.merit(H, 1, H["Fl"], H["cl"], H["eta"][1]) - T(64)
    D = _Device(H)
    W = sim.copy_state(H)
    D.call("ls_test", 1)
    sim.ls_test(W, 1)
    rounds = 0
    while D.read("flags")[6]:
        assert W["flags"][6] == 1 and rounds < 200, rounds
        D.call("ls_step")
        D.call("ls_test", 0)
        sim.ls_step(W)
        sim.ls_test(W, 0)
        rounds += 1
    assert W["flags"][6] == 0
    got = D.download()
    _compare(got, W, 3)
    steps = 24 if f32 else 53
    assert rounds == steps and got["nbk"][:3].tolist() == [3, 4 + steps, 5] and got["alpha"][1] == T(4.0) ** -steps and got["alpha"][1] < H["eps2"]


# ---- random mode: the reductions on ordinary numbers -------------------------------------------------------------------------------------------

def _sum_bound(T, terms):
    """a sum of K products in any order, accumulated in double and rounded to T once: K eps(double) sum |terms| + eps(T)/2 |sum|"""
    terms = np.asarray(terms, np.float64)
    return len(terms) * EPS64 * np.abs(terms).sum() + (float(np.finfo(F32).eps) / 2 * abs(terms.sum()) if T is F32 else 0.0)


def _rel_bound(T, K):
    """relative form for a sum of K non-negative terms, with room for three more operations in T behind it (a scaling, a division or a
    square root, each correctly rounded, none with a condition number above 1)"""
    return K * EPS64 + (float(np.finfo(F32).eps) / 2 if T is F32 else 0.0) + 3 * float(np.finfo(T).eps)


def _wide(a):
    return np.asarray(a, np.float64)


@types
@shapes
def test_random_trial_done(built, shape, f32):
    """random mode: fx = |Ft|^2 / 2 within the bound; epsF, epsc and epstol are set a factor 2 above or below 2 sqrt(fx), sqrt(sum c^2) and
    max(normdual / ds, normprimal) of each row after the simulator has the sums (margin: half the value, asserted against 1000 x the
    bound), so small_res, chk, flags and everything else is compared exactly"""
    T = F32 if f32 else F64
    n, m, p = shape
    scen = _trial_scenarios(T, p)[:16]
    for j, assign in enumerate(_batches(len(scen), BP)):
        H = _trial_state(T, shape, 257, False, j, assign, scen, normal=True)
        pre = sim.copy_state(H)
        sim.trial_done(pre)
        with np.errstate(all="ignore"):
            for b in range(BP):
                v1, v2 = T(2) * np.sqrt(pre["fx"][b]), np.sqrt(sim.rsum(T, [float(v) ** 2 for v in pre["cx"][b, :p]]))
                meas = sim.tmax(pre["normdual"][b] / sim.dual_scaling(pre, b), pre["normprimal"][b])
                H["epsF"][b], H["epsc"][b], H["epstol"][b] = v1 * T(2 if b & 1 else 0.5), v2 * T(2 if b & 2 else 0.5), meas * T(2 if b & 4 else 0.5)
                for v, thr, K in ((v1, H["epsF"][b], m), (v2, H["epsc"][b], max(p, 1)), (meas, H["epstol"][b], max(p, 1))):
                    assert abs(float(v) - float(thr)) >= 1000 * _rel_bound(T, K) * abs(float(v)), (b, v, thr)
        acc = (pre["act"][:BP] != 0) & ((H["inner"][:BP] > 0) | (pre["rej"][:BP] == 0))
        bound = np.array([0.5 * _sum_bound(T, _wide(H["Ft"][b, :m]) ** 2) if acc[b] else 0.0 for b in range(BP)])
        W = _check(H, [("trial_done",)], approx=dict(fx=bound))
        assert (W["small_res"][:BP] != 0).any() and not (W["small_res"][:BP] != 0).all()
        assert (W["fx"][:BP][acc] != H["fx"][:BP][acc]).all()


@types
@shapes
def test_random_line_search(built, shape, f32):
    """random mode: Dphi = g'dx and phi(x) of ls_begin within their bounds — phi = T(0.5) sf - slc + eta scc / 2 from three sums: the sums'
    bounds through the expression, plus eps(T) of each term's magnitude for each of the four operations behind the sums —; then ls_test
    with phix placed |phi(xl)| + |gammaA alpha Dphi| + 1 above or below the threshold (asserted against 1000 x the bound of phi(xl)), so
    bt and flags[6] are compared exactly"""
    T = F32 if f32 else F64
    n, m, p = shape
    epsT = float(np.finfo(T).eps)

    def phi_bound(S, b, F, c, eta):
        f, cc, lam = _wide(F[b, :m]), _wide(c[b, :p]), _wide(S["lam"][b, :p])
        mags = 0.5 * (f ** 2).sum() + np.abs(lam * cc).sum() + abs(float(eta)) / 2 * (cc ** 2).sum()
        return 0.5 * _sum_bound(T, f ** 2) + (_sum_bound(T, lam * cc) + abs(float(eta)) / 2 * _sum_bound(T, cc ** 2) if p else 0.0) + 4 * epsT * mags

    for phase in (0, 1):
        H = _base(T, BP, shape, nnzjF=257, seed=phase, normal=True)
        H["lsm"][:BP] = (np.arange(BP) + phase) % 2
        lsm = H["lsm"] != 0
        lsm[BP:] = False
        with np.errstate(all="ignore"):
            eta = [T(1) / H["delta"][b] if p and lsm[b] else H["eta"][b] for b in range(BP)]
        approx = dict(Dphi=np.array([_sum_bound(T, _wide(H["ls_g"][b, :n]) * _wide(H["d"][b, :n])) for b in range(BP)]),
                      phix=np.array([phi_bound(H, b, H["Fx"], H["cx"], eta[b]) for b in range(BP)]))
        _check(H, [("ls_begin",)], only_rows={k: lsm for k in ("xl", "alpha", "Dphi", "phix")}, approx=approx)
    for j, assign in enumerate(_batches(N_LS_SCEN, BP)):
        H, want, _ = _ls_test_state(T, shape, 257, False, j, assign, normal=True)
        for b, (name, w1, w0, phil, big) in enumerate(want):
            if name in ("satisfied at equality", "failed by one ulp"):   # no equality on rounded sums: the clear cases instead
                t = H["gammaA"] * H["alpha"][b] * H["Dphi"][b]
                H["phix"][b] = phil - t + (big if name == "satisfied at equality" else -big)
            assert float(big) >= 1000 * phi_bound(H, b, H["Fl"], H["cl"], H["eta"][b]), name
            with np.errstate(all="ignore"):
                thr = H["phix"][b] + H["gammaA"] * H["alpha"][b] * H["Dphi"][b]
            assert abs(float(phil) - float(thr)) >= 0.5 * float(big), name
        for first in (1, 0):
            W = _check(H, [("ls_test", first)])
            for b, (name, w1, w0, _, _) in enumerate(want):
                assert W["bt"][b] == (w1 if first else w0), (name, first)


@types
@pytest.mark.parametrize("B", [257])
def test_random_end(built, B, f32):
    """random mode of cnl_outer_end_dev: sum |lam| over p = 300 ordinary numbers, smax = 1/2 so that ds = sum |lam| / (p smax) is a
    reduction's output; epstol a factor 2 above or below the measure (asserted against 1000 x the bound); statuses exactly"""
    T = F32 if f32 else F64
    H = _base(T, B, (3, 2, 300), seed=1, normal=True, smax=0.5)
    H["status"][:B] = 0
    H["done_in"][:B] = np.arange(B) % 3 != 0
    fo = np.arange(B) % 2
    with np.errstate(all="ignore"):
        for b in range(B):
            ds = sim.dual_scaling(H, b)
            assert ds > 1
            meas = sim.tmax(H["normdual"][b] / ds, T(0))
            H["normprimal"][b] = meas / T(4)
            H["epstol"][b] = meas * T(2 if fo[b] else 0.5)
            assert abs(float(meas) - float(H["epstol"][b])) >= 1000 * _rel_bound(T, 300) * float(meas)
    W = _check(H, [("end",)])
    done = H["done_in"][:B] != 0
    assert ((W["status"][:B] == 1) == (done & (fo == 1))).all()


# ---- the loop at statuses other than first_order ---------------------------------------------------------------------------------------------

F3 = dict(curvature=1.5, start=1.0, noise=0.5)      # the family of test_f3_device_resident_lockstep_outer_loop
ROUGH = dict(curvature=3.0, start=2.0, noise=0.5)
BL = 12
COUNTERS = ("iter", "nlinsolve", "nfact", "nbk")
_scalar = {}


def _loop_mods():
    import torch
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import device_loop as DL, hipldl, synthetic as syn
    return torch, DL, hipldl, syn


def _loop_family(shape, kind):
    torch, DL, hipldl, syn = _loop_mods()
    n, p = shape
    return DL.BandQuadFamily(syn.band_structure(n, p), BL, seed=n + p, torch=torch, device="cuda:0", **kind)


def _scalar_runs(fam, key, prm, **kw):
    """outer_loop.solve with the CPU oracle, problem by problem: once per case, shared by the tests that need it"""
    if key not in _scalar:
        from cannoles_jl_amd import outer_loop
        from tests.test_oracle_pinning import oracle_newton, oracle_solver
        _scalar[key] = [outer_loop.solve(fam.host_model(b), oracle_solver, oracle_newton, prm, **kw) for b in range(BL)]
    return _scalar[key]


def _same_decisions(got, ones, tag):
    assert got["status"] == [o["status"] for o in ones], tag
    for k in COUNTERS:
        assert got[k].tolist() == [o[k] for o in ones], (tag, k)


@pytest.mark.parametrize("shape", [(300, 4), (300, 0)])
def test_loop_inner_iteration_limit_ends_stalled(built, shape):
    """max_inner = 1 on the rough family: the device loop gives `stalled` (status 5) where the scalar loop stops at the limit — on
    (300, 4) problems 2, 5, 6 and 11 end first_order and the other eight stall; on (300, 0) five stall — with the scalar loop's iter,
    nlinsolve, nfact and nbk; compact = True gives the same bit for bit; the framework form agrees in statuses and counters"""
    torch, DL, hipldl, syn = _loop_mods()
    from tests.test_compact_gpu import _same
    fam = _loop_family(shape, ROUGH)
    prm = hipldl.default_params()
    ones = _scalar_runs(fam, ("max_inner", shape), prm, max_inner=1)
    status = [o["status"] for o in ones]
    print(f"max_inner = 1, rough {shape}: scalar loop {status}")
    stalled = [b for b in range(BL) if status[b] == "stalled"]
    assert set(status) == {"first_order", "stalled"} and (stalled == [0, 1, 3, 4, 7, 8, 9, 10] if shape[1] else len(stalled) == 5)
    got = DL.solve_batch_device(fam, prm, max_inner=1)
    print(f"max_inner = 1, rough {shape}: device loop {got['status']}, iter = {got['iter'].tolist()}, nbk = {got['nbk'].tolist()}")
    _same_decisions(got, ones, "device")
    packed = DL.solve_batch_device(fam, prm, max_inner=1, compact=True, compact_min_finished=1)
    _same(packed, got)
    assert packed["compactions"] >= 1
    old = DL.solve_batch_device_framework(fam, prm, max_inner=1)
    print(f"max_inner = 1, rough {shape}: framework form {old['status']}")
    _same_decisions(old, ones, "framework")


@pytest.mark.parametrize("rho_max", [100.0, 10.0])
def test_loop_rho_max_ends_exception(built, rho_max):
    """params[6] = rho_max on the (300, 4) family of test_f3_device_resident_lockstep_outer_loop: the rho ladder's values there are 6.06,
    16.1 and 606, so the cuts at 100 and at 10 are far from each.  rho_max = 100: problems 4, 5 and 9 end `exception` at their first Newton
    system (nfact = 5, iter = 1), nine end first_order, some of them after backtracking; rho_max = 10: nine end `exception`, three first_order.  Statuses and counters per
    problem as the scalar loop's, the surviving solutions to that test's tolerances, and the framework form agrees"""
    torch, DL, hipldl, syn = _loop_mods()
    fam = _loop_family((300, 4), F3)
    prm = hipldl.default_params()
    prm[6] = rho_max
    ones = _scalar_runs(fam, ("rho_max", rho_max), prm)
    status = [o["status"] for o in ones]
    print(f"rho_max = {rho_max}: scalar loop {status}")
    exc = [b for b in range(BL) if status[b] == "exception"]
    assert set(status) == {"first_order", "exception"}
    if rho_max == 100.0:
        assert exc == [4, 5, 9] and all((ones[b]["nfact"], ones[b]["iter"]) == (5, 1) for b in exc) and any(o["nbk"] > 0 for o in ones)
    else:
        assert len(exc) == 9 and any(ones[b]["iter"] == 2 for b in exc)
    got = DL.solve_batch_device(fam, prm)
    print(f"rho_max = {rho_max}: device loop {got['status']}, iter = {got['iter'].tolist()}, nfact = {got['nfact'].tolist()}, nbk = {got['nbk'].tolist()}")
    _same_decisions(got, ones, "device")
    for b in range(BL):
        if status[b] == "first_order":
            assert np.allclose(got["solution"][b], ones[b]["solution"], atol=1e-7, rtol=1e-7), b
            assert np.allclose(got["multipliers"][b], ones[b]["multipliers"], atol=1e-6, rtol=1e-6), b
            assert abs(got["objective"][b] - ones[b]["objective"]) <= 1e-9 * max(1.0, ones[b]["objective"]), b
    old = DL.solve_batch_device_framework(fam, prm)
    print(f"rho_max = {rho_max}: framework form {old['status']}")
    _same_decisions(old, ones, "framework")
