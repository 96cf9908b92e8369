"""The lockstep loop on its active problems only, on the GPU.  -m gpu.

Three layers: (1) cnl_set_active_batch — a handle on the first nb problems of its batch writes, for them, exactly what the full-batch
call writes and nothing for the others; (2) cnl_outer_compact_dev / _f32_dev against the pairing rule in numpy
(tests/support/compact_sim.py), every array compared exactly; (3) device_loop.solve_batch_device(compact=True) against compact=False:
every output bit for bit — each problem decides alone, so leaving the finished ones out changes nothing but the work."""
import ctypes as C

import numpy as np
import pytest

from tests.support import compact_sim
from tests.test_band_resident_gpu import _values
from tests.test_band_wide_gpu import _bit_equal, _model_values, _run_dev
from tests.test_compact_cpu import LS_ARRAYS, SCALARS, edge_cases
from tests.test_gpu_parity import _mods

pytestmark = pytest.mark.gpu

CNL_ERR_ARG, CNL_ERR_STATE = 1, 5
B70 = 70


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


# ---- (1) cnl_set_active_batch ----------------------------------------------------------------------------------------------------------

def _handle_cases(hipldl):
    T = hipldl.PLAN_THROUGHPUT
    return {"f64-band-pm": ("band", np.float64, dict(plan_kind=T)),
            "f64-band-resident": ("band", np.float64, dict(plan_kind=T, batch_layout=hipldl.LAYOUT_INTERLEAVED, band_problems_per_group=32)),
            "f32-band-pm": ("band", np.float32, dict(plan_kind=T)),
            "f32-band-il": ("band", np.float32, dict(plan_kind=T, batch_layout=hipldl.LAYOUT_INTERLEAVED)),
            "f32-model-wide": ("model", np.float32, dict(plan_kind=T)),
            "f64-model-register-front": ("model", np.float64, dict(plan_kind=T))}


def _case_data(kind, dtype):
    hipldl, syn, O = _mods()
    if kind == "band":
        s = syn.band_structure(200, 4)
        vals, rhs = _values(syn, s, B70, ladder=(1, 5, 17, 31, B70 - 1), hopeless=9)
    else:
        s = syn.model_band_structure(200, 4)
        vals, rhs = _model_values(syn, s, B70, ladder=(1, 5, 17, 20), hopeless=9)
    if dtype == np.float32:
        vals[9, s.offsets()[0]] = -1e30   # (hopeless, and finite in Float32)
    ro = np.zeros(B70)
    ro[5] = 0.3
    ro[2] = 1e-3
    return s, vals, rhs, ro


class _Passes:
    """the device-pointer passes of one handle on fresh, sentinel-filled outputs; inputs are fixed at construction"""

    def __init__(self, L, s, vals, rhs, ro, dtype):
        torch, dev = _torch()
        hipldl, syn, O = _mods()
        self.L, self.s, self.dtype, self.B = L, s, dtype, vals.shape[0]
        self.tt = torch.float64 if dtype == np.float64 else torch.float32
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)
        self.vals, self.rhs, self.ro = up(vals), up(rhs), up(ro)
        rng = np.random.default_rng(70)
        B, n, m, p = self.B, s.nvar, s.nequ, s.ncon
        u = lambda *sh: up(rng.uniform(-1, 1, sh))
        self.hF, self.hc, self.Jx, self.Jcx = u(B, s.nnzhF), u(B, s.nnzhc), u(B, s.nnzjF), u(B, s.nnzjc)
        self.delta = up(rng.uniform(0.1, 1.0, B))
        self.x, self.r, self.Fx, self.lam, self.cx, self.d = u(B, n), u(B, m), u(B, m), u(B, p), u(B, p), u(B, s.N)
        self.il = bool(L.config["batch_layout"])
        self.params = hipldl.default_params(dtype)
        # rows of solve_ldl!'s d that are unspecified: behind a failed factorisation the multifrontal kernels solve with whatever the
        # factor storage holds (include/cannoles_hip.h); the band kernels leave such a row alone
        self.unspecified = []

    def full(self, shape, value, dt=None):
        torch, dev = _torch()
        return torch.full(shape, value, dtype=dt or self.tt, device=dev)

    def to_layout(self, tv):
        """`tv` [B, nnz] in the handle's layout (always converted by the handle at its FULL batch)"""
        hipldl, syn, O = _mods()
        if not self.il:
            return tv.clone()
        nb = hipldl.get_active_batch(self.L)
        hipldl.set_active_batch(self.L, self.B)
        out = self.full((hipldl.layout_len(self.L, 0),), 9.0)
        hipldl.interleave_dev(self.L, 0, tv, out)
        hipldl.set_active_batch(self.L, nb)
        return out

    def from_layout(self, tin):
        hipldl, syn, O = _mods()
        if not self.il:
            return tin.clone()
        nb = hipldl.get_active_batch(self.L)
        hipldl.set_active_batch(self.L, self.B)
        out = self.full((self.B, self.s.nnzNS), -8.0)
        hipldl.deinterleave_dev(self.L, 0, tin, out)
        hipldl.set_active_batch(self.L, nb)
        return out

    def run(self, vals_in=None):
        """[success, d of solve, d, rho_old, rho, nfact, success, vals after] as tests.test_band_wide_gpu._run_dev returns them, then
        the row passes: vals of prepare, rhs and norms of f1, lambda and Jx'r of CGLS, xt, rt, lamt, dlam of the trial point"""
        torch, dev = _torch()
        hipldl, syn, O = _mods()
        L, s, B = self.L, self.s, self.B
        i32 = torch.int32
        tin = self.to_layout(self.vals if vals_in is None else vals_in)
        su = self.full((B,), -5, i32)
        d2 = self.full((B, s.N), 7.0)
        hipldl.factorize_dev(L, tin, float(self.params[0]), su)
        hipldl.solve_dev(L, self.rhs, d2)
        for b in self.unspecified:
            if b < hipldl.get_active_batch(L):
                d2[b] = 0.0
        d = self.full((B, s.N), 3.0)
        ro, rho = self.ro.clone(), self.full((B,), -2.0)
        nf, ok = self.full((B,), -5, i32), self.full((B,), -5, i32)
        hipldl.newton_system_dev(L, tin, self.rhs, d, ro, rho, nf, ok, self.params)
        out = [su, d2, d, ro, rho, nf, ok, self.from_layout(tin)]
        # rows f2, f1, f4 and the trial point
        pv = self.to_layout(self.full((B, s.nnzNS), 9.0))
        p = s.ncon
        hipldl.prepare_newton_system_dev(L, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, self.hF, self.hc if p else 0, self.Jx, self.Jcx if p else 0,
                                         self.delta if p else 0, pv)
        f1_rhs, f1_nrm = self.full((B, s.N), 5.0), self.full((B, 2), 5.0)
        hipldl.residual_vectors_jac_dev(L, s.nnzjF, s.nnzjc, self.Jx, self.Jcx if p else 0, self.r, self.lam if p else 0, self.Fx,
                                        self.cx if p else 0, f1_rhs, f1_nrm)
        lam_o, jxtr, iters = self.full((B, max(p, 1)), 4.0), self.full((B, s.nvar), 4.0), self.full((B,), -5, i32)
        hipldl.cgls_multipliers_jac_dev(L, s.nnzjF, s.nnzjc, self.Jx, self.Jcx, self.r, lam_o, jxtr, iters_ptr=iters)
        xt, rt = self.full((B, s.nvar), 6.0), self.full((B, s.nequ), 6.0)
        lamt, dlam = self.full((B, max(p, 1)), 6.0), self.full((B, max(p, 1)), 6.0)
        hipldl.trial_point_dev(L, self.x, self.r, self.lam if p else 0, self.d, 1e4, xt, rt, lamt if p else 0, dlam if p else 0)
        # the layout conversions themselves at the handle's active batch
        il_o = dl_o = None
        if self.il:
            il_o = self.full((hipldl.layout_len(L, 0),), 9.0)
            hipldl.interleave_dev(L, 0, self.vals, il_o)
            dl_o = self.full((B, s.nnzNS), -8.0)
            hipldl.deinterleave_dev(L, 0, self.to_layout(self.vals), dl_o)
            il_o = self.from_layout(il_o)
        out += [self.from_layout(pv), f1_rhs, f1_nrm, lam_o, jxtr, iters, xt, rt, lamt, dlam] + ([il_o, dl_o] if self.il else [])
        torch.cuda.synchronize()
        return [a.cpu().numpy() for a in out]


SENTINELS = [-5, 7.0, 3.0, None, -2.0, -5, -5, None, 9.0, 5.0, 5.0, 4.0, 4.0, -5, 6.0, 6.0, 6.0, 6.0, 9.0, -8.0]


@pytest.mark.parametrize("nb", [37, 64])
@pytest.mark.parametrize("case", ["f64-band-pm", "f64-band-resident", "f32-band-pm", "f32-band-il", "f32-model-wide", "f64-model-register-front"])
def test_handle_on_a_prefix_of_its_batch(built, case, nb):
    """newton_system, factorize + solve, prepare, f1 `_jac`, CGLS `_jac`, the trial point (and the layout conversions) on the first nb
    of 70 problems — two full groups of 32 and a partial one; nb = 37 leaves the second group active in part — are bit-equal to the
    full-batch results for problems < nb; every output keeps its sentinel for problems >= nb, the rho slots of an interleaved `vals`
    included; cnl_set_active_batch(h, 70) restores the full-batch results."""
    torch, dev = _torch()
    hipldl, syn, O = _mods()
    kind, dtype, opt = _handle_cases(hipldl)[case]
    s, vals, rhs, ro = _case_data(kind, dtype)
    cfg_ref, ref = _run_dev(s, vals, rhs, ro, dtype=dtype, **opt)   # a handle of its own at the full batch
    rows, cols = s.kkt_pattern()
    L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B70, dtype=dtype, options=hipldl.Options(**opt))
    cfg = L.config
    assert {k: cfg[k] for k in ("band", "kernel", "band_pieces", "band_resident", "batch_layout")} == \
           {k: cfg_ref[k] for k in ("band", "kernel", "band_pieces", "band_resident", "batch_layout")}
    if case == "f64-model-register-front":
        assert not cfg["band"] and cfg["kernel"] == "v2"
    else:
        assert cfg["band"] and cfg["band_pieces"] == (20 if case == "f32-model-wide" else 15)
        assert cfg["band_resident"] == (case == "f64-band-resident") and cfg["batch_layout"] == int(case in ("f64-band-resident", "f32-band-il"))
    assert hipldl.get_active_batch(L) == B70
    run = _Passes(L, s, vals, rhs, ro, dtype)
    if not cfg["band"]:
        run.unspecified = [9]
        ref[1][9] = 0.0
    full0 = run.run()
    assert _bit_equal(full0[:8], ref)
    nfr, okr = ref[5], ref[6]
    assert all(nfr[b] > 1 for b in (1, 5, 17)) and not okr[9] and okr.sum() == B70 - 1

    hipldl.set_active_batch(L, nb)
    assert hipldl.get_active_batch(L) == nb and hipldl.layout_len(L, 0) == (hipldl.il_len(B70, s.nnzNS) if run.il else hipldl.layout_len(L, 0))
    marked = run.vals.clone()
    marked[nb:, -s.nvar:] = 123.0        # rho slots of the problems the handle must not touch
    part = run.run(vals_in=marked)
    for k, (a, f, sent) in enumerate(zip(part, full0, SENTINELS)):
        assert a.shape == f.shape, k
        assert np.array_equal(a[:nb].view(np.uint8), f[:nb].view(np.uint8)), (k, "problems below nb differ from the full-batch call")
        if k == 3:
            want = np.ascontiguousarray(ro, dtype)[nb:]                       # rho_old: read and updated in place
        elif k == 7:
            want = marked[nb:].cpu().numpy()                                  # vals: exactly what went in, rho slots included
        else:
            want = np.full_like(a[nb:], sent)
        assert np.array_equal(a[nb:].view(np.uint8), want.view(np.uint8)), (k, "something of a problem >= nb was written")
    with pytest.raises(hipldl.CnlError) as e:   # host-pointer calls take the whole batch's arrays
        hipldl.try_to_factorize(L, np.ascontiguousarray(vals, dtype), s.nvar, s.nequ, s.ncon, float(run.params[0]))
    assert e.value.code == CNL_ERR_STATE

    hipldl.set_active_batch(L, B70)
    assert _bit_equal(run.run(), full0)
    L.close()


def test_active_batch_errors_and_solve_needs_a_wide_enough_factor(built):
    torch, dev = _torch()
    hipldl, syn, O = _mods()
    s, vals, rhs, ro = _case_data("band", np.float64)
    rows, cols = s.kkt_pattern()
    L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B70, options=hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT))
    for bad in (0, B70 + 1, -4):
        with pytest.raises(hipldl.CnlError) as e:
            hipldl.set_active_batch(L, bad)
        assert e.value.code == CNL_ERR_ARG and hipldl.get_active_batch(L) == B70
    tv = torch.from_numpy(vals).to(dev)
    tr = torch.from_numpy(rhs).to(dev)
    su = torch.zeros(B70, dtype=torch.int32, device=dev)
    d = torch.zeros((B70, s.N), dtype=torch.float64, device=dev)
    hipldl.set_active_batch(L, 37)
    hipldl.factorize_dev(L, tv, float(hipldl.default_params()[0]), su)
    hipldl.solve_dev(L, tr, d)
    hipldl.set_active_batch(L, 64)          # wider than the factorisation: no factor for problems 37 .. 63
    with pytest.raises(hipldl.CnlError) as e:
        hipldl.solve_dev(L, tr, d)
    assert e.value.code == CNL_ERR_STATE
    hipldl.set_active_batch(L, 20)          # narrower: fine
    hipldl.solve_dev(L, tr, d)
    for call in (lambda: hipldl.solve_ldl_(rhs, L.factor, np.zeros_like(rhs)),
                 lambda: hipldl.newton_system_(np.zeros_like(rhs), s.nvar, s.nequ, s.ncon, rhs, vals.copy(), L, ro, hipldl.default_params())):
        with pytest.raises(hipldl.CnlError) as e:
            call()
        assert e.value.code == CNL_ERR_STATE
    torch.cuda.synchronize()
    L.close()


def test_staged_handle_refuses_or_serves(built):
    """a default-plan Float64 handle of 70 problems runs staged: CNL_ERR_STATE with the handle unchanged (or success, with the same
    guarantees); nb = the created batch is accepted by every handle"""
    torch, dev = _torch()
    hipldl, syn, O = _mods()
    s, vals, rhs, ro = _case_data("band", np.float64)
    vals, rhs = _values(syn, s, B70, ladder=(1, 5, 17, 31, B70 - 1))   # (nobody hopeless: see _Passes.unspecified)
    cfg_ref, ref = _run_dev(s, vals, rhs, ro)
    rows, cols = s.kkt_pattern()
    L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B70)
    run = _Passes(L, s, vals, rhs, ro, np.float64)
    hipldl.set_active_batch(L, B70)
    try:
        hipldl.set_active_batch(L, 37)
        served = True
    except hipldl.CnlError as e:
        assert e.code == CNL_ERR_STATE and "cnl_set_active_batch" in str(e)
        served = False
    print(f"default-plan handle of {B70} problems (kernel {L.config['kernel']}): cnl_set_active_batch(37) {'served' if served else 'refused'}")
    if served:
        part = run.run()
        for a, f in zip(part[:3] + part[4:7], ref[:3] + ref[4:7]):
            assert np.array_equal(a[:37].view(np.uint8), f[:37].view(np.uint8))
        assert (part[2][37:] == 3.0).all() and (part[5][37:] == -5).all()
        hipldl.set_active_batch(L, B70)
    assert hipldl.get_active_batch(L) == B70
    assert _bit_equal(run.run()[:8], ref)
    L.close()


# ---- (2) the compaction kernels ---------------------------------------------------------------------------------------------------------

INT32 = ("status", "it", "flags", "nf_new", "ok_new")
INT64 = ("inner", "nfact", "nlin", "nbk")
MASKS = ("phase0", "act", "need", "brk", "ext", "lsm", "rej", "chk", "done_in", "tired", "small_res", "bt")


def _row_width(k, n, m, P, N, nnzjF, nnzjc):
    if k in ("d", "d_new", "rhs_cur", "rhs_t", "ls_g"):
        return N
    if k in ("x", "xt", "xt_e", "xl"):
        return n
    if k in ("r", "Fx", "rt", "Ft", "rt_e", "Fl"):
        return m
    if k in ("cx", "lam", "ct", "lamt", "lamt_e", "cl", "lam_ls"):
        return P
    if k in ("Jv", "Jt"):
        return nnzjF
    if k in ("Jcv", "Jct"):
        return max(nnzjc, 1)
    return 2 if k == "nrm_t" else 1


def _build_state(B, p, f32, share_jc):
    """a state of B problems (n = 5, m = 7) whose every array holds row-identifying values; every second array starts one element off
    a 16-byte boundary (rows are element-aligned only).  Returns (state, {name: tensor}, [moved array names])"""
    torch, dev = _torch()
    hipldl, syn, O = _mods()
    n, m = 5, 7
    P, N, nnzjF, nnzjc = max(p, 1), n + m + p, 11, (3 if p else 0)
    st = hipldl.cnl_outer_state_f32() if f32 else hipldl.cnl_outer_state()
    for k, v in dict(B=B, n=n, m=m, p=p, P=P, N=N, nnzjF=nnzjF, nnzjc=nnzjc, max_inner=10, dmin=1e-8, rhomax=1e10, delta_dec=0.1, smax=100.0,
                     gammaA=1e-2, eps2=1e-30).items():
        setattr(st, k, v)
    ft = torch.float32 if f32 else torch.float64
    keep = {}
    for idx, (k, _) in enumerate(st._fields_):
        if k in SCALARS:
            continue
        if k == "Jct" and share_jc:
            keep[k] = keep["Jcv"]
            setattr(st, k, keep[k].data_ptr())
            continue
        w = 8 if k == "flags" else _row_width(k, n, m, P, N, nnzjF, nnzjc)
        rows_ = 1 if k == "flags" else B
        dt = torch.int32 if k in INT32 else torch.int64 if k in INT64 else torch.uint8 if k in MASKS else ft
        buf = torch.zeros(rows_ * w + 1, dtype=dt, device=dev)
        a = buf[idx % 2:idx % 2 + rows_ * w].view(rows_, w)
        val = (torch.arange(rows_, device=dev)[:, None] * 7 + torch.arange(w, device=dev)[None, :] + idx)
        a.copy_((val % 251 + 1).to(dt) if dt == torch.uint8 else val.to(dt))
        keep[k] = a
        setattr(st, k, a.data_ptr())
    moved = [k for k in keep if k != "flags" and not (k in ("Jcv", "Jct") and nnzjc == 0)]
    return st, keep, moved


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("p", [2, 0])
@pytest.mark.parametrize("B", [70, 1])
def test_compaction_kernels_against_the_pairing_rule(built, B, p, f32):
    """every per-problem array of the state, two extra arrays (rows of 4 and 24 bytes), d_orig and d_counts exactly as
    compact_sim says, for the statuses of every CPU edge case; a second call changes nothing"""
    torch, dev = _torch()
    hipldl, syn, O = _mods()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for name, status, Bc, min_finished in edge_cases(B):
        st, keep, moved = _build_state(B, p, f32, share_jc=not f32)
        keep["status"].copy_(torch.from_numpy(np.asarray(status, np.int32)).to(dev)[:, None])
        st.B = Bc
        e4 = (torch.arange(B, dtype=torch.float32, device=dev) * 3 + 0.5).view(B, 1).contiguous()
        e24 = (torch.arange(B * 3, dtype=torch.float64, device=dev) - 11.0).view(B, 3).contiguous()
        orig = torch.arange(B, dtype=torch.int32, device=dev)
        counts = torch.full((2,), -1, dtype=torch.int32, device=dev)
        work = torch.zeros(B + 2, dtype=torch.int32, device=dev)
        arrays = {k: keep[k] for k in moved}
        arrays.update(e4=e4, e24=e24, orig=orig.view(B, 1))
        before = {k: v.cpu().numpy().copy() for k, v in arrays.items()}
        flags0 = keep["flags"].cpu().numpy().copy()
        still = {k: keep[k].cpu().numpy().copy() for k in keep if k not in moved}
        perm, want_counts = compact_sim.compact(status, Bc, min_finished)
        extras = [(e4.data_ptr(), 4), (e24.data_ptr(), 24)]
        for call in range(2):
            hipldl.outer_compact_dev(st, extras, min_finished, orig, counts, work, stream)
            torch.cuda.synchronize()
            assert tuple(counts.tolist()) == want_counts, (name, call)
            for k, v in arrays.items():
                assert np.array_equal(v.cpu().numpy(), compact_sim.apply(perm, before[k])), (name, call, k)
            for k, v in still.items():
                assert np.array_equal(keep[k].cpu().numpy(), v), (name, call, k)
            assert np.array_equal(keep["flags"].cpu().numpy(), flags0)
            assert np.array_equal(orig.cpu().numpy(), perm), (name, call)


# ---- (3) the loop --------------------------------------------------------------------------------------------------------------------------

ROUGH = dict(curvature=3.0, start=2.0, noise=0.5)
BL = 40
EXACT = ("solution", "multipliers", "r", "objective", "normdual", "normprimal", "epstol", "iter", "nfact", "nlinsolve", "nbk")


def _same(a, b):
    for k in EXACT:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert a["status"] == b["status"] and a["steps"] == b["steps"]


@pytest.mark.parametrize("case", ["f32-300-4-interleaved", "f32-300-0-problem-major", "f64-300-0-band", "f64-300-4-register-front", "f64-300-4-staged"])
def test_loop_on_the_active_problems_is_bit_equal(built, case):
    """the rough family (the rho ladder is climbed, the line search backtracks; its problems finish at different steps), 40 problems,
    compact_min_finished = 1 against compact = False: every output bit for bit, in the original problem order; the loop really left
    finished problems out; the handle went along except where it runs staged; the family is not touched; a second run gives the same"""
    torch, dev = _torch()
    hipldl, syn, O = _mods()
    from cannoles_jl_amd import device_loop as DL
    T = {"plan_kind": hipldl.PLAN_THROUGHPUT}
    shape, dtype, kw, kernel, layout, shrinks = {
        "f32-300-4-interleaved": ((300, 4), np.float32, dict(layout="interleaved"), "band", "interleaved", True),
        "f32-300-0-problem-major": ((300, 0), np.float32, dict(layout="problem-major"), "band", "problem-major", True),
        "f64-300-0-band": ((300, 0), np.float64, dict(tuning=T), "band", None, True),
        "f64-300-4-register-front": ((300, 4), np.float64, dict(tuning=T), "v2", "problem-major", True),
        "f64-300-4-staged": ((300, 4), np.float64, dict(), None, "problem-major", None)}[case]
    n, p = shape
    fam = DL.BandQuadFamily(syn.band_structure(n, p), BL, seed=n + p, torch=torch, device="cuda:0", dtype=dtype, **ROUGH)
    data0 = {k: v.clone() for k, v in fam.d.items()}
    plain = DL.solve_batch_device(fam, **kw)
    assert (kernel is None or plain["kernel"] == kernel) and (layout is None or plain["vals_layout"] == layout)
    assert "compactions" not in plain
    got = DL.solve_batch_device(fam, compact=True, compact_min_finished=1, **kw)
    print(f"{case}: steps = {got['steps']}, compactions = {got['compactions']}, problem_steps = {got['problem_steps']} of {got['steps'] * BL}, "
          f"handle_shrunk = {got['handle_shrunk']}, nlinsolve = {got['nlinsolve'].tolist()}, status = {sorted(set(got['status']))}")
    assert got["kernel"] == plain["kernel"] and got["vals_layout"] == plain["vals_layout"]
    _same(got, plain)
    assert got["compactions"] >= 1 and got["problem_steps"] < got["steps"] * BL
    if shrinks is not None:
        assert got["handle_shrunk"] is shrinks
    for k, v in fam.d.items():
        assert torch.equal(v, data0[k]), k
    again = DL.solve_batch_device(fam, compact=True, **kw)   # (the default threshold: max(32, working batch // 8))
    _same(again, plain)
    assert again["problem_steps"] <= again["steps"] * BL
