"""Float32 rows f1 / f2 / f4 and the trial point on the device (the `_f32_dev` entry points through hipldl's helpers on a Float32
handle) against tests/support/f32_rows.py, the oracle's rows restated in float32.  -m gpu.

Bit for bit: f2 in both layouts, f1 (column tiles and the gather kernel), Jx'r, xt, rt.  Within a few eps(Float32): dlambda and
lambdat (the norm's double sum is ordered differently).  CGLS: the restated recurrence's iteration counts, with every stopping test
at least MARGIN away from its threshold (asserted, so a change of seed cannot pass silently), and the least-squares optimality of
an fp64 lstsq.  A whole device-resident Float32 inner iteration: both layouts bit-equal, the Newton outputs held to the fp64 oracle
as tests/test_float32_gpu.py holds them.
"""
import numpy as np
import pytest

from tests.support import f32_rows as R

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
MARGIN = 1e-3
BWD_TOL = 512 * EPS32
FWD_TOL = 1e-3
CNL_ERR_ARG, CNL_ERR_STATE = 1, 5


def _mods():
    import torch
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    from oracle import oracle as O
    return torch, hipldl, syn, O


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _same(a, b):
    """bit-equal float32 arrays, NaN where the other has NaN (any payload)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    z = np.float32(0)
    return np.array_equal(np.where(np.isnan(a), z, a).view(np.uint32), np.where(np.isnan(b), z, b).view(np.uint32))


def _handle(hipldl, s, B, **opt):
    rows, cols = s.kkt_pattern()
    return hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32,
                               options=hipldl.Options(**opt) if opt else None)


def _model(s, B, seed):
    """the model's arrays of a batch (float32): Hessian and Jacobian values, delta, and the vectors rows f1 and the trial point take"""
    rng = np.random.default_rng(seed)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)   # noqa: E731
    m = {"hF": f(B, s.nnzhF), "hc": f(B, s.nnzhc), "Jx": f(B, s.nnzjF), "Jcx": f(B, s.nnzjc), "delta": np.abs(f(B)),
         "x": f(B, s.nvar), "r": f(B, s.nequ), "lam": f(B, s.ncon), "Fx": f(B, s.nequ), "cx": f(B, s.ncon), "d": f(B, s.N)}
    m["hc"][:, ::7] = 0.0   # H_c <- -hc writes -0.0 there
    m["delta"][3 % B] = 0.0
    return m


def _prepared(s, m, old=None):
    B = m["Jx"].shape[0]
    old = np.ones((B, s.nnzNS), np.float32) if old is None else old
    return R.prepare(old, s.nvar, s.nequ, s.ncon, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, m["hF"], m["hc"], m["Jx"], m["Jcx"], m["delta"])


@pytest.mark.parametrize("hess", [True, False])
def test_prepare_in_both_layouts(built, hess):
    torch, hipldl, syn, O = _mods()
    s = syn.band_structure(1000, 10)
    B = 67
    m = _model(s, B, 1)
    old = np.random.default_rng(2).standard_normal((B, s.nnzNS)).astype(np.float32)
    want = R.prepare(old, s.nvar, s.nequ, s.ncon, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, m["hF"] if hess else None, m["hc"], m["Jx"], m["Jcx"],
                     m["delta"])
    t = {k: _dev(torch, v) for k, v in m.items()}
    args = (s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, t["hF"] if hess else 0, t["hc"], t["Jx"], t["Jcx"], t["delta"])
    L = _handle(hipldl, s, B)
    v = _dev(torch, old)
    hipldl.prepare_newton_system_dev(L, *args, v)
    torch.cuda.synchronize()
    got = v.cpu().numpy()
    assert _same(got, want)
    off = s.offsets()
    assert np.array_equal(got[:, off[4]:off[5]].view(np.uint32), old[:, off[4]:off[5]].view(np.uint32))   # -I: left alone
    if not hess:
        assert np.array_equal(got[:, :off[1]].view(np.uint32), old[:, :off[1]].view(np.uint32))        # H_F without hF: left alone
    assert np.signbit(got[3, off[5]]) and np.signbit(got[0, off[1]]) and got[0, off[1]] == 0   # -delta = -0.0, -hc = -0.0
    L.close()
    Li = _handle(hipldl, s, B, batch_layout=hipldl.LAYOUT_INTERLEAVED)
    vi = torch.zeros(hipldl.layout_len(Li, 0), dtype=torch.float32, device=v.device)
    hipldl.interleave_dev(Li, 0, _dev(torch, old), vi)
    hipldl.prepare_newton_system_dev(Li, *args, vi)
    back = torch.zeros((B, s.nnzNS), dtype=torch.float32, device=v.device)
    hipldl.deinterleave_dev(Li, 0, vi, back)
    torch.cuda.synchronize()
    assert np.array_equal(back.cpu().numpy().view(np.uint32), got.view(np.uint32))
    Li.close()


F1_CASES = [("cfg4", 1000, 10, 96), ("odd", 777, 7, 67), ("unconstrained", 600, 0, 40)]


@pytest.mark.parametrize("name,n,p,B", F1_CASES)
def test_residual_vectors_bit_exact(built, name, n, p, B):
    """row f1 on column tiles and on the gather kernel, bit-equal to each other and to the restatement; the `_jac` twin bit-equal"""
    torch, hipldl, syn, O = _mods()
    s = syn.band_structure(n, p)
    rows, cols = s.kkt_pattern()
    m = _model(s, B, 10 + n)
    if name == "cfg4":
        m["r"][5, 17] = np.nan   # reaches the dual part (the columns of row 17) and both norms
    vals = _prepared(s, m)
    want_rhs, want_nrm = R.residual_vectors(rows, cols, vals, s.nvar, s.nequ, s.ncon, m["r"], m["lam"], m["Fx"], m["cx"])
    if name == "cfg4":
        assert np.isnan(want_rhs[5, :s.nvar]).any() and np.isnan(want_nrm[5]).all()
    t = {k: _dev(torch, v) for k, v in m.items()}
    tv = _dev(torch, vals)
    lam, cx = (t["lam"], t["cx"]) if s.ncon else (0, 0)
    outs = []
    for tiles in (1, 0):
        L = _handle(hipldl, s, B, f1_tiles=tiles)
        assert L.config["f1_tiles"] == bool(tiles) and L.config["float32"]
        rhs = torch.full((B, s.N), 9.0, dtype=torch.float32, device=tv.device)
        nrm = torch.full((B, 2), -1.0, dtype=torch.float32, device=tv.device)
        hipldl.residual_vectors_dev(L, tv, t["r"], lam, t["Fx"], cx, rhs, nrm)
        rhs2, nrm2 = torch.zeros_like(rhs), torch.zeros_like(nrm)
        hipldl.residual_vectors_jac_dev(L, s.nnzjF, s.nnzjc, t["Jx"], t["Jcx"] if s.ncon else 0, t["r"], lam, t["Fx"], cx, rhs2, nrm2)
        torch.cuda.synchronize()
        got = [x.cpu().numpy() for x in (rhs, nrm, rhs2, nrm2)]
        assert _same(got[0], want_rhs) and _same(got[1], want_nrm), tiles
        assert _same(got[2], got[0]) and _same(got[3], got[1]), tiles
        outs.append(got)
        L.close()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(outs[0], outs[1]))


def test_trial_point(built):
    torch, hipldl, syn, O = _mods()
    s = syn.band_structure(1000, 10)
    B = 40
    m = _model(s, B, 3)
    d = m["d"]
    d[2, s.nvar + s.nequ:] *= 1e4        # over the cap
    d[7, s.nvar + s.nequ:] *= 1e25       # squares overflow float: the norm's sum runs in double
    want = R.trial_point(s.nvar, s.nequ, s.ncon, m["x"], m["r"], m["lam"], d, 1e4)
    t = {k: _dev(torch, v) for k, v in m.items()}
    L = _handle(hipldl, s, B)
    out = [torch.full(a.shape, 5.0, dtype=torch.float32, device=t["x"].device) for a in want]
    hipldl.trial_point_dev(L, t["x"], t["r"], t["lam"], t["d"], 1e4, *out)
    torch.cuda.synchronize()
    xt, rt, lt, dl = (x.cpu().numpy() for x in out)
    assert _same(xt, want[0]) and _same(rt, want[1])
    assert np.all(np.abs(dl - want[3]) <= 4 * EPS32 * np.abs(want[3]))
    assert np.all(np.abs(lt - want[2]) <= 4 * EPS32 * (np.abs(m["lam"]) + np.abs(want[3])))
    nrm = np.sqrt(np.sum(dl.astype(np.float64) ** 2, axis=1))
    assert np.isfinite(dl[7]).all() and nrm[7] <= 1e4 * (1 + 4 * EPS32) and nrm[2] <= 1e4 * (1 + 4 * EPS32)
    assert np.array_equal(dl[0], -d[0, s.nvar + s.nequ:])   # under the cap: dlambda = -d
    L.close()


def test_cgls_multipliers(built):
    torch, hipldl, syn, O = _mods()
    s = syn.band_structure(1000, 10)
    rows, cols = s.kkt_pattern()
    B = 24
    m = _model(s, B, 4)
    m["r"][0] = 0.0   # lambda = 1 (src/CaNNOLeS.jl:515-517)
    vals = _prepared(s, m)
    t = {k: _dev(torch, v) for k, v in m.items()}
    tv = _dev(torch, vals)
    L = _handle(hipldl, s, B)
    dev = tv.device
    lam, jt, it = (torch.zeros((B, s.ncon), dtype=torch.float32, device=dev), torch.zeros((B, s.nvar), dtype=torch.float32, device=dev),
                   torch.zeros(B, dtype=torch.int32, device=dev))
    hipldl.cgls_multipliers_dev(L, tv, t["r"], lam, jt, iters_ptr=it)
    lam2, jt2, it2 = torch.zeros_like(lam), torch.zeros_like(jt), torch.zeros_like(it)
    hipldl.cgls_multipliers_jac_dev(L, s.nnzjF, s.nnzjc, t["Jx"], t["Jcx"], t["r"], lam2, jt2, iters_ptr=it2)
    torch.cuda.synchronize()
    lam, jt, it, lam2, jt2, it2 = (x.cpu().numpy() for x in (lam, jt, it, lam2, jt2, it2))
    assert np.array_equal(lam.view(np.uint32), lam2.view(np.uint32)) and np.array_equal(jt.view(np.uint32), jt2.view(np.uint32))
    assert np.array_equal(it, it2)
    off = s.offsets()
    i0, j0 = rows - 1, cols - 1
    for b in range(B):
        lam0, jt0, it0, margin = R.cgls_multipliers(rows, cols, vals[b], s.nvar, s.nequ, s.ncon, m["r"][b])
        assert margin > MARGIN, f"problem {b}: a stopping test lies within {margin:.3g} of its threshold"
        assert _same(jt[b], jt0), b
        assert it[b] == it0, (b, it[b], it0)
        if b == 0:
            assert it[b] == 0 and np.array_equal(lam[b], np.ones(s.ncon, np.float32))
            continue
        A = np.zeros((s.nvar, s.ncon))
        k = np.arange(off[3], off[4])
        A[j0[k], i0[k] - s.nvar - s.nequ] = vals[b, k]
        rhs = jt0.astype(np.float64)
        ls = np.linalg.lstsq(A, rhs, rcond=None)[0]
        assert np.linalg.norm(A.T @ (A @ lam[b].astype(np.float64) - rhs)) <= 2e-3 * np.linalg.norm(A.T @ rhs), b
        assert np.linalg.norm(lam[b] - ls) <= 1e-3 * np.linalg.norm(ls), b
    L.close()


def test_mixed_types_and_layout_rules(built):
    torch, hipldl, syn, O = _mods()
    lib = hipldl.lib()
    s = syn.band_structure(400, 4)
    B = 4
    rows, cols = s.kkt_pattern()
    L64 = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B)
    dev = torch.device("cuda", 0)
    buf = torch.full((B, 2 * max(s.nnzNS, s.N)), 5.0, dtype=torch.float32, device=dev)
    ib = torch.full((4 * B,), 7, dtype=torch.int32, device=dev)
    a, i = buf.data_ptr(), ib.data_ptr()
    calls = [
        lambda h: lib.cnl_prepare_newton_system_f32_dev(h, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, a, a, a, a, a, a, None),
        lambda h: lib.cnl_residual_vectors_f32_dev(h, a, a, a, a, a, a, a, None),
        lambda h: lib.cnl_residual_vectors_jac_f32_dev(h, s.nnzjF, s.nnzjc, a, a, a, a, a, a, a, a, None),
        lambda h: lib.cnl_cgls_multipliers_f32_dev(h, a, a, a, a, 1e-4, 1e-4, 0, 1, i, None),
        lambda h: lib.cnl_cgls_multipliers_jac_f32_dev(h, s.nnzjF, s.nnzjc, a, a, a, a, a, 1e-4, 1e-4, 0, 1, i, None),
        lambda h: lib.cnl_trial_point_f32_dev(h, a, a, a, a, 1e4, a, a, a, a, None),
    ]
    for call in calls:
        assert call(L64._h) == CNL_ERR_STATE, lib.cnl_last_error()
        assert call(None) == CNL_ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == 5.0).all()) and bool((ib == 7).all())   # nothing launched, nothing written
    Li = _handle(hipldl, s, B, batch_layout=hipldl.LAYOUT_INTERLEAVED)
    assert lib.cnl_residual_vectors_f32_dev(Li._h, a, a, a, a, a, a, a, None) == CNL_ERR_STATE
    assert lib.cnl_cgls_multipliers_f32_dev(Li._h, a, a, a, a, 1e-4, 1e-4, 0, 1, i, None) == CNL_ERR_STATE
    torch.cuda.synchronize()
    assert bool((buf == 5.0).all())
    L32 = _handle(hipldl, s, B)
    t64 = torch.zeros((B, 2 * max(s.nnzNS, s.N)), dtype=torch.float64, device=dev)
    with pytest.raises(TypeError):
        hipldl.residual_vectors_dev(L32, t64, buf, buf, buf, buf, buf, buf)
    with pytest.raises(TypeError):
        hipldl.prepare_newton_system_dev(L32, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, buf, buf, buf, buf, buf, t64)
    with pytest.raises(TypeError):
        hipldl.trial_point_dev(L32, buf, buf, buf, t64, 1e4, buf, buf, buf, buf)
    with pytest.raises(TypeError):
        hipldl.cgls_multipliers_jac_dev(L32, s.nnzjF, s.nnzjc, buf, buf, t64, buf)
    with pytest.raises(TypeError):
        hipldl.residual_vectors_jac_dev(L64, s.nnzjF, s.nnzjc, buf, buf, buf, buf, buf, buf, buf, buf)
    torch.cuda.synchronize()
    assert bool((buf == 5.0).all()) and bool((t64 == 0).all())
    for h in (L64, Li, L32):
        h.close()


# ---- one whole device-resident inner iteration (the Newton checks of tests/test_float32_gpu.py, restated here) ----------------
def _backward_error(s, vals, rhs, d):
    import scipy.sparse as sp
    rows, cols = s.kkt_pattern()
    Kl = sp.coo_matrix((np.asarray(vals, np.float64), (rows - 1, cols - 1)), shape=(s.N, s.N)).tocsr()
    K = Kl + sp.tril(Kl, -1).T
    d, rhs = np.asarray(d, np.float64), np.asarray(rhs, np.float64)
    res = K @ d + rhs
    return np.abs(res).max() / (abs(K).sum(axis=1).max() * np.abs(d).max() + np.abs(rhs).max())


def _check_newton_against_oracle(O, s, vals32, rhs32, d, ok, nf, rho, ro, vals_out):
    """tests/test_float32_gpu.py's rules: (success, nfact) and rho / rho_old as the fp64 oracle's on the widened Float32 data (its
    pivots asserted far from eig_tol), backward error <= 512 eps(Float32), forward error <= 1e-3"""
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl
    rows, cols = s.kkt_pattern()
    orc = O.Oracle(s.N, rows, cols, O.canonical_perm(s.nvar, s.nequ, s.ncon))
    p64 = hipldl.default_params(np.float32).astype(np.float64)
    for b in range(vals32.shape[0]):
        v64 = vals32[b].astype(np.float64)
        d0, ok0, rho0, ro0, nf0 = O.newton_system(orc, s.nvar, s.nequ, s.ncon, rhs32[b].astype(np.float64), v64, 0.0, p64)
        D = orc.D
        assert np.abs(np.abs(D) - p64[0]).min() >= MARGIN * np.abs(D).max(), b
        assert bool(ok[b]) == ok0 and int(nf[b]) == nf0, b
        assert np.float32(rho0).view(np.uint32) == np.float32(rho[b]).view(np.uint32), b
        assert np.float32(ro0).view(np.uint32) == np.float32(ro[b]).view(np.uint32), b
        assert np.array_equal(vals_out[b, -s.nvar:].view(np.uint32), v64[-s.nvar:].astype(np.float32).view(np.uint32)), b
        if ok0 and b % 7 == 0:
            assert _backward_error(s, vals_out[b], rhs32[b], d[b]) <= BWD_TOL, b
            assert np.abs(d[b] - d0).max() <= FWD_TOL * np.abs(d0).max(), b


def test_device_resident_inner_iteration(built):
    """prepare -> f1 (`_jac`) -> newton_system_f32_dev -> trial point -> f1 at the trial point, on cfg4's pattern, problem-major and
    interleaved: every output bit-equal between the two, the Newton outputs held to the oracle"""
    torch, hipldl, syn, O = _mods()
    s = syn.band_structure(1000, 10)
    B = 96
    rows, cols = s.kkt_pattern()
    vals64, _ = syn.batch_values(s, B, cfg=4)
    vals32 = vals64.astype(np.float32)
    off = s.offsets()
    m = _model(s, B, 6)
    m.update(hF=vals32[:, off[0]:off[1]], hc=-vals32[:, off[1]:off[2]], Jx=vals32[:, off[2]:off[3]], Jcx=vals32[:, off[3]:off[4]],
             delta=-vals32[:, off[5]])
    m["d"] = None
    scrambled = np.full_like(vals32, 3.0)
    scrambled[:, off[4]:off[5]] = -1.0   # the -I segment: prepare leaves it alone
    t = {k: _dev(torch, np.ascontiguousarray(v)) for k, v in m.items() if v is not None}
    dev = t["x"].device
    p32 = hipldl.default_params(np.float32)
    z = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=dev)   # noqa: E731
    runs = []
    for layout in (0, 1):
        L = _handle(hipldl, s, B, batch_layout=layout)
        vin = _dev(torch, scrambled)
        if layout:
            v = torch.zeros(hipldl.layout_len(L, 0), dtype=torch.float32, device=dev)
            hipldl.interleave_dev(L, 0, vin, v)
        else:
            v = vin
        rhs, nrm, d = z(B, s.N), z(B, 2), z(B, s.N)
        ro, rho = z(B), z(B)
        nf, ok = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        xt, rt, lt, dl = z(B, s.nvar), z(B, s.nequ), z(B, s.ncon), z(B, s.ncon)
        rhs_t, nrm_t = z(B, s.N), z(B, 2)
        hipldl.prepare_newton_system_dev(L, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, t["hF"], t["hc"], t["Jx"], t["Jcx"], t["delta"], v)
        hipldl.residual_vectors_jac_dev(L, s.nnzjF, s.nnzjc, t["Jx"], t["Jcx"], t["r"], t["lam"], t["Fx"], t["cx"], rhs, nrm)
        hipldl.newton_system_dev(L, v, rhs, d, ro, rho, nf, ok, p32)
        hipldl.trial_point_dev(L, t["x"], t["r"], t["lam"], d, 1e4, xt, rt, lt, dl)
        hipldl.residual_vectors_jac_dev(L, s.nnzjF, s.nnzjc, t["Jx"], t["Jcx"], rt, lt, t["Fx"], t["cx"], rhs_t, nrm_t)
        if layout:
            vout = torch.zeros((B, s.nnzNS), dtype=torch.float32, device=dev)
            hipldl.deinterleave_dev(L, 0, v, vout)
        else:
            vout = v
        torch.cuda.synchronize()
        runs.append([x.cpu().numpy() for x in (vout, rhs, nrm, d, ro, rho, nf, ok, xt, rt, lt, dl, rhs_t, nrm_t)])
        L.close()
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    vout, rhs, nrm, d, ro, rho, nf, ok = runs[0][:8]
    want_rhs, want_nrm = R.residual_vectors(rows, cols, vals32, s.nvar, s.nequ, s.ncon, m["r"], m["lam"], m["Fx"], m["cx"])
    assert _same(rhs, want_rhs) and _same(nrm, want_nrm)
    assert ok.all() and (nf == 1).all()
    _check_newton_against_oracle(O, s, vals32, rhs, d, ok, nf, rho, ro, vout)
    # prepare reproduced the generator's values (rho slots: rho = 0 at nfact = 1)
    assert np.array_equal(vout.view(np.uint32), vals32.view(np.uint32))


def test_rows_beyond_the_grid_limits(built):
    """prepare and the trial point on ONE linear grid dimension, row f1 in slices of 65 535 groups of problems: the probes either side
    of each limit against the restatement"""
    torch, hipldl, syn, O = _mods()
    s = syn.band_structure(24, 2)
    B = 263000
    rows, cols = s.kkt_pattern()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    mk = lambda n: torch.randn((B, n), dtype=torch.float32, device=dev, generator=g)   # noqa: E731
    hF, hc, Jx, Jc, de = mk(s.nnzhF), mk(s.nnzhc), mk(s.nnzjF), mk(s.nnzjc), mk(1).abs().reshape(B).contiguous()
    x, r, lam, d, Fx, cx = mk(s.nvar), mk(s.nequ), mk(s.ncon), mk(s.N), mk(s.nequ), mk(s.ncon)
    probe = np.array([0, 65534, 65535, 65536, 262139, 262140, 262141, B - 1])
    c = lambda a: a[probe].cpu().numpy()   # noqa: E731
    for tiles in (1, 0):
        L = _handle(hipldl, s, B, f1_tiles=tiles)
        assert L.config["f1_tiles"] == bool(tiles)
        vals = torch.full((B, s.nnzNS), 7.0, dtype=torch.float32, device=dev)
        hipldl.prepare_newton_system_dev(L, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, hF, hc, Jx, Jc, de, vals)
        out = [torch.zeros_like(a) for a in (x, r, lam, lam)]
        hipldl.trial_point_dev(L, x, r, lam, d, 1e4, *out)
        rhs = torch.zeros((B, s.N), dtype=torch.float32, device=dev)
        nrm = torch.full((B, 2), -1.0, dtype=torch.float32, device=dev)
        hipldl.residual_vectors_dev(L, vals, r, lam, Fx, cx, rhs, nrm)
        torch.cuda.synchronize()
        v0 = R.prepare(np.full((len(probe), s.nnzNS), 7.0, np.float32), s.nvar, s.nequ, s.ncon, s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc,
                       c(hF), c(hc), c(Jx), c(Jc), c(de))
        assert _same(c(vals), v0)
        xt0, rt0, lt0, dl0 = R.trial_point(s.nvar, s.nequ, s.ncon, c(x), c(r), c(lam), c(d), 1e4)
        assert _same(c(out[0]), xt0) and _same(c(out[1]), rt0)
        assert np.all(np.abs(c(out[3]) - dl0) <= 4 * EPS32 * np.abs(dl0))
        assert np.all(np.abs(c(out[2]) - lt0) <= 4 * EPS32 * (np.abs(c(lam)) + np.abs(dl0)))
        rhs0, nrm0 = R.residual_vectors(rows, cols, c(vals), s.nvar, s.nequ, s.ncon, c(r), c(lam), c(Fx), c(cx))
        assert _same(c(rhs), rhs0) and _same(c(nrm), nrm0), tiles
        L.close()
        del vals, rhs, nrm, out
