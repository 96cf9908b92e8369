"""Rows f1 (`residual_vectors_tiled_kernel`, `residual_vectors_kernel`) and f2 (`prepare_kernel`, `prepare_il_kernel`) and the layout
conversions (`interleave_kernel`) at every window, tile and segment edge, in both element types, through hipldl's wrappers on the cases
of tests/support/rows_f1_f2_cases.py (tests/test_rows_f1_f2_cpu.py checks those inputs without a GPU).  -m gpu.

Row f1, both kernels (Options(f1_tiles=1 | 0)); every case first asserts which kernel serves it, config["f1_tiles"], against the
restated host rule: windows at limit - 1, limit, limit + 1 (tiled, tiled, gather), also in a tile that is not the first; columns of
0, 1, 5, 6, 7, 13, 255 (J_F) and 0, 1, 2, 3, 9 (J_c) entries — empty, exactly full and overfull table rows — at nvar = 255, 256, 257,
600, the half-width 3 band, and 256 entries (gather); a NaN that only a tail entry reads; primal tiles (unordered row ranges, a tile
without J_F entries, an uncovered first or last row; one and two primal tiles, the last one partial) and a tile without J_c entries;
every array at every position inside a 16-byte chunk, NaN around it and in every slot of `vals` that row f1 must not read; 1, 63, 64,
65, 511, 512, 513, 519 problems (1, 2, 4 or 8 problems per workgroup, ragged last groups) with the rows beyond the active count
untouched; the rules of the two norms; the `_jac` twin wherever it is served, its refusal where the Jacobian slots are not one run.
Row f2: every segment offset on and beside a chunk boundary and a thread-row boundary, nnz either side of whole chunks, no
constraints, no Hessian entries, no Hessian array, from random `vals`; the interleaved kernel on band shapes whose offsets fall on and
beside its tiles, checked on the raw buffer element for element; the conversions at the block and tile edges with active prefixes.

What is held to what.  Bit-equal, NaN for NaN: everything, to the restatements of rows_f1_f2_cases (which the CPU tests hold bit-equal
to oracle.residual_vectors / oracle.prepare in float64 and f32_rows.residual_vectors / f32_rows.prepare in float32); the two kernels
and the twin to each other.  And one judge formed in longdouble from the inputs alone (rows_f1_f2_cases.dual_bound): every finite dual
entry within (nF + nC + 1) eps sum|terms| of the exact sum — the bound of recursive summation, which a mistake shared by kernel and
restatement does not pass.  Every output array has a guard row either side; `norms` starts from -1.

Not built: interleaved arrays of 1, 7, 8 and 9 elements per problem (the band kernels, which alone take the interleaved layout, start
at nvar = 12, N = 24: the lengths here are 24, 25 and, for 7, 8 and 9 elements in the last block of eight, 31, 32, 33).
"""
import numpy as np
import pytest

from tests.support import rows_f1_f2_cases as K

pytestmark = pytest.mark.gpu

IDS = {np.float64: "f64", np.float32: "f32"}
both_types = pytest.mark.parametrize("dtype", K.DTYPES, ids=[IDS[t] for t in K.DTYPES])
both_kernels = pytest.mark.parametrize("tiles", [1, 0], ids=["tiles", "gather"])
GUARD = 7.5
CNL_ERR_STATE = 5


def _mods():
    import torch
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl
    return torch, hipldl


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _tt(torch, dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _same(a, b):
    """bit-equal arrays of one element type, NaN where the other has NaN (any payload)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    z = a.dtype.type(0)
    return np.array_equal(np.where(np.isnan(a), z, a).view(u), np.where(np.isnan(b), z, b).view(u))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _handle(hipldl, s, B, dtype, **opt):
    """a handle of the element type on the pattern's KKT entries (Float32: the general kernels for the patterns the band kernels do
    not serve)"""
    rows, cols = K.kkt(s)
    if dtype == np.float32 and not opt.get("batch_layout"):
        opt = dict(opt, float32_general=1)
    return hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=dtype, options=hipldl.Options(**opt) if opt else None)


class Guarded:
    """a device array [B][n] with a guard row either side"""

    def __init__(self, torch, B, n, dtype, fill=GUARD):
        self.B, self.fill, self.n = B, fill, n
        self.all = torch.full((B + 2, max(n, 1)), fill, dtype=_tt(torch, dtype), device=torch.device("cuda", 0))
        self.t = self.all[1:B + 1]

    def get(self, nb=None):
        """the first nb rows of the batch, after checking that the guard rows and the rows beyond nb are intact, bit for bit"""
        nb = self.B if nb is None else nb
        a = self.all.cpu().numpy()
        rest = np.concatenate([a[:1], a[nb + 1:]])
        assert np.array_equal(_bits(rest), _bits(np.full_like(rest, self.fill))), "a guard row, or a row beyond the active problems, was written"
        return a[1:nb + 1, :self.n]


def _f1(torch, hipldl, L, s, dtype, t, B, nb=None, jac=True):
    """row f1 on the device arrays t (vals, r, lam, Fx, cx, Jx, Jcx: tensors or addresses) into guarded outputs; the `_jac` twin where the
    pattern has one, bit-equal, and refused with CNL_ERR_STATE where not.  Returns (rhs, norms) of the first nb problems."""
    p = s.ncon
    lam, cx, Jcx = (t["lam"], t["cx"], t["Jcx"]) if p else (0, 0, 0)
    rhs, nrm = Guarded(torch, B, s.N, dtype), Guarded(torch, B, 2, dtype, -1.0)
    hipldl.residual_vectors_dev(L, t["vals"], t["r"], lam, t["Fx"], cx, rhs.t, nrm.t)
    rhs2, nrm2 = Guarded(torch, B, s.N, dtype), Guarded(torch, B, 2, dtype, -1.0)
    if jac:
        hipldl.residual_vectors_jac_dev(L, s.nnzjF, s.nnzjc, t["Jx"], Jcx, t["r"], lam, t["Fx"], cx, rhs2.t, nrm2.t)
    else:
        with pytest.raises(hipldl.CnlError) as e:
            hipldl.residual_vectors_jac_dev(L, s.nnzjF, s.nnzjc, t["Jx"], Jcx, t["r"], lam, t["Fx"], cx, rhs2.t, nrm2.t)
        assert e.value.code == CNL_ERR_STATE
    torch.cuda.synchronize()
    out = rhs.get(nb), nrm.get(nb)
    if jac:
        assert _same(rhs2.get(nb), out[0]) and _same(nrm2.get(nb), out[1]), "the `_jac` twin differs"
    else:
        rhs2.get(0), nrm2.get(0)
    return out


def _tensors(torch, m, vals):
    return dict({k: _dev(torch, m[k]) for k in ("r", "lam", "Fx", "cx", "Jx", "Jcx")}, vals=_dev(torch, vals))


def _judge(s, vals, m, dual):
    """every finite dual entry within the bound of recursive summation of the exact sum (rows_f1_f2_cases.dual_bound)"""
    with np.errstate(invalid="ignore", over="ignore"):
        exact, bound = K.dual_bound(s, vals, m["r"], m["lam"])
        ok = np.isfinite(dual) & np.isfinite(exact.astype(np.float64))
        assert ok.any() and np.all(np.abs(dual.astype(K.LD) - exact)[ok] <= bound[ok])


def _run_case(name, dtype, tiles, B, m=None, vals=None, judge=True):
    """one f1 case on a fresh handle: the serving kernel against the prediction, both entry points, the restatement, the judge"""
    torch, hipldl = _mods()
    if m is None:
        s, m, vals = K.f1_case(name, B, dtype)
    s = K.pattern(name)
    pred = K.predict(s)
    L = _handle(hipldl, s, B, dtype, f1_tiles=tiles)
    assert L.config["f1_tiles"] == (bool(tiles) and pred["f1_tiles"]) and L.config["float32"] == (dtype == np.float32), L.config
    rhs, nrm = _f1(torch, hipldl, L, s, dtype, _tensors(torch, m, vals), B, jac=pred["jac"])
    L.close()
    want = K.restate_f1(s, vals, m["r"], m["lam"], m["Fx"], m["cx"])
    assert _same(rhs, want[0]), np.argwhere(_bits(np.nan_to_num(rhs)) != _bits(np.nan_to_num(want[0])))[:8]
    assert _same(nrm, want[1]), (nrm, want[1])
    if judge:
        _judge(s, vals, m, rhs[:, :s.nvar])
    return rhs, nrm


# ---- row f1 -----------------------------------------------------------------------------------------------------------------------------
def _offset_copy(torch, a, k):
    """the array inside a larger buffer, k elements behind its (256-byte aligned) start, NaN around it: (buffer, address)"""
    buf = torch.full((a.size + 16,), float("nan"), dtype=_tt(torch, a.dtype.type), device=torch.device("cuda", 0))
    if a.size:
        buf[k:k + a.size] = _dev(torch, a.ravel())
    assert buf.data_ptr() % 256 == 0
    return buf, buf.data_ptr() + k * a.itemsize


@both_types
@both_kernels
@pytest.mark.parametrize("name", K.edge_names())
def test_f1_windows_at_their_limits(built, name, tiles, dtype):
    """B = 3, every input as a whole allocation and as a sub-view at each other position of a 16-byte chunk (NaN around it): with the
    row stride nnz = 3 (mod 4) of `vals`, and with the offsets for r and lambda — whose row stride at W_R = nequ, W_L = ncon is the even
    window itself — every window starts at every position of its first chunk, and at the limit takes the largest chunk count the kernel
    can meet (rows_f1_f2_cases.chunk_visits, asserted on the CPU).  Bit-equal to the restatement at every offset."""
    torch, hipldl = _mods()
    B = 3
    s, m, vals = K.f1_case(name, B, dtype)
    pred = K.predict(s)
    L = _handle(hipldl, s, B, dtype, f1_tiles=tiles)
    assert L.config["f1_tiles"] == (bool(tiles) and pred["f1_tiles"]) and L.config["float32"] == (dtype == np.float32), L.config
    want = K.restate_f1(s, vals, m["r"], m["lam"], m["Fx"], m["cx"])
    host = dict(m, vals=vals)
    for k in K.edge_offsets(s.meta.get("which", "F"), dtype):
        held = {key: _offset_copy(torch, host[key], k) for key in ("vals", "r", "lam", "Fx", "cx", "Jx", "Jcx")}
        rhs, nrm = _f1(torch, hipldl, L, s, dtype, {key: v[1] for key, v in held.items()}, B, jac=pred["jac"])
        assert _same(rhs, want[0]), (k, np.argwhere(_bits(rhs) != _bits(want[0]))[:8])
        assert _same(nrm, want[1]), (k, nrm, want[1])
    L.close()
    _judge(s, vals, m, rhs[:, :s.nvar])


@both_types
@both_kernels
@pytest.mark.parametrize("name", K.LONG_NAMES)
def test_f1_long_and_empty_columns(built, name, tiles, dtype):
    """a NaN in r (problem 2) and in lambda (problem 3) in a row that tail entries read: it reaches exactly the columns that read the
    row, and the dual norm"""
    s, m0, _ = K.f1_case(name, 5, dtype)
    m = {k: v.copy() for k, v in m0.items()}
    row, con = K.nan_rows(name)
    m["r"][2, row] = np.nan
    m["lam"][3, con] = np.nan
    rhs, nrm = _run_case(name, dtype, tiles, 5, m, K.vals_of(s, m))
    for b, kind, r in ((2, "F", row), (3, "C", con)):
        hit = np.zeros(s.nvar, bool)
        hit[K.readers(s, kind, r)[0]] = True
        assert hit.any() and np.array_equal(np.isnan(rhs[b, :s.nvar]), hit) and np.isnan(nrm[b, 0]), (b, kind)
    assert np.isfinite(rhs[[0, 1, 4]]).all() and np.isfinite(nrm[[0, 1, 4]]).all() and np.isnan(nrm[2, 1]) and np.isfinite(nrm[3, 1])


@both_types
@both_kernels
@pytest.mark.parametrize("B", [2, 67])
@pytest.mark.parametrize("name", K.PRIMAL_NAMES)
def test_f1_primal_tiles(built, name, B, tiles, dtype):
    """the patterns whose tiles do not own the primal rows (held by the restated host rule on the CPU); a NaN in F in the last primal
    row of the last problem reaches the primal norm of that problem alone"""
    s, m0, _ = K.f1_case(name, B, dtype)
    m = {k: v.copy() for k, v in m0.items()}
    m["Fx"][B - 1, s.nequ - 1] = np.nan
    rhs, nrm = _run_case(name, dtype, tiles, B, m, K.vals_of(s, m))
    assert np.isnan(rhs[B - 1, s.nvar + s.nequ - 1]) and np.isnan(nrm[B - 1, 1]) and np.isnan(rhs).sum() == 1 and np.isnan(nrm).sum() == 1


ALIGN_KEYS = ("vals", "r", "lam", "Fx", "cx", "Jx", "Jcx")
ALIGN_COMBOS = {np.float64: [(1,) * 7, (1, 0, 1, 0, 1, 0, 1), (0, 1, 0, 1, 0, 1, 0), (1, 1, 0, 0, 0, 1, 1), (0, 0, 1, 1, 1, 0, 0)],
                np.float32: [(1,) * 7, (3,) * 7, (2,) * 7, (1, 2, 3, 0, 1, 2, 3), (2, 3, 1, 3, 0, 1, 2), (3, 0, 2, 1, 3, 3, 1), (0, 1, 0, 2, 2, 0, 3)]}


@both_types
@both_kernels
@pytest.mark.parametrize("name", K.ALIGN_NAMES)
def test_f1_caller_alignment(built, name, tiles, dtype):
    """every input as a sub-view of a larger allocation, at every position inside a 16-byte chunk (independently per array; one
    combination has every array odd), NaN in the elements around it: bit-equal to the call on whole allocations"""
    torch, hipldl = _mods()
    B = 3
    s, m, vals = K.f1_case(name, B, dtype)
    pred = K.predict(s)
    L = _handle(hipldl, s, B, dtype, f1_tiles=tiles)
    assert L.config["f1_tiles"] == (bool(tiles) and pred["f1_tiles"])
    host = dict(m, vals=vals)
    base = _f1(torch, hipldl, L, s, dtype, _tensors(torch, m, vals), B)
    want = K.restate_f1(s, vals, m["r"], m["lam"], m["Fx"], m["cx"])
    assert _same(base[0], want[0]) and _same(base[1], want[1])
    for combo in ALIGN_COMBOS[dtype]:
        held = {k: _offset_copy(torch, host[k], o) for k, o in zip(ALIGN_KEYS, combo)}
        got = _f1(torch, hipldl, L, s, dtype, {k: v[1] for k, v in held.items()}, B)
        assert _same(got[0], base[0]) and _same(got[1], base[1]), combo
    # NaN in every slot of vals that is not a Jacobian entry (H_F, H_c, -I, -delta I, rho I): nothing changes
    off = s.offsets()
    dirty = np.full_like(vals, np.nan)
    dirty[:, off[2]:off[4]] = vals[:, off[2]:off[4]]
    t = _tensors(torch, m, dirty)
    got = _f1(torch, hipldl, L, s, dtype, t, B)
    L.close()
    assert _same(got[0], base[0]) and _same(got[1], base[1])


@both_types
@both_kernels
@pytest.mark.parametrize("name", K.PB_NAMES)
def test_f1_problems_per_workgroup(built, name, tiles, dtype):
    """1, 63, 64, 65, 511, 512, 513 and 519 problems on three tiles (and primal tiles): one handle of 519 problems working on a prefix
    (cnl_set_active_batch) where the handle can, a handle of its own otherwise; every problem against the restatement (each has numbers
    of its own), the rows beyond the active count untouched"""
    torch, hipldl = _mods()
    Bmax = max(K.PB_BATCHES)
    s, m, vals = K.f1_case(name, Bmax, dtype)
    want = K.restate_f1(s, vals, m["r"], m["lam"], m["Fx"], m["cx"])
    assert len(np.unique(want[1][:, 0])) == Bmax      # no two problems alike
    t = _tensors(torch, m, vals)
    L = _handle(hipldl, s, Bmax, dtype, f1_tiles=tiles)
    assert L.config["f1_tiles"] == bool(tiles)
    staged = L.config["kernel"] == "v2-staged"
    assert staged == (dtype == np.float64 and name == "band-600-6-3"), L.config
    prefixes = 0
    for nb in sorted(K.PB_BATCHES, reverse=True):
        try:
            hipldl.set_active_batch(L, nb)
            H, prefixes = L, prefixes + (nb < Bmax)
        except hipldl.CnlError as e:      # (a staged Float64 handle is sized by its created batch)
            assert e.code == CNL_ERR_STATE
            H = _handle(hipldl, s, nb, dtype, f1_tiles=tiles)
            assert H.config["f1_tiles"] == bool(tiles)
        rhs, nrm = _f1(torch, hipldl, H, s, dtype, t, Bmax, nb=nb)
        if H is not L:
            H.close()
        assert _same(rhs, want[0][:nb]) and _same(nrm, want[1][:nb]), nb
    L.close()
    # a staged handle (the Float64 one of the band) is sized by its created batch and refuses every prefix; every other handle
    # here — the Float32 general ones, the Float64 general one of 519 unordered problems — works on all of them
    assert prefixes == (0 if staged else len(K.PB_BATCHES) - 1), (staged, prefixes)
    _judge(s, vals[:8], {k: v[:8] for k, v in m.items()}, want[0][:8, :s.nvar])


@both_types
@both_kernels
def test_f1_norms(built, tiles, dtype):
    """all-zero dual (+0.0, not the -1 the array starts from), a primal part of -0.0 only (+0.0), +-inf, NaN beside inf (NaN wins), the
    largest dual entry in the last, partial tile, the largest primal entry in the c part"""
    name = "band-600-6-3"
    s = K.pattern(name)
    m = K.model(s, 6, dtype, 3)
    v = {n: i for i, n in enumerate(K.norm_variants(s, m))}
    rhs, nrm = _run_case(name, dtype, tiles, 6, m, K.vals_of(s, m))
    zero = _bits(np.zeros(2, dtype))
    assert np.array_equal(_bits(nrm[v["zero"], :1]), zero[:1]) and np.array_equal(_bits(nrm[v["minus-zero"]]), zero)
    assert np.isposinf(nrm[v["inf"]]).all() and np.isnan(nrm[v["nan-beside-inf"]]).all()
    assert nrm[v["last-tile"], 0] == np.abs(rhs[v["last-tile"], 512:s.nvar]).max() > np.abs(rhs[v["last-tile"], :512]).max()
    assert nrm[v["c-part"], 1] == 50


@both_types
@both_kernels
@pytest.mark.parametrize("name", K.OTHER_NAMES)
def test_f1_gather_patterns_and_the_refusal_of_the_twin(built, name, tiles, dtype):
    """empty columns in the gather kernel (its loads of absent entries); KKT entries in shuffled order: the gather kernel serves
    residual_vectors_dev, the `_jac` twin answers CNL_ERR_STATE and writes nothing"""
    assert not K.predict(K.pattern(name))["f1_tiles"] and K.predict(K.pattern(name))["jac"] == (name == "scattered")
    _run_case(name, dtype, tiles, 5)


# ---- row f2 -----------------------------------------------------------------------------------------------------------------------------
def _prepare_args(torch, s, m, hess, dummy):
    """(nnzhF, nnzhc, nnzjF, nnzjc, hF, hc, Jx, Jcx, delta) for prepare_newton_system_dev; without constraints hc / Jcx are null, hF is
    a valid address even where it has no element"""
    t = {k: _dev(torch, m[k]) for k in ("hF", "hc", "Jx", "Jcx", "delta")}
    hF = (t["hF"] if s.nnzhF else dummy) if hess else 0
    return (s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, hF, t["hc"] if s.ncon else 0, t["Jx"], t["Jcx"] if s.ncon else 0, t["delta"]), t


def _check_prepared(s, got, old, want, hess):
    """bit for bit (and so sign bit for sign bit) the restatement; the slots the rule leaves alone keep their bits; rho I is +0.0"""
    o = [0] + K.offsets_of(K.counts_of(s))
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:8]
    assert np.array_equal(_bits(got[:, o[4]:o[5]]), _bits(old[:, o[4]:o[5]]))                  # -I
    assert np.array_equal(_bits(got[:, o[6]:]), _bits(np.zeros_like(got[:, o[6]:])))           # rho I: +0.0
    if not hess:
        assert np.array_equal(_bits(got[:, :o[1]]), _bits(old[:, :o[1]]))
    if s.ncon:
        assert np.signbit(got[:, o[1]:o[2]:7]).all() and not got[:, o[1]:o[2]:7].any()          # -hc = -0.0 where hc = 0
        assert np.signbit(got[3 % len(got), o[5]:o[6]]).all() and not got[3 % len(got), o[5]:o[6]].any()   # -delta = -0.0


def _offset_names(dtype):
    return list(K.offset_cases(dtype))


@pytest.mark.parametrize("dtype,name", [(t, n) for t in K.DTYPES for n in _offset_names(t)],
                         ids=[f"{IDS[t]}-{n}" for t in K.DTYPES for n in _offset_names(t)])
def test_f2_segment_and_chunk_edges(built, dtype, name):
    torch, hipldl = _mods()
    counts = K.offset_cases(dtype)[name]
    s = K.segment_pattern(counts)
    dummy = torch.zeros(4, dtype=_tt(torch, dtype), device=torch.device("cuda", 0))
    for B in (1, 5):
        m = K.model(s, B, dtype, 7 + B)
        old = np.random.default_rng(B).standard_normal((B, s.nnzNS)).astype(dtype)
        L = _handle(hipldl, s, B, dtype)
        for hess in (True, False):
            args, keep = _prepare_args(torch, s, m, hess, dummy)
            v = Guarded(torch, B, s.nnzNS, dtype)
            v.t.copy_(_dev(torch, old))
            hipldl.prepare_newton_system_dev(L, *args, v.t)
            torch.cuda.synchronize()
            _check_prepared(s, v.get(), old, K.restate_prepare(old, counts, m, dtype, hess), hess)
        L.close()


def _il_handle(hipldl, s, B, dtype):
    opt = dict(batch_layout=hipldl.LAYOUT_INTERLEAVED)
    if dtype == np.float64:
        opt["plan_kind"] = hipldl.PLAN_THROUGHPUT
    L = _handle(hipldl, s, B, dtype, **opt)
    assert L.config["band"] and L.config["batch_layout"] == 1 and L.config["float32"] == (dtype == np.float32), L.config
    return L


def _padded(torch, n, dtype, fill):
    """a flat device array of n elements with 64 guard elements either side"""
    whole = torch.full((n + 128,), fill, dtype=_tt(torch, dtype), device=torch.device("cuda", 0))
    return whole, whole[64:64 + n]


def _guards_intact(whole, fill):
    a = whole.cpu().numpy()
    return np.array_equal(_bits(a[:64]), _bits(np.full_like(a[:64], fill))) and np.array_equal(_bits(a[-64:]), _bits(np.full_like(a[-64:], fill)))


@both_types
@pytest.mark.parametrize("B", [1, 31, 32, 33, 67])
def test_f2_interleaved(built, B, dtype):
    """prepare_il_kernel on band shapes whose offsets and nnz fall on and beside multiples of its tile (128 doubles, 256 floats) and of the
    blocks of eight: after deinterleave_dev the problem-major result; on the raw buffer every pad and every slot the rule leaves alone
    keeps the bits it had"""
    torch, hipldl = _mods()
    for n, p in K.il_shapes(dtype)[0]:
        s = K.band(n, p)
        counts = K.counts_of(s)
        m = K.model(s, B, dtype, 100 + n)
        old = np.random.default_rng(n).standard_normal((B, s.nnzNS)).astype(dtype)
        dummy = torch.zeros(4, dtype=_tt(torch, dtype), device=torch.device("cuda", 0))
        Lp = _handle(hipldl, s, B, dtype)
        Li = _il_handle(hipldl, s, B, dtype)
        n_il = hipldl.layout_len(Li, 0)
        assert n_il == K.il_len(B, s.nnzNS)
        pp, ee = np.meshgrid(np.arange(B), np.arange(s.nnzNS), indexing="ij")
        at = K.il_index(pp, ee, s.nnzNS)
        for hess in (True, False):
            args, keep = _prepare_args(torch, s, m, hess, dummy)
            want = K.restate_prepare(old, counts, m, dtype, hess)
            v = Guarded(torch, B, s.nnzNS, dtype)
            v.t.copy_(_dev(torch, old))
            hipldl.prepare_newton_system_dev(Lp, *args, v.t)
            whole, raw = _padded(torch, n_il, dtype, GUARD)
            hipldl.interleave_dev(Li, 0, _dev(torch, old), raw)
            torch.cuda.synchronize()
            before = raw.cpu().numpy()
            hipldl.prepare_newton_system_dev(Li, *args, raw)
            back = Guarded(torch, B, s.nnzNS, dtype)
            hipldl.deinterleave_dev(Li, 0, raw, back.t)
            torch.cuda.synchronize()
            _check_prepared(s, v.get(), old, want, hess)
            assert np.array_equal(_bits(back.get()), _bits(want)), (n, p, hess)
            expect = before.copy()
            assert np.array_equal(_bits(expect[at]), _bits(old))       # interleave_dev put `old` where band_il_index says
            expect[at] = want
            assert np.array_equal(_bits(raw.cpu().numpy()), _bits(expect)), (n, p, hess)
            assert _guards_intact(whole, GUARD)
        Lp.close()
        Li.close()


@both_types
@pytest.mark.parametrize("B", K.IL_BATCHES)
@pytest.mark.parametrize("length", list(K.IL_LENGTHS))
def test_interleave_and_back(built, length, B, dtype):
    """interleave_dev / deinterleave_dev of the N-vectors (N = length) and of `vals` of band(n, p): the interleaved buffer element for
    element by band_il_index, zeros in every pad and spare block, the round trip the identity; on a prefix of the batch the problems
    beyond it keep their bits in both directions"""
    torch, hipldl = _mods()
    n, p = K.IL_LENGTHS[length]
    s = K.band(n, p)
    assert s.N == length
    L = _il_handle(hipldl, s, B, dtype)
    rng = np.random.default_rng(length + B)
    for which, ln in ((1, s.N), (0, s.nnzNS)):
        n_il = hipldl.layout_len(L, which)
        assert n_il == K.il_len(B, ln)
        src = rng.standard_normal((B, ln)).astype(dtype)
        src[src == 0] = 1
        pp, ee = np.meshgrid(np.arange(B), np.arange(ln), indexing="ij")
        at = K.il_index(pp, ee, ln)
        for nb in [B] + [x for x in (1, 31, 33) if x < B]:
            hipldl.set_active_batch(L, nb)
            whole, raw = _padded(torch, n_il, dtype, GUARD)
            hipldl.interleave_dev(L, which, _dev(torch, src), raw)
            back = Guarded(torch, B, ln, dtype)
            hipldl.deinterleave_dev(L, which, raw, back.t)
            torch.cuda.synchronize()
            # a group of 32 problems that holds an active one: data, pads and spare block of the active problems and of the places
            # beyond the created batch are written (zeros where there is no element); the problems [nb, B) keep what the buffer
            # held, and so does every later group
            expect = np.full(n_il, GUARD, dtype)
            blocks = (ln + 7) // 8 + 1
            e = np.arange(blocks * 8)
            for q in range((nb + 31) // 32 * 32):
                if q < nb or q >= B:
                    expect[((q // 32 * blocks + e // 8) * 32 + q % 32) * 8 + e % 8] = 0
            expect[at[:nb].ravel()] = src[:nb].ravel()
            assert np.array_equal(_bits(raw.cpu().numpy()), _bits(expect)), (which, nb)
            assert _guards_intact(whole, GUARD)
            assert np.array_equal(_bits(back.get(nb)), _bits(src[:nb])), (which, nb)
        hipldl.set_active_batch(L, B)
    L.close()
