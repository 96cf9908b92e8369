"""The inputs of tests/test_rows_f1_f2_gpu.py, checked without a GPU (tests/support/rows_f1_f2_cases.py): the GPU tests must neither
fail on their inputs nor pass on them.

The constants parsed from csrc/kernels.h are the ones the cases were designed for; every pattern has the windows, the longest column,
the `own` decision and the number of primal tiles it is named for (by the restated host rule `tiles`); the rows where the GPU tests
put a NaN are read only by tail entries; the restatements of rows f1 and f2 are oracle.residual_vectors / oracle.prepare bit for bit
in float64 and f32_rows.residual_vectors / f32_rows.prepare in float32, and meet the bound of recursive summation against the exact
sums; the f2 generator puts every offset where its case says, and the band shapes of the interleaved cases fall on and beside the
tile multiples.
"""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from oracle import oracle as O
from tests.support import f32_rows as R
from tests.support import rows_f1_f2_cases as K

IDS = {np.float64: "f64", np.float32: "f32"}
both_types = pytest.mark.parametrize("dtype", K.DTYPES, ids=[IDS[t] for t in K.DTYPES])


def _same(a, b):
    """bit-equal arrays of one element type, NaN where the other has NaN (any payload)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    z = a.dtype.type(0)
    return np.array_equal(np.where(np.isnan(a), z, a).view(u), np.where(np.isnan(b), z, b).view(u))


def test_constants_are_the_ones_the_cases_are_made_for():
    assert K.constants() == {"RVT_COLS": 256, "RVT_KF": 6, "RVT_KC": 2, "RVT_MAXF": 2046, "RVT_MAXR": 510, "RVT_MAXC": 510,
                             "RVT_MAXL": 510, "RVT_PROWS": 2048}
    assert K.MAX_COL == 255


def test_tile_rule_on_the_known_band():
    """the windows of band_structure(600, 6) and of its half-width 3 twin, computed once by hand from the host rule"""
    w = lambda s: [(d["wF"], d["wR"], d["wC"], d["wL"]) for d in K.tiles(s)["tiles"]]   # noqa: E731
    assert w(K.band(600, 6, 2)) == [(1283, 258, 256, 3), (1292, 260, 256, 4), (443, 90, 88, 1)]
    assert [x[0] for x in w(K.band(600, 6, 3))] == [1801, 1822, 625]


@pytest.mark.parametrize("which", "FRCL")
def test_window_edges(which):
    key = {"F": "wF", "R": "wR", "C": "wC", "L": "wL"}[which]
    lim = K.limit(which)
    for d, tiled in ((-1, True), (0, True), (1, False)):
        s = K.pattern(f"edge-{which}-{lim + d}")
        T = K.tiles(s)
        assert len(T["tiles"]) == 1 and T["tiles"][0][key] == lim + d, (which, d)
        assert T["tiled"] == tiled == K.predict(s)["f1_tiles"]
        for k2, w2 in (("wF", "F"), ("wR", "R"), ("wC", "C"), ("wL", "L")):     # every other window is within its limit
            assert k2 == key or T["tiles"][0][k2] <= K.limit(w2) - 1
        if tiled:
            assert T["own"] and T["primal_tiles"] == 0
        # the window starts at every position of a 16-byte chunk, in either element type, within the three problems of the test and the
        # caller offsets it gives the window's array (every array as a sub-view at every offset; nnz = 3 (mod 4) moves the windows
        # of vals from problem to problem besides); at the limit the largest chunk count the kernel can meet is among them:
        # (limit + 2 (E - 1)) // E
        assert s.nnzNS % 4 == 3
        for dtype in K.DTYPES:
            E = K.chunk_elems(dtype)
            seen = K.chunk_visits(s, which, dtype)
            assert {p for p, _ in seen} == set(range(E)), (which, d, dtype, seen)
            if d == 0:
                assert max(n for _, n in seen) == (lim + 2 * (E - 1)) // E == {2: {2046: 1024, 510: 256}, 4: {2046: 513, 510: 129}}[E][lim]
        # both ends of the window are read from LDS (by an entry the table holds), not through the index lists of a long column
        if tiled:
            keep = K.constants()["RVT_KF" if which in "FR" else "RVT_KC"]
            assert max(K.window_ends(s, which)) < keep, K.window_ends(s, which)
    assert K.pattern(f"edge-{which}-{lim}").nvar == K.constants()["RVT_COLS"]


def test_two_tile_edge():
    T = K.tiles(K.pattern("two-tile-edge"))
    t0, t1 = T["tiles"]
    assert t1["wF"] == K.limit("F") and t0["wF"] <= K.limit("F") // 4 and T["tiled"] and K.pattern("two-tile-edge").nnzNS % 4 == 3
    assert K.window_ends(K.pattern("two-tile-edge"), "F", 1) == (0, 0) and t1["fslo"] % 4 == 0
    for dtype in K.DTYPES:
        E = K.chunk_elems(dtype)
        seen = K.chunk_visits(K.pattern("two-tile-edge"), "F", dtype, t=1)
        assert {p for p, _ in seen} == set(range(E)) and max(n for _, n in seen) == (K.limit("F") + 2 * (E - 1)) // E
    even = lambda w: (w + 3) & ~1   # noqa: E731
    assert T["lds"] == even(t1["wF"]) + even(t1["wR"]) + 2 * even(0) > even(t0["wF"]) + even(t0["wR"]) + 2 * even(0)


@pytest.mark.parametrize("name", K.LONG_NAMES)
def test_long_columns(name):
    s, T, C = K.pattern(name), K.tiles(K.pattern(name)), K.constants()
    (ptrF, _, _), (ptrC, _, _) = K.columns(name)
    if name.startswith("band"):
        hw = int(name.split("-")[3])
        assert T["nF"] == 2 * hw + 1 and T["tiled"] == (hw == 3) and len(T["tiles"]) == 3
        # the last row: column n - hw - 1 reads it through its last entry (rank 2 hw: a tail entry)
        c, rk = K.readers(s, "F", s.nequ - 1)
        assert (s.nvar - hw - 1, 2 * hw) in set(zip(c.tolist(), rk.tolist())) and 2 * hw >= C["RVT_KF"]
        return
    over = name == "long-over"
    lens_f, lens_c = set(np.diff(ptrF).tolist()), set(np.diff(ptrC).tolist())
    M = K.MAX_COL
    assert lens_f == (set(K.F_LENS) - ({M} if over else set())) | ({M + 1} if over else set()) and lens_c == set(K.C_LENS)
    assert T["nF"] == (M + 1 if over else M) and T["nC"] == 9 and T["tiled"] == (not over)
    assert len(T["tiles"]) == (s.nvar + 255) // 256
    # the rows where the NaN goes: read by tail entries only, and by some
    row, con = K.nan_rows(name)
    for kind, r, keep in (("F", row, C["RVT_KF"]), ("C", con, C["RVT_KC"])):
        c, rk = K.readers(s, kind, r)
        assert len(c) > 0 and (rk >= keep).all(), (kind, rk.min())
    # a column's entries are not in row order (the COO order of the sum is not the sorted one)
    (_, _, idxF), _ = K.columns(name)
    assert any(np.any(np.diff(idxF[ptrF[c]:ptrF[c + 1]]) < 0) for c in range(s.nvar))


@pytest.mark.parametrize("name", K.PRIMAL_NAMES)
def test_primal_tile_patterns(name):
    s, T = K.pattern(name), K.tiles(K.pattern(name))
    assert T["tiled"] and K.predict(s)["f1_tiles"]
    t = T["tiles"]
    if name.startswith("unordered"):
        assert len(t) == 3 and t[1]["rlo"] + t[1]["wR"] <= t[0]["rlo"]      # tile 1's rows lie below tile 0's
        assert not T["own"] and T["primal_tiles"] == {2047: 1, 2048: 1, 2049: 2}[s.nequ] and T["nF"] > K.constants()["RVT_KF"]
    elif name == "gap-F":
        assert t[1]["wF"] == 0 and t[1]["wR"] == 0 and t[0]["wF"] > 0 and t[2]["wF"] > 0 and not T["own"] and T["primal_tiles"] == 1
    elif name == "gap-C":
        assert t[1]["wC"] == 0 and t[1]["wL"] == 0 and t[0]["wC"] > 0 and t[2]["wC"] > 0 and s.ncon > 0
        assert T["own"] and T["primal_tiles"] == 0      # (this one keeps its rows: w_C == 0 in one workgroup of the owning path)
    else:
        (_, _, idxF), _ = K.columns(name)
        missing = 0 if name.endswith("first") else s.nequ - 1
        assert len(t) == 1 and set(range(s.nequ)) - set(idxF.tolist()) == {missing} and not T["own"] and T["primal_tiles"] == 1
    if not T["own"]:
        assert all(d["own_lo"] == d["own_hi"] == 0 for d in t)


def test_gather_and_refusal_patterns():
    s = K.pattern("scattered")
    (ptrF, _, _), (ptrC, _, _) = K.columns("scattered")
    assert not K.tiles(s)["tiled"] and (np.diff(ptrF) == 0).sum() >= 20 and (np.diff(ptrC) == 0).any() and K.predict(s)["jac"]
    assert K.predict(K.pattern("shuffled-kkt")) == {"f1_tiles": False, "jac": False}
    for name in K.f1_names():
        if name != "shuffled-kkt":
            assert K.predict(K.pattern(name))["jac"], name


def test_batches_sit_on_the_switch_points_of_problems_per_workgroup():
    """1, 2, then 4 (double) or 8 (float) problems per workgroup from 64 and 512 problems on; 519 leaves a ragged last group for both"""
    assert {63, 64, 65, 511, 512, 513} <= set(K.PB_BATCHES) and 519 % 4 != 0 and 519 % 8 != 0 and 65 % 2 == 1
    for name in K.PB_NAMES:
        assert len(K.tiles(K.pattern(name))["tiles"]) == 3
    assert K.pattern("band-600-6-3").N == 1206 and K.tiles(K.pattern("unordered-2049"))["primal_tiles"] == 2


@both_types
@pytest.mark.parametrize("name", K.f1_names())
def test_f1_restatement(name, dtype):
    """the restatement in `dtype` is the named reference's (oracle: float64, problem by problem; f32_rows: float32) and lies within the
    bound of recursive summation of the exact sums"""
    s, m, vals = K.f1_case(name, 3, dtype)
    rhs, nrm = K.restate_f1(s, vals, m["r"], m["lam"], m["Fx"], m["cx"])
    assert rhs.dtype == dtype and nrm.dtype == dtype and rhs.shape == (3, s.N)
    rows, cols = K.kkt(s)
    if dtype == np.float32:
        rhs0, nrm0 = R.residual_vectors(rows, cols, vals, s.nvar, s.nequ, s.ncon, m["r"], m["lam"], m["Fx"], m["cx"])
        assert _same(rhs, rhs0) and _same(nrm, nrm0)
    else:
        for b in (0, 2):
            rhs0, nrm0 = O.residual_vectors(rows, cols, vals[b], s.nvar, s.nequ, s.ncon, m["r"][b], m["lam"][b], m["Fx"][b], m["cx"][b])
            assert _same(rhs[b], rhs0) and _same(nrm[b], np.array(nrm0)), b
    exact, bound = K.dual_bound(s, vals, m["r"], m["lam"])
    assert np.all(np.abs(rhs[:, :s.nvar].astype(K.LD) - exact) <= bound)
    assert (bound > 0).any() and np.all(bound[exact != 0] < np.abs(exact[exact != 0]).max())


@both_types
def test_norm_variants(dtype):
    s = K.pattern("band-600-6-3")
    m = K.model(s, 6, dtype, 3)
    v = {n: i for i, n in enumerate(K.norm_variants(s, m))}
    vals = K.vals_of(s, m)
    rhs, nrm = K.restate_f1(s, vals, m["r"], m["lam"], m["Fx"], m["cx"])
    dual, primal = rhs[:, :s.nvar], rhs[:, s.nvar:]
    zero = np.zeros(1, dtype)
    assert not dual[v["zero"]].any() and _same(nrm[v["zero"], :1], zero)
    assert not dual[v["minus-zero"]].any() and np.signbit(primal[v["minus-zero"]]).all() and _same(nrm[v["minus-zero"]], np.zeros(2, dtype))
    assert np.isinf(dual[v["inf"]]).any() and not np.isnan(dual[v["inf"]]).any() and np.isposinf(nrm[v["inf"]]).all()
    assert {np.inf, -np.inf} <= set(dual[v["inf"]][np.isinf(dual[v["inf"]])].tolist())
    assert np.isinf(dual[v["nan-beside-inf"]]).any() and np.isnan(nrm[v["nan-beside-inf"]]).all()
    assert np.argmax(np.abs(dual[v["last-tile"]])) >= 512 and s.nvar - 512 < 256
    assert np.argmax(np.abs(primal[v["c-part"]])) == s.nequ + s.ncon - 1 and nrm[v["c-part"], 1] == 50


@both_types
def test_f2_generator_hits_the_named_offsets(dtype):
    C = K.chunk(dtype)
    cases = K.offset_cases(dtype)
    for i in range(1, 7):
        got = {K.offsets_of(cases[n])[i - 1] % C for n in cases if n.startswith(f"o{i}@") and "C" in n}
        assert got == {C - 1, 0, 1}, (i, got)
        rows = {K.offsets_of(cases[n])[i - 1] % 256 for n in cases if n.startswith(f"o{i}@row")}
        assert rows == {255, 1}, (i, rows)
        assert all(K.offsets_of(cases[n])[i - 1] >= C - 1 for n in cases if n.startswith(f"o{i}@") and "C" in n)
    assert [sum(cases[f"nnz@{t}"]) for t in ("C-1", "C", "C+1", "2C+1")] == [C - 1, C, C + 1, 2 * C + 1]
    assert cases["ncon=0"][1] == cases["ncon=0"][3] == cases["ncon=0"][5] == 0 and cases["nnzhF=0"][0] == 0
    for name, counts in cases.items():
        s = K.segment_pattern(counts)
        assert K.counts_of(s) == counts and s.nnzNS == sum(counts), name
        rows, cols = s.kkt_pattern()
        assert (rows >= cols).all(), name    # lower triangle
        for a in (s.hF, s.hc, s.jF, s.jc):     # no entry twice inside a segment
            assert len(set(zip(np.asarray(a[0]).tolist(), np.asarray(a[1]).tolist()))) == len(a[0]), name


@both_types
def test_prepare_restatement(built, dtype):
    """restate_prepare is oracle.prepare (float64, problem by problem) and f32_rows.prepare (float32), with and without a Hessian"""
    for name in ("o3@1C", "ncon=0", "nnzhF=0"):
        counts = K.offset_cases(dtype)[name]
        s = K.segment_pattern(counts)
        m = K.model(s, 5, dtype, 2)
        old = np.random.default_rng(1).standard_normal((5, s.nnzNS)).astype(dtype)
        for hess in (True, False):
            got = K.restate_prepare(old, counts, m, dtype, hess)
            hF = m["hF"] if hess else None
            if dtype == np.float32:
                want = R.prepare(old, s.nvar, s.nequ, s.ncon, *counts[:4], hF, m["hc"], m["Jx"], m["Jcx"], m["delta"])
            else:
                want = old.copy()
                for b in range(5):
                    O.prepare(want[b], s.nvar, s.nequ, s.ncon, *counts[:4], None if hF is None else hF[b], m["hc"][b] if s.ncon else None,
                              m["Jx"][b], m["Jcx"][b] if s.ncon else None, float(m["delta"][b]))
            assert _same(got, want), (name, hess)
            o = K.offsets_of(counts)
            assert _same(got[:, o[3]:o[4]], old[:, o[3]:o[4]]) and not got[:, o[5]:].any() and not np.signbit(got[:, o[5]:]).any()
            if s.ncon:
                assert np.signbit(got[3, o[4]]) and got[3, o[4]] == 0 and np.signbit(got[0, o[0]]) and got[0, o[0]] == 0   # -delta, -hc: -0.0


@both_types
def test_interleaved_shapes(dtype):
    """the band shapes of the prepare_il cases: every offset and nnz within one element of a multiple of the tile in some shape, o1, o3,
    o5, o6 and nnz on one exactly (o2 = 4 n - 3 and o4 = 10 n - 9 are odd); the lengths of the conversion cases are N = 2 n + p"""
    shapes, got = K.il_shapes(dtype)
    T = K.il_tile(dtype)
    assert {i for i, _ in got} == set(range(1, 8)) and {(1, 0), (3, 0), (5, 0), (6, 0), (7, 0)} <= got
    for n, p in shapes:
        s = K.band(n, p)
        assert K.counts_of(s) == K.band_counts(n, p)
        assert any((x - d) % T == 0 for x in K.offsets_of(K.band_counts(n, p)) for d in (-1, 0, 1))
    for length, (n, p) in K.IL_LENGTHS.items():
        assert K.band(n, p).N == length
    assert {127, 128, 129, 1025} <= set(K.IL_LENGTHS) and {7, 0, 1} <= {x % 8 for x in K.IL_LENGTHS if x < 127}
    assert min(n for n, _ in K.IL_LENGTHS.values()) == 12          # the smallest order the band kernels take
    from cannoles_jl_amd import hipldl
    p, e = np.meshgrid(np.arange(70), np.arange(129), indexing="ij")
    assert np.array_equal(K.il_index(p, e, 129), hipldl.il_index(p, e, 129)) and K.il_len(70, 129) == hipldl.il_len(70, 129)
    assert len(np.unique(K.il_index(p, e, 129))) == p.size and K.il_index(p, e, 129).max() < K.il_len(70, 129)
