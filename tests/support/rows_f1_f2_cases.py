"""Cases for row f1 (`residual_vectors_kernel`, `residual_vectors_tiled_kernel`), row f2 (`prepare_kernel`, `prepare_il_kernel`) and the
layout conversions (`interleave_kernel`) at every window, tile and segment edge, in both element types (test infrastructure, not part of
the product).  Pure numpy; tests/test_rows_f1_f2_cpu.py checks these inputs, tests/test_rows_f1_f2_gpu.py runs them.

Constants.  The window limits, the table widths, the tile's columns and the rows of a primal tile are PARSED from csrc/kernels.h
(`constants()`), and the 255 entries a column may have at most (the byte the count occupies in a table word) from the host rule in
csrc/capi_handle.cpp (`nF > 255 || nC > 255`), so a changed constant moves the cases with it.

Tile restatement.  `tiles(s)` restates the host rule that decides, per tile of RVT_COLS columns, the four windows (slots of J_F, rows
of r, slots of J_c, rows of lambda), whether the pattern is served by the column tiles at all (every window within its limit, no column
above 255 entries), whether the tiles own the primal rows (their row ranges an ordered cover of 0 .. nequ) and otherwise how many
primal tiles follow.

Patterns (diagonal H_F and H_c: the KKT analysis is trivial, only the Jacobians vary; a synthetic.Structure each):
  band(n, p, hw)            synthetic.band_structure
  window_edge(which, width) one tile, the named window (F, R, C, L) exactly `width` elements, the others small
  two_tile_edge()           two tiles, tile 1 at the J_F limit, tile 0 small: the LDS size comes from a tile that is not the first
  long_columns(nvar)        column lengths from {0, 1, 5, 6, 7, 13, 255} (J_F) and {0, 1, 2, 3, 9} (J_c), a column's entries in shuffled
                            row order; the last residual row and the last constraint are read ONLY by tail entries (rank >= RVT_KF /
                            RVT_KC) of their columns; over=True: one column of 256 entries (gather kernel)
  unordered_rows(nequ)      three tiles whose row ranges are not an ordered cover (tile 1's rows lie below tile 0's): primal tiles
  gap_tile("F" | "C")       a tile without J_F entries between two that have some; a tile without J_c entries likewise (ncon > 0)
  uncovered_row(which)      one tile, the first or last residual row without an entry
  scattered()               entries anywhere in `vals`, empty columns: gather kernel whatever the option says
  shuffled_kkt()            a small band whose KKT entries are handed over in shuffled order: the Jacobian slots are not one run each,
                            the `_jac` twin refuses
A pattern's KKT entries are `kkt(s)`: Structure.kkt_pattern(), or the shuffled order of meta["order"].

Restatements.  `restate_f1` / `restate_prepare` are tests/support/f32_rows.py's recipes with the element type passed on: numpy in that
type, every operation rounded once, per-column sums in COO order.  The CPU tests hold them bit-equal to oracle.residual_vectors /
oracle.prepare (float64) and to f32_rows.residual_vectors / f32_rows.prepare (float32).

Judge.  `dual_bound` forms every dual entry in longdouble from the inputs alone, and the bound of recursive summation: an entry is
fl(s1 - s2) with s1, s2 recursive sums of nF, nC rounded products, so |computed - exact| <= gamma(n) sum|terms| with
n = max(nF, nC) + 1 <= nF + nC + 1 and gamma(n) = n u / (1 - n u) <= n eps (u = eps / 2, n u < 1 / 2).  The judge's own rounding
(products and sums in longdouble: the same bound with eps(longdouble)) is added; nothing else is.
"""
import functools
import os
import re

import numpy as np

from tests.support import f32_rows as R

LD = np.longdouble
DTYPES = (np.float64, np.float32)
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "cannoles.jl_amd", "csrc")


def _max_col():
    """entries of a column at most (the count is a byte of the table word): parsed from the host rule, `nF > 255 || nC > 255`"""
    with open(os.path.join(_CSRC, "capi_handle.cpp")) as f:
        m = re.search(r"\bnF\s*>\s*(\d+)\s*\|\|\s*nC\s*>\s*(\d+)", f.read())
    assert m and m.group(1) == m.group(2)
    return int(m.group(1))


MAX_COL = _max_col()



@functools.lru_cache(maxsize=None)
def constants():
    """RVT_* of csrc/kernels.h, parsed from the header text"""
    with open(os.path.join(_CSRC, "kernels.h")) as f:
        text = f.read()
    out = {}
    for name in ("RVT_COLS", "RVT_KF", "RVT_KC", "RVT_MAXF", "RVT_MAXR", "RVT_MAXC", "RVT_MAXL", "RVT_PROWS"):
        m = re.search(r"\b" + name + r"\s*=\s*(\d+)", text)
        assert m, name
        out[name] = int(m.group(1))
    return out


def limit(which):
    return constants()["RVT_MAX" + which]


# ---- patterns ------------------------------------------------------------------------------------------------------------------------
def _syn():
    from cannoles_jl_amd import synthetic as syn
    return syn


def _structure(nvar, nequ, ncon, jF, jc, name, **meta):
    """diagonal H_F and H_c; jF / jc: (rows, cols), 0-based, in COO order"""
    d = np.arange(1, nvar + 1, dtype=np.int64)
    z = np.zeros(0, np.int64)
    one = lambda a: (np.asarray(a[0], np.int64) + 1, np.asarray(a[1], np.int64) + 1)   # noqa: E731
    s = _syn().Structure(nvar, nequ, ncon, (d, d), (d, d) if ncon else (z, z), one(jF), one(jc) if ncon else (z, z), name=name, meta=meta)
    for a, nr in ((s.jF, nequ), (s.jc, ncon)):
        assert len(a[0]) == 0 or (a[0].min() >= 1 and a[0].max() <= nr and a[1].min() >= 1 and a[1].max() <= nvar)
        assert len(set(zip(a[0].tolist(), a[1].tolist()))) == len(a[0]), "an entry twice"
    return s


def kkt(s):
    """rows, cols (1-based) of the KKT entries as the handle gets them"""
    rows, cols = s.kkt_pattern()
    o = s.meta.get("order")
    return (rows, cols) if o is None else (rows[o], cols[o])


def band(n, p, hw=2):
    return _syn().band_structure(n, p, hw=hw)


def _dense_then_last(nrows, ncols, count, col0=0):
    """`count` entries of an nrows x ncols block (columns from col0): the first count - 1 of its first ncols - 1 columns in row-major
    order, then the block's last entry, the only one of the last column.  The block's first and last row are read, and the first and
    the last slot belong to entries of rank 0 in their columns: the kernel reads both ends of the slot window through the table,
    from LDS, not through the index lists of a long column's tail."""
    k = np.arange(count - 1)
    assert count - 1 <= nrows * (ncols - 1)
    return np.concatenate([k // (ncols - 1), [nrows - 1]]), col0 + np.concatenate([k % (ncols - 1), [ncols - 1]])


def _mod4(base, choices):
    """the choice c with base + c = 3 (mod 4): a row stride of `vals` that moves the window inside its 16-byte chunk from problem to
    problem in either element type (positions 0, 1, 0 in double; 0, 3, 2 in float: the last one of a chunk is among them)"""
    return next(c for c in choices if (base + c) % 4 == 3)


def window_edge(which, width):
    cols = constants()["RVT_COLS"]
    i = np.arange(cols)
    if which == "F":     # W_F = nnz(J_F): every J_F slot lies in the one tile
        nequ = _mod4(2 * cols + width, (9, 10, 11, 12))
        s = _structure(cols, nequ, 0, _dense_then_last(nequ, cols, width), None, f"edge-F-{width}")
    elif which == "R":   # W_R = nequ: an entry in the first and in the last row; a few more entries for the stride of vals
        r = np.arange(width)
        extra = _mod4(2 * cols + 2 * width, (1, 3))
        s = _structure(cols, width, 0, (np.concatenate([r, np.arange(extra) + 5]), np.concatenate([r % cols, np.arange(extra) + 200])), None,
                       f"edge-R-{width}")
    elif which == "C":   # W_C = nnz(J_c)
        ncon = _mod4(5 * cols + width, (2, 3, 4, 5))
        s = _structure(cols, cols, ncon, (i, i), _dense_then_last(ncon, cols, width), f"edge-C-{width}")
    else:                # W_L = ncon: entries in the first and the last constraint and a few between
        e = _mod4(5 * cols + width, (5, 6, 7, 8))
        k = np.array([0, 1, width // 2, width - 2, 5, 6, 7, width - 1][8 - e:])
        s = _structure(cols, cols, width, (i, i), (np.concatenate([[0], k[1:]]), np.array([0, 7, 100, 200, 30, 31, 32, 255][8 - e:])), f"edge-L-{width}")
    s.meta.update(which=which, width=width)
    return s


def two_tile_edge():
    cols, w = constants()["RVT_COLS"], limit("F")
    nequ = _mod4(4 * cols + cols + w, (9, 10, 11, 12))
    i = np.arange(cols)
    r1, c1 = _dense_then_last(nequ, cols, w, col0=cols)
    return _structure(2 * cols, nequ, 0, (np.concatenate([i % nequ, r1]), np.concatenate([i, c1])), None, "two-tile-edge")


def window_ends(s, which, t=0):
    """the smallest rank (position in its column, COO order) among the entries that read the first and the last element of window
    `which` of tile t: below RVT_KF / RVT_KC the kernel reads that element from LDS"""
    T = tiles(s)["tiles"][t]
    ptr, slot, idx = _columns(s)[0 if which in "FR" else 1]
    lo, w = {"F": ("fslo", "wF"), "R": ("rlo", "wR"), "C": ("cslo", "wC"), "L": ("llo", "wL")}[which]
    c0, c1 = t * constants()["RVT_COLS"], min(s.nvar, (t + 1) * constants()["RVT_COLS"])
    out = []
    for target in (T[lo], T[lo] + T[w] - 1):
        q = ptr[c0] + np.nonzero((slot if which in "FC" else idx)[ptr[c0]:ptr[c1]] == target)[0]
        out.append(int((q - ptr[np.searchsorted(ptr, q, side="right") - 1]).min()))
    return tuple(out)


def chunk_elems(dtype):
    """elements of a 16-byte chunk"""
    return 2 if dtype == np.float64 else 4


def chunk_visits(s, which, dtype, B=3, t=0):
    """{(position of the window's first element inside its 16-byte chunk, chunks of the window)} over the B problems of a case and
    the caller offsets the GPU test gives the window's array (`edge_offsets`): the array starts `k` elements behind a 16-byte
    boundary, problem b's window at element k + b * stride + lo of it; chunks = (w + position + E - 1) // E as the kernel counts"""
    T = tiles(s)["tiles"][t]
    E = chunk_elems(dtype)
    lo, w, stride = {"F": (T["fslo"], T["wF"], s.nnzNS), "C": (T["cslo"], T["wC"], s.nnzNS), "R": (T["rlo"], T["wR"], s.nequ),
                     "L": (T["llo"], T["wL"], s.ncon)}[which]
    return {((k + b * stride + lo) % E, (w + (k + b * stride + lo) % E + E - 1) // E) for b in range(B) for k in edge_offsets(which, dtype)}


def edge_offsets(which, dtype):
    """caller offsets (elements) of the array a window lies in, in the window-edge tests: every array is passed as a whole allocation
    and as a sub-view 1 .. E - 1 elements behind a 16-byte boundary.  (`vals`: the row stride nnz = 3 (mod 4) alone walks both
    positions in double and positions 0, 3, 2 in float within three problems; r and lambda: at W_R = nequ, W_L = ncon the row stride
    IS the even window, and a whole allocation stays at position 0, or 0 and 2.)"""
    return tuple(range(chunk_elems(dtype)))


F_LENS, C_LENS = (0, 1, 5, 6, 7, 13, MAX_COL), (0, 1, 2, 3, 9)


def long_columns(nvar, over=False, seed=5):
    rng = np.random.default_rng(seed + nvar)
    nequ, ncon = 400, 40
    lf = rng.choice(F_LENS[:-1], nvar, p=[0.15, 0.2, 0.2, 0.2, 0.15, 0.1])
    lc = rng.choice(C_LENS, nvar, p=[0.35, 0.3, 0.2, 0.1, 0.05])
    lf[:len(F_LENS)] = F_LENS          # every length at least once; column 6 has the 255 maximum
    lc[:len(C_LENS)] = C_LENS
    lf[nvar - 1], lc[nvar - 1] = 13, 9   # the last column (the tile's last live thread) is overfull in both
    if over:
        lf[6] = MAX_COL + 1
    jF, jc = ([], []), ([], [])
    for (rr, cc), lens, nr, keep in ((jF, lf, nequ, constants()["RVT_KF"]), (jc, lc, ncon, constants()["RVT_KC"])):
        for c in range(nvar):
            n = int(lens[c])
            rows = rng.choice(nr - 1, n, replace=False)     # shuffled row order; the last row is kept out ...
            if n > keep:
                rows[-1] = nr - 1                            # ... and read only as the LAST entry of the overfull columns
            rr.append(rows)
            cc.append(np.full(n, c))
    cat = lambda a: (np.concatenate(a[0]), np.concatenate(a[1]))   # noqa: E731
    return _structure(nvar, nequ, ncon, cat(jF), cat(jc), f"long-{nvar}" + ("-over" if over else ""), tail_row=nequ - 1, tail_con=ncon - 1)


def _tile_columns(rng, c0, ncols, row_lo, row_hi, lens):
    rr, cc = [], []
    for c in range(c0, c0 + ncols):
        n = int(rng.choice(lens))
        rr.append(row_lo + rng.choice(row_hi - row_lo, n, replace=False))
        cc.append(np.full(n, c))
    return rr, cc


def _pin(rr, first, last):
    """the first column of a tile reads its first row, the last column its last row: the row window is what the case says"""
    rr[0][0], rr[-1][-1] = first, last
    for a in (rr[0], rr[-1]):
        assert len(set(a.tolist())) == len(a)


def unordered_rows(nequ, seed=9):
    cols = constants()["RVT_COLS"]
    rng = np.random.default_rng(seed)
    rows_of = [(1000, 1400), (0, 400), (nequ - 300, nequ)]     # tile 1's rows lie below tile 0's
    rr, cc = [], []
    for t, (lo, hi) in enumerate(rows_of):
        a, b = _tile_columns(rng, t * cols, cols, lo, hi, (1, 3, 5, 6, 7))
        a[0], a[-1], b[0], b[-1] = a[0][:1], a[-1][:1], b[0][:1], b[-1][:1]
        _pin(a, lo, hi - 1)
        rr += a
        cc += b
    k, c = _tile_columns(rng, 0, 3 * cols, 0, 5, (0, 1, 2, 3))
    return _structure(3 * cols, nequ, 5, (np.concatenate(rr), np.concatenate(cc)), (np.concatenate(k), np.concatenate(c)), f"unordered-{nequ}")


def gap_tile(kind, seed=4):
    cols = constants()["RVT_COLS"]
    rng = np.random.default_rng(seed)
    if kind == "F":      # tile 1 has no J_F entry (and one J_c entry, so that its columns are not all zero)
        rr, cc = [], []
        for t, (lo, hi) in ((0, (0, 300)), (2, (300, 600))):
            a, b = _tile_columns(rng, t * cols, cols, lo, hi, (1, 5, 7))
            a[0], a[-1], b[0], b[-1] = a[0][:1], a[-1][:1], b[0][:1], b[-1][:1]
            _pin(a, lo, hi - 1)
            rr += a
            cc += b
        jc = (np.array([0, 1, 2, 2]), np.array([3, cols + 9, 2 * cols + 1, 5]))
        return _structure(3 * cols, 600, 3, (np.concatenate(rr), np.concatenate(cc)), jc, "gap-F")
    # tile 1 has no J_c entry, its neighbours have; J_F a tridiagonal band in row order: the tiles own their rows
    n = 3 * cols
    b = band(n, 0, hw=1)
    c = np.concatenate([np.arange(0, cols, 3), np.arange(2 * cols, n, 2)])
    k = rng.integers(0, 6, len(c))
    k[0], k[-1] = 0, 5
    return _structure(n, n, 6, (b.jF[0] - 1, b.jF[1] - 1), (k, c), "gap-C")


def uncovered_row(which):
    cols, nequ = constants()["RVT_COLS"], 300
    i = np.arange(nequ)
    c = (i * 7) % cols
    keep = i != (0 if which == "first" else nequ - 1)
    i2 = np.concatenate([i[keep], (i[keep] + 1)[i[keep] + 1 < nequ - 1][::2]])       # a second entry in some columns
    c2 = np.concatenate([c[keep], ((i[keep] * 7 + 3) % cols)[i[keep] + 1 < nequ - 1][::2]])
    sel = np.unique(np.stack([i2, c2]), axis=1)
    sel = sel[:, sel[0] != (0 if which == "first" else nequ - 1)]
    return _structure(cols, nequ, 2, (sel[0], sel[1]), (np.array([0, 1, 1]), np.array([0, 100, 255])), f"uncovered-{which}")


def scattered(seed=3):
    rng = np.random.default_rng(seed)
    nvar, nequ, ncon = 300, 700, 3
    k = np.sort(rng.choice(nequ * nvar, 900, replace=False))       # row-major order: a tile's slots lie anywhere in J_F
    r, c = k // nvar, k % nvar
    keep = (c % 11 != 0)                                            # empty columns
    kc = np.sort(rng.choice(ncon * nvar, 60, replace=False))
    keepc = (kc % nvar) % 5 != 0
    return _structure(nvar, nequ, ncon, (r[keep], c[keep]), ((kc // nvar)[keepc], (kc % nvar)[keepc]), "scattered")


def shuffled_kkt(seed=8):
    s = band(300, 3)
    s.name = "shuffled-kkt"
    s.meta["order"] = np.random.default_rng(seed).permutation(s.nnzNS)
    return s


@functools.lru_cache(maxsize=None)
def pattern(name):
    """a pattern by name: "band-n-p-hw", "edge-W-width", "two-tile-edge", "long-nvar", "long-over", "unordered-nequ", "gap-F", "gap-C",
    "uncovered-first", "uncovered-last", "scattered", "shuffled-kkt"; cached, treat as read-only"""
    a = name.split("-")
    if a[0] == "band":
        return band(int(a[1]), int(a[2]), int(a[3]))
    if a[0] == "edge":
        return window_edge(a[1], int(a[2]))
    if a[0] == "long":
        return long_columns(257, over=True) if a[1] == "over" else long_columns(int(a[1]))
    if a[0] == "unordered":
        return unordered_rows(int(a[1]))
    if a[0] == "gap":
        return gap_tile(a[1])
    if a[0] == "uncovered":
        return uncovered_row(a[1])
    return {"two-tile-edge": two_tile_edge, "scattered": scattered, "shuffled-kkt": shuffled_kkt}[name]()


def edge_names():
    return [f"edge-{w}-{limit(w) + d}" for w in "FRCL" for d in (-1, 0, 1)] + ["two-tile-edge"]


LONG_NAMES = ("long-255", "long-256", "long-257", "long-600", "band-600-6-3", "band-600-6-4", "long-over")
PRIMAL_NAMES = ("unordered-2047", "unordered-2048", "unordered-2049", "gap-F", "gap-C", "uncovered-first", "uncovered-last")
ALIGN_NAMES = ("band-777-7-2", "long-257")
PB_NAMES = ("band-600-6-3", "unordered-2049")
PB_BATCHES = (1, 63, 64, 65, 511, 512, 513, 519)
OTHER_NAMES = ("scattered", "shuffled-kkt")


def f1_names():
    out = []
    for n in tuple(edge_names()) + LONG_NAMES + PRIMAL_NAMES + ALIGN_NAMES + PB_NAMES + OTHER_NAMES:
        if n not in out:
            out.append(n)
    return out


# ---- the host rule restated ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def columns(name):
    return _columns(pattern(name))


def _columns(s):
    """the transposed Jacobians as the handle builds them: per kind (ptr, slot, idx), a column's entries in COO order"""
    rows, cols = kkt(s)
    i0, j0 = np.asarray(rows, np.int64) - 1, np.asarray(cols, np.int64) - 1
    n, m = s.nvar, s.nequ
    out = []
    for sel, base in (((j0 < n) & (i0 >= n) & (i0 < n + m), n), ((j0 < n) & (i0 >= n + m), n + m)):
        k = np.nonzero(sel)[0]
        k = k[np.argsort(j0[k], kind="stable")]
        ptr = np.concatenate([[0], np.cumsum(np.bincount(j0[k], minlength=n))])
        out.append((ptr, k, i0[k] - base))
    return out


def tiles(s):
    """csrc/capi_handle.cpp's rule for the column tiles of row f1, restated.  Returns a dict: "tiles" (per tile fslo, wF, rlo, wR, cslo,
    wC, llo, wL, own_lo, own_hi), "nF", "nC" (the longest columns), "tiled" (every window within its limit, no column above 255
    entries), "own", "primal_tiles", "lds" (elements of the largest tile, as the host counts them)."""
    K = constants()
    (ptrF, slotF, idxF), (ptrC, slotC, idxC) = _columns(s)
    nt = (s.nvar + K["RVT_COLS"] - 1) // K["RVT_COLS"]
    T, tiled, lds = [], True, 0
    even = lambda w: (w + 3) & ~1   # noqa: E731
    for t in range(nt):
        c0, c1 = t * K["RVT_COLS"], min(s.nvar, (t + 1) * K["RVT_COLS"])
        d = {}
        for lo_k, w_k, a in (("fslo", "wF", slotF[ptrF[c0]:ptrF[c1]]), ("rlo", "wR", idxF[ptrF[c0]:ptrF[c1]]),
                             ("cslo", "wC", slotC[ptrC[c0]:ptrC[c1]]), ("llo", "wL", idxC[ptrC[c0]:ptrC[c1]])):
            d[lo_k], d[w_k] = (int(a.min()), int(a.max() - a.min() + 1)) if len(a) else (0, 0)
        d["own_lo"] = d["own_hi"] = 0
        T.append(d)
        if d["wF"] > K["RVT_MAXF"] or d["wR"] > K["RVT_MAXR"] or d["wC"] > K["RVT_MAXC"] or d["wL"] > K["RVT_MAXL"]:
            tiled = False
        lds = max(lds, even(d["wF"]) + even(d["wR"]) + even(d["wC"]) + even(d["wL"]))
    nF, nC = int(np.diff(ptrF).max()), int(np.diff(ptrC).max())
    if nF > MAX_COL or nC > MAX_COL:
        tiled = False
    own, prev = s.nequ > 0, 0
    for t in range(nt):
        if not own:
            break
        lo, hi = T[t]["rlo"], T[t]["rlo"] + T[t]["wR"]
        next_lo = T[t + 1]["rlo"] if t + 1 < nt else s.nequ
        own_hi = min(hi, max(next_lo, prev)) if t + 1 < nt else s.nequ
        if prev < lo or own_hi > hi or own_hi < prev:
            own = False
            break
        T[t]["own_lo"], T[t]["own_hi"] = prev, own_hi
        prev = own_hi
    if own and prev != s.nequ:
        own = False
    if not own:
        for d in T:
            d["own_lo"] = d["own_hi"] = 0
    return {"tiles": T, "nF": nF, "nC": nC, "tiled": tiled, "own": own and tiled, "lds": lds,
            "primal_tiles": ((s.nequ + K["RVT_PROWS"] - 1) // K["RVT_PROWS"] if tiled and not own else 0)}


def predict(s):
    """what a handle of the pattern must report before any number is looked at: config["f1_tiles"] under Options(f1_tiles=1), and whether
    the `_jac` twin is served (each Jacobian one run of slots, and J_F not empty)"""
    (_, slotF, _), (_, slotC, _) = _columns(s)
    run = lambda a: len(a) == 0 or int(a.max() - a.min() + 1) == len(a)   # noqa: E731
    return {"f1_tiles": tiles(s)["tiled"], "jac": bool(run(slotF) and run(slotC) and len(slotF) > 0)}


# ---- inputs and restatements ---------------------------------------------------------------------------------------------------------
def model(s, B, dtype, seed):
    """the model's arrays of a batch in `dtype` (tests/test_float32_rows_gpu._model in either type): zeros in hc (-0.0 after the flip)
    and one delta equal to 0; every problem has numbers of its own"""
    rng = np.random.default_rng(seed)
    f = lambda *sh: rng.standard_normal(sh).astype(dtype)   # noqa: E731
    m = {"hF": f(B, s.nnzhF), "hc": f(B, s.nnzhc), "Jx": f(B, s.nnzjF), "Jcx": f(B, s.nnzjc), "delta": np.abs(f(B)),
         "x": f(B, s.nvar), "r": f(B, s.nequ), "lam": f(B, s.ncon), "Fx": f(B, s.nequ), "cx": f(B, s.ncon)}
    m["hc"][:, ::7] = 0
    m["delta"][3 % B] = 0
    return m


def restate_prepare(old, counts, m, dtype, hess=True):
    """f32_rows.prepare in `dtype`; counts = (nnzhF, nnzhc, nnzjF, nnzjc, nequ, ncon, nvar)"""
    v = np.array(old, dtype, copy=True)
    o = np.concatenate([[0], np.cumsum(counts)])
    ncon = counts[5]
    if hess:
        v[:, :o[1]] = m["hF"]
    if ncon:
        v[:, o[1]:o[2]] = -m["hc"]
        v[:, o[3]:o[4]] = m["Jcx"]
        v[:, o[5]:o[6]] = -m["delta"].reshape(-1, 1)
    v[:, o[2]:o[3]] = m["Jx"]
    v[:, o[6]:] = 0
    return v


def counts_of(s):
    return (s.nnzhF, s.nnzhc, s.nnzjF, s.nnzjc, s.nequ, s.ncon, s.nvar)


def vals_of(s, m, old=None):
    """`vals` [B][nnz] as prepare leaves them (from ones), in the order of kkt(s)"""
    dtype = m["Jx"].dtype
    B = m["Jx"].shape[0]
    v = restate_prepare(np.ones((B, s.nnzNS), dtype) if old is None else old, counts_of(s), m, dtype)
    o = s.meta.get("order")
    return v if o is None else np.ascontiguousarray(v[:, o])


def restate_f1(s, vals, r, lam, Fx, cx):
    """f32_rows.residual_vectors in the element type of `vals`: (rhs [B][N], norms [B][2])"""
    T = vals.dtype
    rows, cols = kkt(s)
    rF, rC = R.column_ranks(rows, cols, s.nvar, s.nequ, s.ncon)
    with np.errstate(invalid="ignore", over="ignore"):
        dual = R.column_sums(rF, vals, r, s.nvar, T) - R.column_sums(rC, vals, lam, s.nvar, T)
        primal = np.concatenate([Fx - r, cx], axis=1)
        ninf = lambda v: np.max(np.abs(v), axis=1) if v.shape[1] else np.zeros(v.shape[0], T)   # noqa: E731
        return np.concatenate([dual, primal], axis=1), np.stack([ninf(dual), ninf(primal)], axis=1).astype(T)


def dual_bound(s, vals, r, lam):
    """(exact [B][nvar] longdouble, bound [B][nvar] longdouble): every dual entry formed in longdouble from the inputs, and
    (nF + nC + 1) (eps + eps(longdouble)) sum|terms| (module docstring).  The entries of a column come from `_columns`, this module's
    own grouping of the KKT entries, not from the helper the restatement uses."""
    B = vals.shape[0]
    exact, mag, cnt = np.zeros((s.nvar, B), LD), np.zeros((s.nvar, B), LD), np.zeros(s.nvar, LD)
    for (ptr, slot, idx), x, sign in zip(_columns(s), (r, lam), (1, -1)):
        col = np.repeat(np.arange(s.nvar), np.diff(ptr))
        t = (vals[:, slot].astype(LD) * x[:, idx].astype(LD)).T
        np.add.at(exact, col, sign * t)
        np.add.at(mag, col, np.abs(t))
        cnt += np.diff(ptr)
    eps = LD(np.finfo(vals.dtype).eps) + LD(np.finfo(LD).eps)
    return exact.T, (cnt + 1)[None, :] * eps * mag.T


def readers(s, kind, row):
    """(columns, ranks) of the entries that read residual row / constraint `row` (kind "F" / "C")"""
    ptr, _, idx = _columns(s)[0 if kind == "F" else 1]
    q = np.nonzero(idx == row)[0]
    c = np.searchsorted(ptr, q, side="right") - 1
    return c, q - ptr[c]


def nan_rows(name):
    """the residual row and the constraint (None without constraints) where the long-column tests put a NaN: the rows of the pattern
    that only tail entries read, or — a band has none — the last row, which column n - hw - 1 reads through its last entry"""
    s = pattern(name)
    if "tail_row" in s.meta:
        return s.meta["tail_row"], s.meta["tail_con"]
    return s.nequ - 1, (s.ncon - 1 if s.ncon else None)


@functools.lru_cache(maxsize=None)
def f1_case(name, B, dtype, seed=0):
    """(structure, model arrays, vals) of an f1 case; cached, treat as read-only"""
    s = pattern(name)
    m = model(s, B, dtype, 1000 * B + seed + sum(map(ord, name)))
    return s, m, vals_of(s, m)


NORM_VARIANTS = ("zero", "minus-zero", "inf", "nan-beside-inf", "last-tile", "c-part")


def norm_variants(s, m):
    """the first six problems of `m` changed in place for the rules of the two norms (NORM_VARIANTS); vals are formed afterwards.
    A dual entry is s1 - s2 with both sums started from +0.0: it is never -0.0, so the -0.0 of "minus-zero" sits in the primal part
    (Fx = -0.0, r = +0.0, cx = -0.0: every primal entry is -0.0, the norm is +0.0) beside an all-zero dual."""
    T = m["r"].dtype.type
    cols = constants()["RVT_COLS"]
    m["r"][0] = 0; m["lam"][0] = 0                              # noqa: E702  all-zero dual: the norm stays +0.0, not the prefill
    m["r"][1] = 0; m["lam"][1] = 0; m["Fx"][1] = -T(0); m["cx"][1] = -T(0)   # noqa: E702
    m["r"][2, s.nequ // 2] = -np.inf                            # -inf in r: +-inf in the dual, inf in both norms
    m["r"][3, s.nequ // 2] = np.inf; m["r"][3, s.nequ // 3] = np.nan    # noqa: E702  NaN beside inf: NaN wins
    last = (np.asarray(s.jF[1]) - 1) >= (s.nvar - 1) // cols * cols
    m["Jx"][4, last] *= T(1000); m["lam"][4] = 0               # noqa: E702  the largest dual entry in the last, partial tile
    m["cx"][5, s.ncon - 1] = T(-50)                             # the largest primal entry in the c part (tile 0 writes it)
    return NORM_VARIANTS


# ---- row f2: segment and chunk edges ---------------------------------------------------------------------------------------------------
def chunk(dtype):
    """slots of `vals` a workgroup of prepare_kernel serves: 256 threads x 4 doubles or 8 floats"""
    return 1024 if dtype == np.float64 else 2048


def il_tile(dtype):
    """elements of a problem a workgroup of prepare_il_kernel serves"""
    return 128 if dtype == np.float64 else 256


def _lower(n, count):
    """the first `count` entries of the lower triangle of order n, diagonal first, then the subdiagonals"""
    rr, cc, k = [], [], 0
    while sum(map(len, rr)) < count:
        assert k < n
        j = np.arange(n - k)
        rr.append(j + k)
        cc.append(j)
        k += 1
    return (np.concatenate(rr)[:count] + 1, np.concatenate(cc)[:count] + 1) if count else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def _wrapped(nr, n, count):
    """the first `count` entries (i, (i + k) mod n), k = 0, 1, ..: distinct while k < n"""
    assert count <= nr * n
    q = np.arange(count)
    return q % nr, (q % nr + q // nr) % n


def segments(nnzhF, nnzhc, nnzjF, nnzjc, nequ, ncon, nvar):
    """a pattern with exactly these segment sizes, banded, sized only to hit the counts"""
    assert (ncon > 0 or (nnzhc == 0 and nnzjc == 0)) and nnzjF > 0
    s = _structure(nvar, nequ, ncon, _wrapped(nequ, nvar, nnzjF), _wrapped(ncon, nvar, nnzjc) if ncon else None, "segments")
    s.hF = _lower(nvar, nnzhF)
    if ncon:
        s.hc = _lower(nvar, nnzhc)
    assert counts_of(s) == (nnzhF, nnzhc, nnzjF, nnzjc, nequ, ncon, nvar)
    return s


BASE_SIZES = (0.6, 0.3, 0.7, 0.3, 0.25, 0.2, 0.35)     # segment sizes in chunks: offsets 0.6, 0.9, 1.6, 1.9, 2.15, 2.35, nnz 2.7


def _sizes(C, scale=1.0):
    return [max(1, int(round(f * C * scale))) for f in BASE_SIZES]


def offset_cases(dtype):
    """{name: counts}: offset o_i (i = 1 .. 6) on k C - 1, k C, k C + 1 (the first chunk boundary behind o_(i-1)) and on j 256 -+ 1 (a
    thread-row boundary inside a chunk), the other segments as in BASE_SIZES; nnz on C - 1, C, C + 1, 2 C + 1; no constraints; no
    Hessian entries"""
    C = chunk(dtype)
    out = {}
    for i in range(1, 7):
        base = _sizes(C)
        before = sum(base[:i - 1])
        k = before // C + 1
        j = (before + base[i - 1]) // 256 * 256
        if j - 1 <= before:
            j += 256
        for tag, target in ((f"{k}C-1", k * C - 1), (f"{k}C", k * C), (f"{k}C+1", k * C + 1), ("row-1", j - 1), ("row+1", j + 1)):
            sz = list(base)
            sz[i - 1] = target - before
            out[f"o{i}@{tag}"] = tuple(sz)
    for tag, nnz in (("C-1", C - 1), ("C", C), ("C+1", C + 1), ("2C+1", 2 * C + 1)):
        sz = _sizes(C, nnz / (2.7 * C))
        sz[6] += nnz - sum(sz)
        out[f"nnz@{tag}"] = tuple(sz)
    sz = _sizes(C)
    out["ncon=0"] = (sz[0], 0, sz[2], 0, sz[4], 0, sz[6])
    out["nnzhF=0"] = (0,) + tuple(sz[1:])
    return out


def offsets_of(counts):
    return [int(x) for x in np.cumsum(counts)]


@functools.lru_cache(maxsize=None)
def segment_pattern(counts):
    return segments(*counts)


def band_counts(n, p):
    """segment sizes of band_structure(n, p) (half-width 2)"""
    return (3 * n - 3, n if p else 0, 5 * n - 6, n if p else 0, n, p, n)


@functools.lru_cache(maxsize=None)
def il_shapes(dtype):
    """band shapes (n, p) for prepare_il_kernel, chosen greedily so that the six offsets and nnz fall on and beside multiples of the tile
    (128 doubles, 256 floats): returns (shapes, {(i, d)}) with i = 1 .. 7 (7: nnz) and d = offset mod tile in {-1, 0, 1}"""
    T = il_tile(dtype)

    def hits(n, p):
        o = offsets_of(band_counts(n, p))
        return {(i + 1, d) for i, x in enumerate(o) for d in (-1, 0, 1) if (x - d) % T == 0 and x - d > 0}
    cand = [(n, p) for n in range(2 * T // 12, 5 * T // 2) for p in (1, 2, 3, 4, 5, 6, 7) if n % p == 0 and n >= 16]
    shapes, got = [], set()
    for _ in range(5):
        best = max(cand, key=lambda c: (len(hits(*c) - got), -c[0]))
        if not hits(*best) - got:
            break
        shapes.append(best)
        got |= hits(*best)
    return tuple(shapes), got


def il_index(p, e, length):
    """csrc/band.h, band_il_index: element e of problem p in an array interleaved over groups of 32 problems in blocks of eight elements,
    one spare block per problem"""
    blocks = (length + 7) // 8 + 1
    return ((p // 32 * blocks + e // 8) * 32 + p % 32) * 8 + e % 8


def il_len(batch, length):
    return (batch + 31) // 32 * ((length + 7) // 8 + 1) * 32 * 8


# lengths of the conversion cases: N = 2 n + p of band(n, p).  The band kernels, which alone take the interleaved layout, start at n = 12:
# 1, 7, 8 and 9 elements per problem cannot be built; 24 and 25 are the smallest, 31, 32, 33 the first with 7, 8, 9 elements mod 8
IL_LENGTHS = {24: (12, 0), 25: (12, 1), 31: (15, 1), 32: (16, 0), 33: (16, 1), 127: (63, 1), 128: (64, 0), 129: (64, 1), 1025: (512, 1)}
IL_BATCHES = (1, 31, 32, 33, 65)
