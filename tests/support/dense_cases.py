"""Inputs of the dense-backend tests (tests/test_dense_cases_cpu.py, tests/test_dense_gpu.py): one generator, numpy only.

A case is a residual-block Newton system with a DENSE residual Jacobian (csrc/dense.hip serves it): J_F m x n in column-major
COO, H_F = diagonal + first subdiagonal (an entry in an off-diagonal tile at every 64-row edge), and with constraints H_c on the
diagonal again (duplicate positions, summed) and min(10, n) random variables per constraint row.  The residual pivots are
-U(0.5, 2), not -1: w = -1 / d_r differs from 1, so the scaled operand diag(w) J of J'WJ is not a copy of J.

Every shape exists for one edge of the kernels (64: tile, 128: macro tile of dn_syrk2, 16: row chunk of dn_syrk2, 2048: rows
dn_yrhs stages at a time, 7: row tiles per pass of dn_ladder, 3: row tiles per workgroup of dn_panel).
"""
import numpy as np

from cannoles_jl_amd import synthetic as syn

# (n, m, p): what the shape is there for
SHAPES = [
    (64, 1, 0),      # exactly one full tile; a single residual row (m < 16)
    (64, 40, 0),     # m < n; m padded to 64
    (65, 130, 0),    # one real row in the last tile
    (129, 70, 0),    # Tn = 3: half-empty macro tile, clamped column pointers; m no multiple of 16
    (126, 150, 4),   # constraints straddle the edge at 128; T = 3 > Tn = 2: padded J columns meet non-zero multiplier components of x
    (128, 16, 1),    # the last tile holds one row, and it is a -delta pivot; m = 16
    (192, 200, 0),   # Tn = 3, all tiles full
    (470, 64, 3),    # T = 8: second pass of dn_ladder, three workgroups of dn_panel
    (64, 2100, 0),   # second 2048-row round of dn_yrhs, nine row blocks of dn_jx
]
TALL = (64, 2100, 0)   # J'WJ dominates H_F = -4: the "climbers" succeed at once
SEED = 1               # what the GPU tests use (the CPU test vouches for exactly these inputs)
MIX = 5                # problems of one ladder mix
GRAPH_CASE = ((96, 50, 0), 3)   # shape and batch of the graph-cache test: healthy, hopeless, climber
# general form (an irregular pattern condensed to ONE dense matrix): random_structure(n, m, p, density, seed) whose condensed
# order n + p = 454 needs T = 8 tiles per side — the ladder's second pass over the row tiles
GENERAL = (450, 300, 4, 0.02, 1)


def shape_id(shape):
    return "n%d-m%d-p%d" % shape


def structure(n, m, p, seed):
    rng = np.random.default_rng([seed, n, m, p])
    jr, jc = np.tile(np.arange(1, m + 1), n), np.repeat(np.arange(1, n + 1), m)          # dense J_F, column-major
    hd = np.arange(1, n + 1)
    hF = (np.concatenate([hd, hd[1:]]), np.concatenate([hd, hd[:-1]]))                   # diagonal + first subdiagonal
    z = np.zeros(0, np.int64)
    if p > 0:
        k = min(10, n)
        hc = (hd, hd)                                                                     # duplicates of the diagonal
        cr = np.repeat(np.arange(1, p + 1), k)
        cc = np.concatenate([np.sort(rng.choice(n, k, replace=False)) + 1 for _ in range(p)])
        jcs = (cr, cc)
    else:
        hc, jcs = (z, z), (z, z)
    return syn.Structure(n, m, p, hF, hc, (jr, jc), jcs, name="dense-case")


def values(s, B, seed):
    """(vals, rhs, rho_old) of B problems; by b % 5: 0 and 4 healthy, 1 hopeless (H_F = NaN), 2 indefinite (H_F diagonal -4)
    climbing from rho_old = 0, 3 the same from rho_old = 2."""
    n, m, p = s.nvar, s.nequ, s.ncon
    off = s.offsets()
    vals = np.zeros((B, s.nnzNS))
    rhs = np.zeros((B, s.N))
    rho_old = np.zeros(B)
    for b in range(B):
        rng = np.random.default_rng([seed, n, m, p, b])
        vals[b, off[0]:off[1]] = np.concatenate([rng.uniform(0.2, 1.0, n), rng.uniform(-0.05, 0.05, n - 1)])
        if p > 0:
            vals[b, off[1]:off[2]] = rng.uniform(-0.05, 0.05, n)
            vals[b, off[3]:off[4]] = rng.uniform(-1, 1, s.nnzjc)
            vals[b, off[5]:off[6]] = -0.1
        vals[b, off[2]:off[3]] = rng.standard_normal(m * n) / np.sqrt(n)
        vals[b, off[4]:off[5]] = -rng.uniform(0.5, 2.0, m)
        rhs[b] = rng.standard_normal(s.N)
        kind = b % 5
        if kind == 1:
            vals[b, off[0]:off[1]] = np.nan
        elif kind in (2, 3):
            vals[b, off[0]:off[0] + n] = -4.0
            if kind == 3:
                rho_old[b] = 2.0
    return vals, rhs, rho_old


def rungs(rho_old, nfact, params):
    """The rho of every factorisation newton_system! made (the first one at the rho slots as given: 0): the ladder of
    src/CaNNOLeS.jl:1029-1047 replayed from the returned nfact."""
    kdec, kinc, klarge, rho0, rhomax, rhomin = params[2:8]
    out = [0.0]
    if nfact > 1:
        rho = rho0 if rho_old == 0.0 else max(rhomin, kdec * rho_old)
        out.append(rho)
        while len(out) < nfact:
            rho = klarge * rho if rho_old == 0.0 else kinc * rho
            out.append(rho)
    return out


_cache = {}


def oracle_case(shape, B=MIX, seed=SEED):
    """The case and what the CPU oracle makes of it on the canonical order, computed once per session and shared (read-only):
    dict(s, rows, cols, vals, rhs, rho_old, d, ok, rho, ro, nf, vals_after)."""
    key = (shape, B, seed)
    if key not in _cache:
        from oracle import oracle as O
        s = structure(*shape, seed)
        rows, cols = s.kkt_pattern()
        vals, rhs, ro_in = values(s, B, seed)
        orc = O.Oracle(s.N, rows, cols, O.canonical_perm(s.nvar, s.nequ, s.ncon))
        v = vals.copy()
        d, ok, rho, ro, nf = O.newton_system_batch(orc, B, s.nvar, s.nequ, s.ncon, rhs, v, ro_in, O.default_params())
        c = dict(s=s, rows=rows, cols=cols, vals=vals, rhs=rhs, rho_old=ro_in, d=d, ok=ok, rho=rho, ro=ro, nf=nf, vals_after=v)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def general_case(B=3):
    """(s, vals, rhs) of the general-form case; values as tests/test_gpu_parity.py::test_irregular_sparsity_dense_treatment"""
    n, m, p, dens, seed = GENERAL
    s = syn.random_structure(n, m, p, dens, seed=seed)
    vr = [syn.random_values(s, 40 + b) for b in range(B)]
    return s, np.stack([v for v, _ in vr]), np.stack([r for _, r in vr])
