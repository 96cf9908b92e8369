"""The inputs of tests/test_dense_gpu.py, checked on the CPU oracle alone: the decisions every case is built for, and pivots far
above the rounding noise at every rung the ladder tries — the GPU tests compare decisions bit for bit and may neither skip nor
reclassify a problem, so no decision of theirs may hang on a pivot that a different summation order could turn."""
import numpy as np
import pytest

from tests.support import dense_cases as dc

NOISE = 4096.0 * np.finfo(float).eps   # tools/fuzz_parity.py calls a decision undetermined when min|D| <= NOISE max|D|


@pytest.fixture(scope="module")
def oracle_mod():
    from oracle import oracle as O
    O.build()
    return O


def _rung_margins(O, orc, s, vals, rho_old, nf, rho, params, problems):
    """min|D| / max|D| over every rung of `problems`, each rung refactorised by the oracle: fails only at the last one"""
    worst = np.inf
    n = s.nvar
    for b in problems:
        rr = dc.rungs(rho_old[b], int(nf[b]), params)
        assert len(rr) == nf[b] and rr[-1] == rho[b]
        for k, r in enumerate(rr):
            vv = vals[b].copy()
            if k > 0:
                vv[-n:] = r
            good = orc.try_to_factorize(vv, s.nvar, s.nequ, s.ncon, params[0])
            assert good == (k == len(rr) - 1)
            D = np.abs(orc.D)
            assert D.min() > NOISE * D.max(), (b, r, D.min() / D.max())
            worst = min(worst, D.min() / D.max())
    return worst


# the GPU tests' own inputs (B = 5 of SEED; the graph-cache case), and the same shapes at another seed with two mixes
CASES = [(sh, dc.MIX, dc.SEED) for sh in dc.SHAPES] + [dc.GRAPH_CASE + (dc.SEED,)] + [(sh, 5 if sh == dc.TALL else 10, 7) for sh in dc.SHAPES]


@pytest.mark.parametrize("shape,B,seed", CASES, ids=lambda v: dc.shape_id(v) if isinstance(v, tuple) else str(v))
def test_dense_case_decisions_and_pivot_margins(oracle_mod, shape, B, seed):
    O = oracle_mod
    tall = shape == dc.TALL
    c = dc.oracle_case(shape, B, seed)
    s, ok, nf, rho, ro = c["s"], c["ok"], c["nf"], c["rho"], c["ro"]
    n, m, p = shape
    assert (s.nvar, s.nequ, s.ncon, s.N) == (n, m, p, n + m + p)
    assert s.nnzhF == 2 * n - 1 and s.nnzjF == m * n and s.nnzjc == p * min(10, n) and s.nnzhc == (n if p else 0)
    assert (np.abs(c["vals"][0, s.offsets()[4]:s.offsets()[5]] + 1.0) > 1e-3).any()      # residual pivots are not -1: w != 1
    params = O.default_params()
    for b in range(B):
        kind = b % 5
        if kind in (0, 4):
            assert ok[b] and nf[b] == 1 and rho[b] == 0.0 and ro[b] == 0.0
        elif kind == 1:   # no rho repairs NaN: the ladder runs out, rho_old stays
            assert not ok[b] and nf[b] == 20 and rho[b] > params[6] and ro[b] == 0.0
        elif tall:
            assert ok[b] and nf[b] == 1 and rho[b] == 0.0 and ro[b] == c["rho_old"][b]
        elif kind == 2:
            assert ok[b] and nf[b] == 5 and rho[b] == dc.rungs(0.0, 5, params)[-1] and ro[b] == rho[b]   # rho0 x 100^3 = 6.055
        else:
            assert ok[b] and nf[b] == 3 and rho[b] == dc.rungs(2.0, 3, params)[-1] and ro[b] == rho[b]   # 2 / 3 x 8 = 5.333
    if not tall:
        assert nf[np.arange(B) % 5 != 1].max() >= 3
    # the rho slots: the last rho tried, where the ladder ran
    for b in range(B):
        want = 0.0 if nf[b] == 1 else dc.rungs(c["rho_old"][b], int(nf[b]), params)[-1]
        assert (c["vals_after"][b, -n:] == want).all()
    # every rung of every problem some rho repairs
    orc = O.Oracle(s.N, c["rows"], c["cols"], O.canonical_perm(n, m, p))
    problems = [b for b in range(B) if b % 5 != 1]
    worst = _rung_margins(O, orc, s, c["vals"], c["rho_old"], nf, rho, params, problems)
    print(f"{dc.shape_id(shape)} B {B} seed {seed}: min|D| / max|D| over all rungs >= {worst:.2e}")


def test_general_form_case_is_large_enough_and_determined(built, oracle_mod):
    """The irregular case of the general form: its condensed system needs eight tiles per side (order >= 449) on the plan the
    GPU test asks for, and both value sets decide far above the noise."""
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl
    O = oracle_mod
    B = 3
    s, vals, rhs = dc.general_case(B)
    rows, cols = s.kkt_pattern()
    P = hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, batch=B, options=hipldl.Options(general_dense=2))
    assert s.N - P.info["ncond"] >= 449 and P.info["fmax"] > 64
    params = O.default_params()
    orc = O.Oracle(s.N, rows, cols, O.canonical_perm(s.nvar, s.nequ, s.ncon))
    off = s.offsets()
    for scale in (1.0, -20.0):
        v = vals.copy()
        v[:, off[0]:off[1]] *= scale
        v0 = v.copy()
        d, ok, rho, ro, nf = O.newton_system_batch(orc, B, s.nvar, s.nequ, s.ncon, rhs, v, np.zeros(B), params)
        assert ok.all() and (nf == (1 if scale > 0 else 6)).all()
        worst = _rung_margins(O, orc, s, v0, np.zeros(B), nf, rho, params, range(B))
        print(f"general form, H_F x {scale}: min|D| / max|D| over all rungs >= {worst:.2e}")
