"""The mover table of the resident band program (csrc/band.h: BAND_MK_*; cnl_plan_get prefix "bandm") without a GPU: every used
piece descriptor of an epoch has exactly one table entry, in a staging set of a matching kind, with the descriptor's slot; the
address a set forms from its word is, for every lane, problem group and a partly filled last workgroup, the address the resident
kernel's descriptor decode forms; an interpreter that stages the pieces set by set gives the resident interpreter's bits; and a
pattern whose epochs do not fit the typed sets has no table, so its handles stay on the resident instance."""
import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn
from tests.support import band_mover_sim as M
from tests.support.band_res_sim import ResidentBandSim, decode
from tests.support.band_sim import NPIECE

SHAPES = [(200, 4, 2, {}), (200, 0, 2, {}), (360, 6, 1, {}), (96, 2, 2, {}), (1000, 10, 2, {"band_kernel": 2}), (2000, 20, 2, {}), (10000, 50, 2, {})]
REFUSED = (100, 2, 2)   # resident program: yes; an epoch of it needs more sets of a kind than the split has
_plans = {}


def _plan(n, p, hw, opt):
    key = (n, p, hw, tuple(sorted(opt.items())))
    if key not in _plans:
        s = syn.band_structure(n, p, hw=hw)
        rows, cols = s.kkt_pattern()
        _plans[key] = (s, hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT, **opt)))
    return _plans[key]


def _walk(pl):
    """(part, loff, nnz, N, epoch, sweep, descriptors, table words) of every epoch and sweep"""
    r = ResidentBandSim(pl)
    assert r.ok and pl.array("bandm_info").tolist() == [1, M.MOV_EW, M.FVALS, M.BVALS, M.BFACTOR]
    for q, P in enumerate(r.parts):
        T = M.table(pl, q)
        assert T.shape == (P["nepochs"], 2, NPIECE)
        for e in range(P["nepochs"]):
            for sweep, f in ((0, r.BE_FP), (1, r.BE_BP)):
                yield q, P["loff"], r.nnz, r.N, e, sweep, P["epochs"][e, f: f + NPIECE], T[e, sweep]


@pytest.mark.parametrize("n,p,hw,opt", SHAPES)
def test_one_entry_per_descriptor_in_a_set_of_its_kind(built, n, p, hw, opt):
    _, pl = _plan(n, p, hw, opt)
    typed = 0
    for q, loff, nnz, N, e, sweep, descs, words in _walk(pl):
        want = sorted(decode(int(pc), True) for pc in descs if pc >= 0)
        got = []
        for k, w in enumerate(words):
            pc = M.piece_of(sweep, k, int(w), loff)
            if pc is None:
                assert w == -1
                continue
            got.append(pc)
            kd = M.kind(sweep, k)
            if kd == M.MK_VALS:
                assert pc[0] == 0 and pc[2] % 8 == 0, (q, e, sweep, k)
            elif kd == M.MK_FACTOR:
                assert pc[0] == 2 and sweep == 1, (q, e, sweep, k)
            typed += kd != M.MK_GENERAL
        assert sorted(got) == want, (q, e, sweep)
        # ... and it is the table the assignment rule gives
        assert M.assign(descs, sweep, loff) == [int(w) for w in words], (q, e, sweep)
    assert typed > 0


@pytest.mark.parametrize("n,p,hw,opt", SHAPES)
def test_table_address_is_the_decoded_address(built, n, p, hw, opt):
    """every lane and problem group, a full workgroup and last workgroups of batch % 32 = 1 and 13 problems, `rhs` problem-major and
    interleaved; a typed word's byte offset fits 31 bits"""
    _, pl = _plan(n, p, hw, opt)
    lane, group, nvalid = np.arange(64)[None, None, :], np.arange(4)[None, :, None], np.array([32, 1, 13])[:, None, None]
    for q, loff, nnz, N, e, sweep, descs, words in _walk(pl):
        by_piece = {decode(int(pc), True): int(pc) for pc in descs if pc >= 0}
        for k, w in enumerate(words):
            pc = M.piece_of(sweep, k, int(w), loff)
            if pc is None:
                continue
            assert 0 <= int(w) < 1 << 31
            for ril in (0, 1):
                a = M.table_address(sweep, k, int(w), loff, nnz, N, ril, lane, group, nvalid)
                b = M.decode_address(by_piece[pc], loff, nnz, N, ril, lane, group, nvalid)
                assert a[0] == b[0] and a[1].shape == (3, 4, 64) and np.array_equal(a[1], b[1]), (q, e, sweep, k, ril)


@pytest.mark.parametrize("n,p,hw,opt", SHAPES)
def test_staging_by_the_table_gives_the_resident_bits(built, params, n, p, hw, opt):
    s, pl = _plan(n, p, hw, opt)
    B = 2 if n >= 10000 else 3
    vals, rhs = syn.batch_values(s, B, cfg=3 if n >= 10000 else 4)
    if n == 200 and p == 4:   # a ladder climber and a problem no rho rescues
        vals[1], rhs[1] = syn.band_values(s, 5001, stress="ladder")
        vals[2, s.offsets()[0]] = -1e300
    sim = M.MoverBandSim(pl)
    assert sim.ok and sim.has_table
    v1, v0 = vals.copy(), vals.copy()
    out1 = sim.newton_system(v1, rhs, s.nvar, 0.0, params)
    out0 = ResidentBandSim(pl).newton_system(v0, rhs, s.nvar, 0.0, params)
    ok = out0[1].astype(bool)
    assert np.array_equal(out1[0][ok].view(np.int64), out0[0][ok].view(np.int64))
    assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(out1[1:], out0[1:]))
    assert np.array_equal(v1.view(np.int64), v0.view(np.int64))


def test_the_table_leaves_the_programs_as_they_are(built):
    """tuning band_mover_table = 0 builds no table; every program array is the same words with and without it"""
    s, pl1 = _plan(200, 4, 2, {})
    _, pl0 = _plan(200, 4, 2, {"band_mover_table": 0})
    assert pl1.array("bandm_info")[0] == 1 and pl0.array("bandm_info")[0] == 0 and pl0.array("bandm_table0").size == 0
    for prefix in ("band", "bandr", "band4"):
        assert np.array_equal(pl1.array(f"{prefix}_info"), pl0.array(f"{prefix}_info"))
        for q in (0, 1):
            for k in ("part", "fops", "bops", "epochs", "borders"):
                assert np.array_equal(pl1.array(f"{prefix}_{k}{q}"), pl0.array(f"{prefix}_{k}{q}")), (prefix, k, q)


def test_an_epoch_that_does_not_fit_the_typed_sets_refuses_the_table(built):
    """the family has such patterns (short chains: n = 100 with 2, 5 or 10 constraints): the resident program exists, some epoch's
    pieces do not fit the sets by the assignment rule, and the plan has no table — its handles stay on the resident instance"""
    n, p, hw = REFUSED
    _, pl = _plan(n, p, hw, {})
    r = ResidentBandSim(pl)
    assert r.ok and pl.array("bandm_info")[0] == 0
    assert pl.array("bandm_table0").size == 0 and pl.array("bandm_table1").size == 0
    misfits = [(q, e, sweep) for q, P in enumerate(r.parts) for e in range(P["nepochs"]) for sweep, f in ((0, r.BE_FP), (1, r.BE_BP))
               if M.assign(P["epochs"][e, f: f + NPIECE], sweep, P["loff"]) is None]
    assert misfits
    # the rule itself: with no general set left, an epoch with a piece of `rhs` does not fit
    _, pl = _plan(200, 4, 2, {})
    r = ResidentBandSim(pl)
    E = r.parts[0]["epochs"][3]
    assert M.assign(E[r.BE_FP: r.BE_FP + NPIECE], 0, 0) is not None and M.assign(E[r.BE_FP: r.BE_FP + NPIECE], 0, 0, fvals=NPIECE) is None
