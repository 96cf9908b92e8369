"""The RESIDENT form of the band program (csrc/band.h; cnl_plan_get prefix "bandr") without a GPU: pieces of `vals` are aligned
blocks of eight elements that keep their LDS slot while the next epoch of the sweep needs them.  The program is interpreted with
slots, residency and skipped commits (tests/support/band_res_sim.py) against the oracle, with the tolerances of
tests/test_band_cpu.py; every operand word is checked by NAME against the program the form was derived from; and the blocks of
`vals` a system loads are counted (tools/band_block_count.py) against limits that come from the 15-piece program's own counts —
21 888 blocks touched forward of which 15 015 are distinct, 9 383 backward of which 7 506 — not from a run of the new code."""
import importlib.util
import os

import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn
from oracle import oracle as O
from tests.support.band_res_sim import BSLOTS, FSLOTS, NSTAGE, ResidentBandSim, decode, operand_names
from tests.support.band_sim import BandSim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = (10000, 50)
SMALL = [(200, 4, 2, {}), (200, 0, 2, {}), (1000, 10, 2, {"band_kernel": 2}), (360, 6, 1, {}), (96, 2, 2, {}), (2000, 20, 2, {})]


def _counter():
    spec = importlib.util.spec_from_file_location("band_block_count", os.path.join(ROOT, "tools", "band_block_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _plan(s, **opt):
    rows, cols = s.kkt_pattern()
    return hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT, **opt)), rows, cols


def _check(s, vals, rhs, params, rho_old=0.0, **opt):
    pl, rows, cols = _plan(s, **opt)
    sim = ResidentBandSim(pl)
    assert sim.ok, "a pattern the 15-piece program serves has a resident form"
    B = vals.shape[0]
    v = vals.copy()
    d, ok, rho, ro, nf = sim.newton_system(v, rhs, s.nvar, rho_old, params)
    orc = O.Oracle(s.N, rows, cols, O.canonical_perm(s.nvar, s.nequ, s.ncon))
    v0 = vals.copy()
    d0, ok0, rho0, ro0, nf0 = O.newton_system_batch(orc, B, s.nvar, s.nequ, s.ncon, rhs, v0, np.full(B, float(rho_old)), params)
    assert np.array_equal(ok, ok0) and np.array_equal(nf, nf0) and np.array_equal(rho, rho0) and np.array_equal(ro, ro0)
    assert np.array_equal(v[:, -s.nvar:], v0[:, -s.nvar:])
    for b in range(B):
        if ok0[b]:
            assert np.abs(d[b] - d0[b]).max() <= 1e-11 * np.abs(d0[b]).max()
    # ... and the 15-piece program, whose steps and arithmetic it shares, gives the same bits on this interpreter
    v1 = vals.copy()
    d1 = BandSim(pl).newton_system(v1, rhs, s.nvar, rho_old, params)[0]
    assert np.array_equal(d[ok0], d1[ok0])
    return pl, sim


@pytest.mark.parametrize("n,p,hw,opt", SMALL)
def test_resident_program_reproduces_the_oracle(built, params, n, p, hw, opt):
    s = syn.band_structure(n, p, hw=hw)
    vals, rhs = syn.batch_values(s, 3, cfg=4)
    _check(s, vals, rhs, params, **opt)


def test_resident_program_ladder_and_hopeless(built, params):
    """the ladder runs the forward sweep again from its first epoch: nothing is resident across sweeps"""
    s = syn.band_structure(400, 4)
    vals = np.stack([syn.band_values(s, 5000 + b, stress="ladder")[0] for b in range(3)])
    rhs = np.stack([syn.band_values(s, 5000 + b, stress="ladder")[1] for b in range(3)])
    vals[2, s.offsets()[0]] = -1e300
    _check(s, vals, rhs, params)
    _check(s, vals, rhs, params, rho_old=0.3)


def test_resident_program_full_size_headline_pattern(built, params):
    s = syn.band_structure(*HEADLINE)
    vals, rhs = syn.batch_values(s, 2, cfg=3)
    _check(s, vals, rhs, params)


def _slot_rules(pl):
    """descriptors: at most NSTAGE loads per epoch, each into a slot of the sweep, no slot twice, aligned blocks of vals unless packed
    as the 15-piece program packs them; the steps, rows, borders and every epoch field behind the pieces are the 15-piece program's"""
    a, r = BandSim(pl, "band"), ResidentBandSim(pl)
    assert r.ok and (r.nparts, r.m0, r.n, r.N, r.nnz, r.lsize) == (a.nparts, a.m0, a.n, a.N, a.nnz, a.lsize)
    for Pa, Pr in zip(a.parts, r.parts):
        assert all(Pa[k] == Pr[k] for k in ("nsteps", "nepochs", "npiv", "nevents", "loff"))
        assert np.array_equal(Pa["borders"], Pr["borders"])
        assert np.array_equal(Pa["epochs"][:, 2 * r.NPIECE:], Pr["epochs"][:, 2 * r.NPIECE:])
        assert Pa["fops"].shape == Pr["fops"].shape and Pa["bops"].shape == Pr["bops"].shape
        for f, nslots in ((r.BE_FP, FSLOTS), (r.BE_BP, BSLOTS)):
            for E in Pr["epochs"]:
                pcs = [decode(int(pc), True) for pc in E[f: f + r.NPIECE] if pc >= 0]
                assert len(pcs) <= NSTAGE and all(pc < 0 for pc in E[f + len(pcs): f + r.NPIECE])
                slots = [sl for _, sl, _ in pcs]
                assert len(set(slots)) == len(slots) and all(0 <= sl < nslots for sl in slots)
    return a, r


@pytest.mark.parametrize("n,p,hw,opt", SMALL + [HEADLINE + (2, {})])
def test_every_operand_is_in_the_slot_its_offset_names(built, n, p, hw, opt):
    """slot safety: walking both sweeps with the names (array, element) of what every LDS element holds — a slot an epoch does not read
    is freed — every operand word of the resident program reads the element the same word of the 15-piece program reads"""
    pl, _, _ = _plan(syn.band_structure(n, p, hw=hw), **opt)
    a, r = _slot_rules(pl)
    want, got = operand_names(a, False), operand_names(r, True)
    assert None not in want and len(want) == len(got)
    bad = [i for i, (x, y) in enumerate(zip(want, got)) if x != y]
    assert not bad, (len(bad), bad[:5], [(want[i], got[i]) for i in bad[:5]])


def test_headline_block_loads(built):
    """blocks of vals loaded per system, both parts: forward <= 16 000 (21 888 today, 15 015 distinct; the slack is one stream left
    unaligned in part 0, 626 epochs, and the first epochs), backward <= 7 700 (9 383 today, 7 506 distinct)"""
    pl, _, _ = _plan(syn.band_structure(*HEADLINE))
    cnt = _counter()
    today, res = cnt.vals_block_loads(pl, "band"), cnt.vals_block_loads(pl, "bandr")
    print("blocks of vals per system:", today, res)
    assert (today["forward"], today["forward_distinct"], today["backward"], today["backward_distinct"]) == (21888, 15015, 9383, 7506)
    assert res["forward"] <= 16000
    assert res["backward"] <= 7700


def test_tuning_switches_the_resident_program_off(built):
    pl, _, _ = _plan(syn.band_structure(200, 4), band_resident=0)
    assert pl.array("band_info")[0] == 1 and pl.array("bandr_info")[0] == 0
    # patterns the 15-piece program does not serve have no resident form either
    pl, _, _ = _plan(syn.band_structure(200, 4, hw=3))
    assert pl.array("bandr_info")[0] == 0
