"""Factor records of the band kernels (csrc/band.hip) without a GPU.  The compute lanes store each pivot's record straight to the
launch's element-major record region; the record's first element comes from the program the generator writes (csrc/band.cpp),
unchanged: forward BS_LB / BS_LX hold the record's offset in the half-epoch out ring, BE_LBASE / BE_LBASE2 the first record
element of each half.  These tests pin that contract against the backward sweep's pieces of the factor (the mover reads records
where the backward step blocks say they are) and pin the program itself to a hash recorded before the kernels stopped staging
records in LDS."""
import hashlib
import json
import os

import numpy as np
import pytest

import cannoles_jl_amd  # noqa: F401
from cannoles_jl_amd import hipldl, synthetic as syn
from tests.support.band_sim import (BE_BP, BE_LBASE, BE_LBASE2, BE_NSTEP, BF_PIVOT_B, BF_PIVOT_X, BS_FLAGS, BS_LB, BS_LX, EPOCH, EW,
                                    LOUT_OFF, LREC, NPIECE, RW, SW)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "band_program_headline.json")
HEADLINE = (10000, 50)   # bench.py's pattern: band_structure(n = nequ = 10^4, ncon = 50)


def _plan(s, **opt):
    rows, cols = s.kkt_pattern()
    return hipldl.Plan(s.N, rows, cols, s.nvar, s.nequ, s.ncon, options=hipldl.Options(plan_kind=hipldl.PLAN_THROUGHPUT, **opt))


def _blocks(ops, nsteps):
    """step block offsets of a forward (or backward) stream, in stream order"""
    out, o = [], 0
    for _ in range(nsteps):
        out.append(o)
        o += SW + RW * ((int(ops[o + BS_FLAGS]) >> 8) & 255)
    return out


def _program_names(nparts, prefix):
    names = [f"{prefix}_info"]
    for q in range(nparts):
        names += [f"{prefix}_{k}{q}" for k in ("part", "fops", "bops", "epochs", "borders")]
    return names


def program_hashes(pl):
    """sha256 of every band program array cnl_plan_get exposes, 8-byte and 4-byte programs"""
    nparts = int(pl.array("band_info")[1])
    out = {}
    for prefix in ("band", "band4"):
        for name in _program_names(nparts, prefix):
            a = np.ascontiguousarray(pl.array(name)).astype(np.int32)
            out[name] = {"len": int(a.size), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}
    return out


def _check_record_indices(pl, prefix, esz):
    nparts = int(pl.array(f"{prefix}_info")[1])
    for q in range(nparts):
        pinfo = pl.array(f"{prefix}_part{q}")
        nsteps, nevents = int(pinfo[0]), int(pinfo[3])
        fops, bops = pl.array(f"{prefix}_fops{q}"), pl.array(f"{prefix}_bops{q}")
        E = pl.array(f"{prefix}_epochs{q}").reshape(-1, EW)
        fo = _blocks(fops, nsteps)
        bo = _blocks(bops, nsteps)[::-1]   # the backward stream runs from the last step to the first
        ep = np.repeat(np.arange(len(E)), E[:, BE_NSTEP])
        assert len(ep) == nsteps
        written = []
        for u in range(nsteps):
            e = E[ep[u]]
            fl = int(fops[fo[u] + BS_FLAGS])
            assert int(bops[bo[u] + BS_FLAGS]) & 255 == fl & 255
            for flag, word in ((BF_PIVOT_B, BS_LB), (BF_PIVOT_X, BS_LX)):
                if not fl & flag:
                    continue
                # the kernel's index (band.hip, frec_index): ring offset / element size - BAND_LOUT_OFF + BE_LBASE of the step's half
                off = int(fops[fo[u] + word])
                assert off % esz == 0
                half = BE_LBASE if u % EPOCH < EPOCH // 2 else BE_LBASE2
                r = off // esz - LOUT_OFF + int(e[half])
                # ... is where the backward step finds the record: an element of a factor piece (array 2) of the same epoch
                boff = int(bops[bo[u] + word]) // esz
                pc = int(e[BE_BP + boff // 8])
                assert pc >= 0 and pc >> 28 == 2, (u, pc)
                assert r == (pc & ((1 << 28) - 1)) + boff % 8, (q, u, r)
                written.append(r)
        # one record per factor event, each written once, consecutive from the part's first element
        assert sorted(written) == [LREC * k for k in range(nevents)]


@pytest.mark.parametrize("n,p,hw,opt", [(200, 4, 2, {}), (200, 0, 2, {}), (1000, 10, 2, {"band_kernel": 2}), (360, 6, 1, {}), (96, 2, 2, {}),
                                        (2000, 20, 2, {})])
def test_forward_record_index_is_the_backward_one(built, n, p, hw, opt):
    """every pivot's record goes to the element the backward sweep reads it from, in both programs"""
    pl = _plan(syn.band_structure(n, p, hw=hw), **opt)
    assert pl.array("band_info")[0] == 1
    _check_record_indices(pl, "band", 8)
    _check_record_indices(pl, "band4", 4)


def test_headline_program_is_unchanged(built):
    """bench.py's pattern: the record indices hold, and the program arrays are those recorded in tests/golden"""
    pl = _plan(syn.band_structure(*HEADLINE))
    _check_record_indices(pl, "band", 8)
    _check_record_indices(pl, "band4", 4)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert want["pattern"] == list(HEADLINE)
    assert program_hashes(pl) == want["arrays"]


def test_record_region_fits_the_factor_storage(built):
    """a workgroup's region is NL x lsize elements: the last record element of every part, and the slack the backward pieces may
    read behind it, stay below lsize"""
    pl = _plan(syn.band_structure(*HEADLINE))
    info = pl.array("band_info")
    nparts, lsize = int(info[1]), int(info[6])
    for q in range(nparts):
        pinfo = pl.array(f"band_part{q}")
        loff, nevents = int(pinfo[4]), int(pinfo[3])
        E = pl.array(f"band_epochs{q}").reshape(-1, EW)
        pcs = E[:, BE_BP:BE_BP + NPIECE].ravel()
        pcs = pcs[(pcs >= 0) & (pcs >> 28 == 2)] & ((1 << 28) - 1)
        assert loff % 8 == 0 and loff + LREC * nevents <= lsize
        assert loff + int(pcs.max()) + 8 <= lsize


if __name__ == "__main__":   # PYTHONPATH=. python tests/test_band_records_cpu.py records the fixture again
    pl = _plan(syn.band_structure(*HEADLINE))
    with open(GOLDEN, "w") as f:
        json.dump({"pattern": list(HEADLINE), "arrays": program_hashes(pl)}, f, indent=1)
        f.write("\n")
    print("wrote", GOLDEN)
