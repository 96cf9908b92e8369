"""The MOVER TABLE of the resident band program (csrc/band.h: BAND_MK_*; cnl_plan_get prefix "bandm") on the CPU: the table's format
restated, the address a staging set forms from a table word, the address the resident kernel's descriptor decode (csrc/band.hip,
BAND_ISSUE_GEN) forms for the same piece, the rule that assigns an epoch's pieces to sets, and an interpreter that stages every piece
in the set and slot the table names."""
import numpy as np

from tests.support.band_res_sim import SLOT_SHIFT, ResidentBandSim, decode
from tests.support.band_sim import NPIECE

MK_GENERAL, MK_VALS, MK_FACTOR = 0, 1, 2
FVALS, BVALS, BFACTOR = 11, 5, 6          # typed sets: forward 11 vals + 4 general, backward 5 vals + 6 factor + 4 general
MOV_EW = 2 * NPIECE                       # words per epoch: forward sets, then backward sets
SLOT_MASK = 31
NL = 32                                   # problems per workgroup of the instance = problems per group of the interleaved layout
EL_BYTES = NL * 8                         # typed byte offset per element index


def kind(sweep, k, fvals=FVALS, bvals=BVALS, bfactor=BFACTOR):
    if sweep == 0:
        return MK_VALS if k < fvals else MK_GENERAL
    return MK_VALS if k < bvals else MK_FACTOR if k < bvals + bfactor else MK_GENERAL


def table(plan, q):
    """[epoch][sweep][set] words of part q; None where the plan has no table"""
    if plan.array("bandm_info")[0] == 0:
        return None
    return plan.array(f"bandm_table{q}").reshape(-1, 2, NPIECE)


def piece_of(sweep, k, w, loff):
    """(array, slot, first element of the part's array) of the piece set k of a sweep carries, None for an unused set"""
    if w < 0:
        return None
    kd = kind(sweep, k)
    if kd == MK_GENERAL:
        return decode(int(w), True)
    off, slot = int(w) & ~SLOT_MASK, int(w) & SLOT_MASK
    assert off % EL_BYTES == 0
    return (0, slot, off // EL_BYTES) if kd == MK_VALS else (2, slot, off // EL_BYTES - loff)


def _movp(lane, group, nvalid):
    """problem of a mover lane inside the workgroup, clamped to the problems the batch has (csrc/band.hip: movp); lane, group and
    nvalid may be arrays that broadcast"""
    return np.minimum(group * 8 + lane // 8, nvalid - 1)


def decode_address(pc, loff, nnz, N, ril, lane, group, nvalid):
    """csrc/band.hip, BAND_ISSUE_GEN for the instance the table serves (Float64, 32 problems per workgroup, factor records stored
    directly, `vals` interleaved): (array, byte offset from the workgroup's base of that array) lane `lane` loads for problem group
    `group` of the piece with resident descriptor pc"""
    le = lane % 8
    arr = pc >> 28
    el = (pc & ((1 << SLOT_SHIFT) - 1)) + (loff if arr == 2 else 0)
    il = True if arr == 0 else bool(ril) if arr == 1 else True
    ilw = NL * 8
    m = el & 7 if il else 0
    gap = ilw - 8 if il and arr != 2 else 0
    tm = NL if arr == 2 else 1
    pb = ((el >> 3) * ilw if il else el) * 8
    strd = 1 if arr == 2 else 8 if il else nnz if arr == 0 else N
    t = m + le
    tl = t * tm + (t >> 3) * gap
    return arr, pb + ((_movp(lane, group, nvalid) * strd + tl) << 3)


def table_address(sweep, k, w, loff, nnz, N, ril, lane, group, nvalid):
    """the same from the table word of set k: a typed set adds the word's byte offset and a lane offset that no epoch changes"""
    kd = kind(sweep, k)
    if kd == MK_GENERAL:
        return decode_address(int(w), loff, nnz, N, ril, lane, group, nvalid)
    le, p = lane % 8, _movp(lane, group, nvalid)
    off = int(w) & ~SLOT_MASK
    if kd == MK_VALS:
        return 0, off + (p * 8 + le) * 8
    return 2, off + (p + le * NL) * 8


def assign(descs, sweep, loff, fvals=FVALS, bvals=BVALS, bfactor=BFACTOR):
    """csrc/band.cpp, build_band_mover for one epoch and sweep: the fifteen table words of the resident descriptors `descs`, or None
    where the epoch does not fit the sets (a typed set carries only its kind, a piece whose typed sets are taken travels in a general
    one) or a typed offset does not fit 31 bits"""
    nv, nf = (bvals, bfactor) if sweep else (fvals, 0)
    nxt = {MK_VALS: 0, MK_FACTOR: nv, MK_GENERAL: nv + nf}
    end = {MK_VALS: nv, MK_FACTOR: nv + nf, MK_GENERAL: NPIECE}
    out = [-1] * NPIECE
    for pc in descs:
        if pc < 0:
            continue
        a, slot, el = decode(int(pc), True)
        kd = MK_VALS if a == 0 and el % 8 == 0 else MK_FACTOR if a == 2 else MK_GENERAL
        if nxt[kd] == end[kd]:
            kd = MK_GENERAL
        if nxt[kd] == end[kd]:
            return None
        w = int(pc)
        if kd != MK_GENERAL:
            off = (el + (loff if kd == MK_FACTOR else 0)) * EL_BYTES
            if off >= 1 << 31:
                return None
            w = off | slot
        out[nxt[kd]] = w
        nxt[kd] += 1
    return out


class MoverBandSim(ResidentBandSim):
    """ResidentBandSim with every epoch's pieces staged from the mover table: set by set, each piece into the slot its word names"""

    def __init__(self, plan):
        super().__init__(plan, "bandr")
        self.has_table = plan.array("bandm_info")[0] == 1
        for q, P in enumerate(self.parts):
            P["mover"] = table(plan, q)

    def _stage(self, blk, pieces, arrays, P, e, sweep):
        staged = []
        for k, w in enumerate(P["mover"][e, sweep]):
            pc = piece_of(sweep, k, int(w), P["loff"])
            staged.append(-1 if pc is None else (pc[0] << 28) | (pc[1] << SLOT_SHIFT) | pc[2])
        super()._stage(blk, np.array(staged, dtype=np.int64), arrays, P, e, sweep)
