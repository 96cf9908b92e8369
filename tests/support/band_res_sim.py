"""The RESIDENT form of the band program (csrc/band.h: BAND_RES_SLOT_SHIFT; cnl_plan_get prefix "bandr") on the CPU interpreter:
a piece descriptor names the LDS slot it is committed to, an unused descriptor commits nothing, a slot no load of the epoch
writes keeps what it held — and is poisoned here as soon as an epoch does not read it, which is when the generator may hand it
to another block.  The forward sweep has the four slots of the out ring beside the fifteen piece slots, because the kernel that
runs this form stores factor records directly (BandSim.direct_records).  Also: the operands of a program by NAME (array,
element), to compare the resident form with the program it was derived from word for word."""
import numpy as np

from tests.support.band_sim import (BF_ENTER_B, BF_PIVOT_B, BF_PIVOT_X, BR_DI, BR_DR, BR_J0, BR_RR, BS_BC0, BS_BC1, BS_BORDER, BS_DG0, BS_DX,
                                    BS_FLAGS, BS_LB, BS_LX, BS_OD, BS_RHO, BS_RX, EPOCH, HW, LOUT_MAX, LREC, NB, NPIECE, NS, RW, SW, BandSim)

SLOT_SHIFT = 23
FSLOTS, BSLOTS, NSTAGE = NPIECE + LOUT_MAX // 8, NPIECE, NPIECE   # slots of the forward / backward sweep, staging register sets


def decode(pc, resident):
    """(array, slot or None, first element) of a piece descriptor"""
    if resident:
        return pc >> 28, (pc >> SLOT_SHIFT) & 31, pc & ((1 << SLOT_SHIFT) - 1)
    return pc >> 28, None, pc & ((1 << 28) - 1)


def epoch_operands(P, E, sim, sweep):
    """LDS element offsets an epoch's steps read, in stream order: (first element, count) per operand word"""
    ops = P["bops" if sweep else "fops"]
    o = int(E[sim.BE_BOFF if sweep else sim.BE_FOFF])
    end = o + int(E[sim.BE_OPLEN])
    out = []
    while o < end:
        st = ops[o: o + SW]
        fl = int(st[BS_FLAGS])
        nrows = (fl >> 8) & 255
        out += [(int(w) // 8, 1) for w in st[BS_DG0: BS_RX + 1]]
        if sweep:
            for flag, word in ((BF_PIVOT_X, BS_LX), (BF_PIVOT_B, BS_LB)):
                if fl & flag:
                    out.append((int(st[word]) // 8, LREC))
        for i in range(nrows):
            rb = ops[o + SW + RW * i: o + SW + RW * (i + 1)]
            out += [(int(rb[k]) // 8, 1) for k in [BR_DI] + list(range(BR_J0, BR_J0 + NB)) + [BR_RR]]
        o += SW + RW * nrows
    return out


class ResidentBandSim(BandSim):
    """forward / backward are BandSim's, step for step and in the same arithmetic order, with two differences: the operand pieces of an
    epoch are staged by _stage (slots, residency, skipped commits), and the factor records go straight to the factor storage
    (_record_target) instead of through the out ring, whose LDS the forward sweep's slots reach into"""
    direct_records = True

    def __init__(self, plan, prefix="bandr"):
        super().__init__(plan, prefix)
        self._first = {}

    def _stage(self, blk, pieces, arrays, P, e, sweep):
        nslots = BSLOTS if sweep else FSLOTS
        if e == (P["nepochs"] - 1 if sweep else 0):
            blk[:, :self.ZERO_OFF] = np.nan          # a sweep starts with nothing resident
        loaded = set()
        assert (pieces >= 0).sum() <= NSTAGE
        for pc in pieces:
            if pc < 0:                               # unused: commits nothing
                continue
            a, slot, base = decode(int(pc), True)
            assert slot < nslots and slot not in loaded, (e, sweep, slot)
            loaded.add(slot)
            arr = arrays[a]
            if base + 8 > arr.shape[1]:              # the spare block behind an interleaved array / the slack behind the records
                arr = np.concatenate([arr, np.full((arr.shape[0], base + 8 - arr.shape[1]), np.nan)], axis=1)
            blk[:, 8 * slot: 8 * slot + 8] = arr[:, base: base + 8]
        read = set()
        for off, cnt in epoch_operands(P, P["epochs"][e], self, sweep):
            if off != self.ZERO_OFF:
                read.update({off // 8, (off + cnt - 1) // 8})
        assert all(s < nslots for s in read), (e, sweep, sorted(read))
        for s in range(FSLOTS):                      # a slot the epoch does not read is free: what it held must not be read later
            if s not in read and s not in loaded:
                blk[:, 8 * s: 8 * s + 8] = np.nan


    def _record_target(self, blk, Lq, E, first_half, off):
        """where a forward step writes the factor record whose BS_LB / BS_LX word is `off`: (array, first element)"""
        if not self.direct_records:
            return blk, off // 8
        return Lq, off // 8 - self.LOUT_OFF + int(E[self.BE_LBASE if first_half else self.BE_LBASE2])

    def forward(self, vals, rhs, rho, ovr, tol, Lst):
        B = vals.shape[0]
        npos = np.zeros(B, np.int64)
        nzer = np.zeros(B, np.int64)
        wins = []
        for q, P in enumerate(self.parts):
            S = np.zeros((NS + 1, NS + 1, B))
            c = np.zeros((NS + 1, B))
            blk = np.zeros((B, self.LANE))
            ops, o = P["fops"], 0
            Lq = Lst[:, P["loff"]:]
            starts = np.concatenate([[0], np.cumsum(P["epochs"][:, self.BE_NSTEP])])
            assert starts[-1] == P["nsteps"]
            ep_of = np.repeat(np.arange(P["nepochs"]), P["epochs"][:, self.BE_NSTEP])
            for u in range(P["nsteps"]):
                if u == starts[ep_of[u]]:
                    E = P["epochs"][ep_of[u]]
                    if u and not self.direct_records:   # factor records of the previous epoch's second half
                        Ep = P["epochs"][ep_of[u] - 1]
                        Lq[:, Ep[self.BE_LBASE2]: Ep[self.BE_LBASE2] + Ep[self.BE_LCNT2]] = blk[:, self.LOUT_OFF: self.LOUT_OFF + Ep[self.BE_LCNT2]]
                    self._stage(blk, E[self.BE_FP: self.BE_FP + self.NPIECE], (vals, rhs), P, ep_of[u], 0)
                    assert o == E[self.BE_FOFF] and E[self.BE_OPLEN] <= 256
                st = ops[o: o + SW]
                fl = int(st[BS_FLAGS])
                nrows = (fl >> 8) & 255
                assert (st[1:BS_LB + 2] % 8 == 0).all()
                v = lambda off: blk[:, off // 8]
                es = u % NS
                live = [(u - HW + k) % NS for k in range(NB)]   # live slots: [0] = this step's pivot .. [HW] = the entering variable
                ps = live[0]
                # enter
                diag = (v(st[BS_DG0]) + v(st[BS_DG0 + 1])) + v(st[BS_DG0 + 2])
                rv = v(st[BS_RHO])
                if not (fl >> 16) & 1:
                    rv = np.where(ovr, rho, rv)
                S[es, es] = diag + rv
                for k in range(1, HW + 1):
                    s = (es - k) % NS
                    S[es, s] = S[s, es] = v(st[BS_OD + 2 * (k - 1)]) + v(st[BS_OD + 2 * (k - 1) + 1])
                S[NS, es] = S[es, NS] = v(st[BS_BC0]) + v(st[BS_BC1])
                c[es] = v(st[BS_RX])
                # rows
                for i in range(nrows):
                    rb = ops[o + SW + RW * i: o + SW + RW * (i + 1)]
                    dr = v(rb[BR_DI])
                    npos += dr > tol
                    nzer += np.abs(dr) <= tol
                    w = -1.0 / dr
                    J = [v(rb[BR_J0 + k]) for k in range(NB)]
                    tr = v(rb[BR_RR]) * w
                    for ka in range(NB):
                        a = live[ka]
                        ta = J[ka] * w
                        for kb in range(ka + 1):
                            b = live[kb]
                            S[a, b] = S[a, b] + ta * J[kb]
                            S[b, a] = S[a, b]
                        c[a] = c[a] + tr * J[ka]
                # border pivot
                if fl & BF_PIVOT_B:
                    bt = P["borders"][st[BS_BORDER]]
                    S[NS, NS] = S[NS, NS] + vals[:, bt[0]]
                    c[NS] = c[NS] + rhs[:, bt[1]]
                    d = S[NS, NS].copy()
                    npos += d > tol
                    nzer += np.abs(d) <= tol
                    w = np.stack([S[NS, live[k]] for k in range(NB)])
                    l = w / d
                    z = c[NS] / d
                    for ka in range(NB):
                        a = live[ka]
                        for kb in range(ka + 1):
                            b = live[kb]
                            S[a, b] = S[a, b] - w[ka] * l[kb]
                            S[b, a] = S[a, b]
                        c[a] = c[a] - w[ka] * z
                    rec, off = self._record_target(blk, Lq, P["epochs"][ep_of[u]], u - starts[ep_of[u]] < EPOCH // 2, st[BS_LB])
                    rec[:, off: off + NB] = l.T
                    rec[:, off + NB] = z
                    S[NS, :] = 0.0
                    S[:, NS] = 0.0
                    c[NS] = 0.0
                # band pivot
                if fl & BF_PIVOT_X:
                    d = S[ps, ps].copy()
                    npos += d > tol
                    nzer += np.abs(d) <= tol
                    w = S[:, ps].copy()
                    l = w / d
                    z = c[ps] / d
                    oth = live[1:] + [NS]
                    for ia, a in enumerate(oth):
                        for b in oth[: ia + 1]:
                            S[a, b] = S[a, b] - w[a] * l[b]
                            S[b, a] = S[a, b]
                        c[a] = c[a] - w[a] * z
                    rec, off = self._record_target(blk, Lq, P["epochs"][ep_of[u]], u - starts[ep_of[u]] < EPOCH // 2, st[BS_LX])
                    for k in range(1, NB):
                        rec[:, off + k - 1] = l[live[k]]
                    rec[:, off + 4] = l[NS]
                    rec[:, off + 5] = z
                    S[ps, :] = np.nan   # a pivoted slot holds nothing until the next variable enters it
                    S[:, ps] = np.nan
                    c[ps] = np.nan
                o += SW + RW * nrows
                if self.direct_records:
                    continue
                if u - starts[ep_of[u]] == EPOCH // 2 - 1 or (u + 1 == starts[ep_of[u] + 1] and u - starts[ep_of[u]] < EPOCH // 2 - 1):
                    Ec = P["epochs"][ep_of[u]]   # factor records of the epoch's first half
                    Lq[:, Ec[self.BE_LBASE]: Ec[self.BE_LBASE] + Ec[self.BE_LCNT]] = blk[:, self.LOUT_OFF: self.LOUT_OFF + Ec[self.BE_LCNT]]
                    blk[:, self.LOUT_OFF: self.ZERO_OFF] = np.nan
            if not self.direct_records:
                Ep = P["epochs"][P["nepochs"] - 1]
                Lq[:, Ep[self.BE_LBASE2]: Ep[self.BE_LBASE2] + Ep[self.BE_LCNT2]] = blk[:, self.LOUT_OFF: self.LOUT_OFF + Ep[self.BE_LCNT2]]
            wins.append((S, c))
        junction = None
        if self.nparts == 2:
            n, m0 = self.n, self.m0
            sL = [(m0 + i) % NS for i in range(HW)]
            sR = [(n - 1 - m0 - i) % NS for i in range(HW)]
            (SL, cL), (SR, cR) = wins
            SJ = np.zeros((HW, HW, B))
            cJ = np.zeros((HW, B))
            for i in range(HW):
                for j in range(HW):
                    SJ[i, j] = SL[sL[i], sL[j]] + SR[sR[i], sR[j]]
                cJ[i] = cL[sL[i]] + cR[sR[i]]
            lj = np.zeros((HW, HW, B))
            zj = np.zeros((HW, B))
            for i in range(HW):
                d = SJ[i, i].copy()
                npos += d > tol
                nzer += np.abs(d) <= tol
                w = SJ[:, i].copy()
                zj[i] = cJ[i] / d
                for a in range(i + 1, HW):
                    lj[a, i] = w[a] / d
                for a in range(i + 1, HW):
                    for b in range(i + 1, a + 1):
                        SJ[a, b] = SJ[a, b] - w[a] * lj[b, i]
                        SJ[b, a] = SJ[a, b]
                    cJ[a] = cJ[a] - w[a] * zj[i]
            junction = (lj, zj)
        return npos, nzer, junction

    def backward(self, vals, rhs, Lst, junction, d):
        B = vals.shape[0]
        n, m0 = self.n, self.m0
        xj = None
        if self.nparts == 2:
            lj, zj = junction
            xj = np.zeros((HW, B))
            for i in range(HW - 1, -1, -1):
                xj[i] = zj[i] - sum(lj[a, i] * xj[a] for a in range(i + 1, HW))
                d[:, m0 + i] = -xj[i]
        for q, P in enumerate(self.parts):
            xs = np.zeros((NS + 1, B))
            if xj is not None:
                for i in range(HW):
                    xs[((m0 + i) if q == 0 else (n - 1 - m0 - i)) % NS] = xj[i]
            blk = np.zeros((B, self.LANE))
            ops, o = P["bops"], 0
            Lq = Lst[:, P["loff"]:]
            starts = np.concatenate([[0], np.cumsum(P["epochs"][:, self.BE_NSTEP])])
            ep_of = np.repeat(np.arange(P["nepochs"]), P["epochs"][:, self.BE_NSTEP])
            for u in range(P["nsteps"] - 1, -1, -1):
                if u == starts[ep_of[u] + 1] - 1:
                    E = P["epochs"][ep_of[u]]
                    self._stage(blk, E[self.BE_BP: self.BE_BP + self.NPIECE], (vals, rhs, Lq), P, ep_of[u], 1)
                    assert o == E[self.BE_BOFF]
                st = ops[o: o + SW]
                fl = int(st[BS_FLAGS])
                nrows = (fl >> 8) & 255
                v = lambda off: blk[:, off // 8]
                live = [(u - HW + k) % NS for k in range(NB)]
                ps = live[0]
                if fl & BF_PIVOT_X:
                    off = st[BS_LX] // 8
                    x = blk[:, off + 5].copy()
                    for k in range(1, NB):
                        x = x - blk[:, off + k - 1] * xs[live[k]]
                    x = x - blk[:, off + 4] * xs[NS]
                    xs[ps] = x
                    blk[:, st[BS_DX] // 8] = -x
                if fl & BF_PIVOT_B:
                    off = st[BS_LB] // 8
                    x = blk[:, off + NB].copy()
                    for k in range(NB):
                        x = x - blk[:, off + k] * xs[live[k]]
                    xs[NS] = x
                    d[:, P["borders"][st[BS_BORDER]][2]] = -x
                for i in range(nrows):
                    rb = ops[o + SW + RW * i: o + SW + RW * (i + 1)]
                    acc = -v(rb[BR_RR])
                    for k in range(NB):
                        acc = acc + v(rb[BR_J0 + k]) * xs[live[k]]
                    blk[:, rb[BR_DR] // 8] = acc / v(rb[BR_DI])
                if fl & BF_ENTER_B:
                    xs[NS] = 0.0
                o += SW + RW * nrows
                if u == starts[ep_of[u]]:
                    E = P["epochs"][ep_of[u]]
                    d[:, E[self.BE_DXLO]: E[self.BE_DXLO] + E[self.BE_DXCNT]] = blk[:, self.DX_OFF: self.DX_OFF + E[self.BE_DXCNT]]
                    d[:, E[self.BE_DRLO]: E[self.BE_DRLO] + E[self.BE_DRCNT]] = blk[:, self.DR_OFF: self.DR_OFF + E[self.BE_DRCNT]]


def operand_names(sim, resident):
    """every operand word of the program -> the (array, element) its LDS offset holds when the step reads it ("zero": the zero
    cell, None: a slot nothing valid is in), parts, sweeps and steps in execution order"""
    out = []
    for P in sim.parts:
        for sweep in (0, 1):
            names = {}
            order = range(P["nepochs"] - 1, -1, -1) if sweep else range(P["nepochs"])
            for e in order:
                E = P["epochs"][e]
                words = epoch_operands(P, E, sim, sweep)
                pcs = E[sim.BE_BP: sim.BE_BP + sim.NPIECE] if sweep else E[sim.BE_FP: sim.BE_FP + sim.NPIECE]
                new = {}
                for k, pc in enumerate(pcs):
                    if pc < 0:
                        continue
                    a, slot, base = decode(int(pc), resident)
                    slot = k if slot is None else slot
                    assert not any(8 * slot + i in new for i in range(8)), "two loads into one slot"
                    new.update({8 * slot + i: (a, base + i) for i in range(8)})
                if resident:
                    read = set()
                    for off, cnt in words:
                        if off != sim.ZERO_OFF:
                            read.update({off // 8, (off + cnt - 1) // 8})
                    names = {k: v for k, v in names.items() if k // 8 in read and k not in new}
                    names.update(new)
                else:
                    names = new
                for off, cnt in words:
                    for i in range(cnt):
                        out.append("zero" if off == sim.ZERO_OFF else names.get(off + i))
    return out
