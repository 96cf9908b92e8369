"""What the tests of the staged rho ladder of subtree handles share (tuning subtree_ladder = R: csrc/capi_run.cpp — launch_subtrees —,
csrc/kernels.hip — subtree_ladder_kernel, the first decide, the rung decide and the commit) — tests/test_subtree_ladder_cpu.py and
tests/test_subtree_ladder_gpu.py: numpy only.

Nothing is invented here.  Shapes, mixes, oracles and bars are those of tests/support/general_subtrees_cases.py (GS: the seven-kind
mix in double, WANT_NF = [1, 20, 6, 4, 1, 1, 20]) and tests/support/f32_subtrees_cases.py (FS: the five-kind mix in float,
WANT_NF = [1, 10, 5, 4, 1]).  Two further parameter sets are default_params with ONLY rhomax changed, so that every rho a rung tries —
and with it every verdict the existing tests vouch for — is a rho of the default ladder:
    `between`  rhomax = sqrt(klarge) x rho_2 of the rho_old = 0 ladder, between rho_2 and rho_3: its failures exhaust at nfact 3
    `below`    rhomax = rho_0 / 10, below rho_1: rung 1 is tried above rhomax and the reference's loop never runs

The sequence is stated three times, each from the reference (src/CaNNOLeS.jl:1019-1051) by itself:
    reference_ladder  the reference's loop on a sequence of verdicts (what the sequential kernel runs);
    staged_ladder     the staged sequence on the same verdicts, problem by problem: first decide, R rung decides, the resumed
                      climbers — the state machine of the kernels, in the handle's element type;
    SubtreeLadderSim  (and SubtreeLadderSimF32) the staged sequence on a BATCH with done masks over GS.SubtreeSim's task-by-task walk:
                      first attempt, R rungs, backward stages, commit, climbers, with a trace of the launches.
`launches(R, S)` is the launch-count formula of the issue as a function."""
import numpy as np

from tests.support import dense_general_cases as GC
from tests.support import f32_subtrees_cases as FS
from tests.support import general_subtrees_cases as GS

F32, F64 = np.float32, np.float64
GRID12, GRID16, GRID32, FOREST3 = GS.GRID12, GS.GRID16, GS.GRID32, GS.FOREST3
R_MAX = 64
R_SWEEP = (0, 1, 2, 3, 4, 5, 19, 24)      # double: see tests/test_subtree_ladder_cpu.py for what each value is the edge of
R_EXHAUST = {F64: 19, F32: 9}             # the rung whose decide finds rho_{R+1} > rhomax for the mix's failures (nfact 20 / 10)
DONE_CLIMBING, DONE_FIRST, DONE_RUNGS = 0, 1, 2


def launches(R, S, call="newton_system"):
    """launches of one call of a subtree handle with S stages and subtree_ladder = R"""
    if call == "try_to_factorize":
        return S + 1
    if call == "solve_ldl":
        return 2 * S
    return 2 * S + 2 if R == 0 else (R + 2) * S + R + 3


# ---- the parameter sets ----
def params_between(p):
    """rhomax between rho_2 and rho_3 of the rho_old = 0 ladder, nothing else changed"""
    q = np.array(p)
    q[6] = q.dtype.type(np.sqrt(float(q[4]))) * (q[4] * q[5])
    assert q[4] * q[5] < q[6] < q[4] * (q[4] * q[5])
    return q


def params_below(p):
    """rhomax below rho_1 = rho_0 (and below max(rhomin, kdec x 2) of the problems that come with rho_old = 2)"""
    q = np.array(p)
    q[6] = q[5] / q.dtype.type(10)
    assert q[7] < q[6] < q[5]
    return q


PARAM_SETS = {"default": lambda p: np.array(p), "between": params_between, "below": params_below}
_cases = {}


def case_with_params(c, name, f32=False):
    """the case `c` (GS.case / FS.case) with the oracle's results under parameter set `name`, computed once and shared read-only"""
    if name == "default":
        return c
    key = (id(c), name)
    if key not in _cases:
        from oracle import oracle as O
        s = c["s"]
        p = PARAM_SETS[name](c["p32"] if f32 else c["params"])
        orc = O.Oracle(s.N, c["rows"], c["cols"], O.canonical_perm(s.nvar, s.nequ, s.ncon))
        va = np.array(c["vals"], F64)
        d, ok, rho, rold, nf = O.newton_system_batch(orc, len(va), s.nvar, s.nequ, s.ncon, np.array(c["rhs"], F64), va, np.array(c["rho_old"], F64),
                                                     np.array(p, F64))
        out = dict(c, d=d, ok=np.asarray(ok, bool), rho=rho, ro=rold, nf=np.asarray(nf, np.int64), vals_after=va)
        out["p32" if f32 else "params"] = p
        if not f32:
            out["key"] = (c["key"], name)
        _cases[key] = out
    return _cases[key]


# ---- the reference's loop and the staged sequence, on a sequence of verdicts ----
def reference_ladder(verdict, rho_old, p, T=F64):
    """src/CaNNOLeS.jl:1019-1051 as the sequential kernel runs it; verdict(attempt, rho) -> bool (attempt 0: rho as given).
    Returns (ok, rho, rho_old, nfact, wrote) with wrote = the last rho tried (None: the rho slots are not touched)."""
    p = np.asarray(p, T)
    kdec, kinc, klarge, rho0, rhomax, rhomin = p[2], p[3], p[4], p[5], p[6], p[7]
    ro = T(rho_old)
    rho, wrote, nfact = T(0), None, 0
    ok = bool(verdict(nfact, None))
    nfact += 1
    if not ok:
        rho = rho0 if ro == 0 else max(rhomin, T(kdec * ro))
        wrote = rho
        ok = bool(verdict(nfact, rho))
        nfact += 1
        while not ok and rho <= rhomax:
            rho = T(klarge * rho) if ro == 0 else T(kinc * rho)
            if rho <= rhomax:
                wrote = rho
                ok = bool(verdict(nfact, rho))
                nfact += 1
        if rho <= rhomax:
            ro = rho
    return ok, T(rho), T(ro), nfact, wrote


def first_decide(ok, rho_old, p, T):
    """the first decide of a call with R > 0: the state of one problem"""
    if ok:
        return dict(done=DONE_FIRST, ok=True, rho=T(0), ro=T(rho_old), nf=1, next=None, wrote=None)
    ro = T(rho_old)
    return dict(done=DONE_CLIMBING, ok=False, rho=None, ro=ro, nf=1, next=p[5] if ro == 0 else max(p[7], T(p[2] * ro)), wrote=None)


def rung_decide(st, ok, k, p, T):
    """the decide behind rung k for a problem that is not done (st: its state, changed in place)"""
    assert st["done"] == DONE_CLIMBING
    kinc, klarge, rhomax = p[3], p[4], p[6]
    r = st["next"]
    st["nf"], st["wrote"] = k + 1, r
    if ok:
        st.update(ok=True, rho=r, done=DONE_RUNGS)
        if r <= rhomax:
            st["ro"] = r
        return
    if not r <= rhomax:                      # rung 1 above rhomax: the loop never runs
        st.update(rho=r, done=DONE_RUNGS)
        return
    nx = T(klarge * r) if st["ro"] == 0 else T(kinc * r)
    if not nx <= rhomax:                     # exhausted: rho_{k+1} is never tried
        st.update(rho=nx, done=DONE_RUNGS)
        return
    st["next"] = nx


def resume(st, verdict, R, p, T):
    """the climbers of a problem still climbing after R rungs: the reference's while loop entered at rho_{R+1}"""
    assert st["done"] == DONE_CLIMBING and st["nf"] == R + 1
    kinc, klarge, rhomax = p[3], p[4], p[6]
    ro = st["ro"]
    rho = wrote = st["next"]
    nfact = R + 1
    ok = bool(verdict(nfact, rho))
    nfact += 1
    while not ok and rho <= rhomax:
        rho = T(klarge * rho) if ro == 0 else T(kinc * rho)
        if rho <= rhomax:
            wrote = rho
            ok = bool(verdict(nfact, rho))
            nfact += 1
    if rho <= rhomax:
        ro = rho
    st.update(ok=ok, rho=rho, ro=ro, nf=nfact, wrote=wrote, done=DONE_RUNGS)


def staged_ladder(verdict, rho_old, p, R, T=F64):
    """the staged sequence of one problem on a sequence of verdicts; the outputs of reference_ladder and the attempts made, in order,
    as (attempt, rho, where) with where in ("first", "rung", "climbers")"""
    assert R >= 1
    p = np.asarray(p, T)
    tried = [(0, None, "first")]
    st = first_decide(bool(verdict(0, None)), rho_old, p, T)
    for k in range(1, R + 1):
        if st["done"]:
            continue                         # the workgroups of a problem that is done leave at once
        tried.append((k, st["next"], "rung"))
        rung_decide(st, bool(verdict(k, st["next"])), k, p, T)
    if not st["done"]:
        def seen(a, rho):
            tried.append((a, rho, "climbers"))
            return verdict(a, rho)
        resume(st, seen, R, p, T)
    return (st["ok"], T(st["rho"]), T(st["ro"]), st["nf"], st["wrote"]), tried


# ---- the staged sequence on a batch, over the task-by-task walk ----
class LadderSequence:
    """mixin over GS.SubtreeSim / FS.SubtreeSimF32: `call` runs a batch through the launches of launch_subtrees with subtree_ladder = R.
    A forward pass of (problem, rho) is one walk of SubtreeSim.factor — stage by stage, the tasks of a stage forwards or reversed — and
    is kept per (problem, rho): a rung repeats the walk at another rho, never at the same one.  self.passes: the launches in order, as
    (kind, rung, problems the launch has work for)."""
    T = F64
    inertia_override = None      # {(problem, attempt): bool}: a hand-made inertia sequence in place of the factorisation's verdict

    def _inner(self, vals, rhs, p):
        if not self.ncond:
            return np.asarray(vals, self.T), np.asarray(rhs, self.T), 0, 0
        cb = self.condense(vals, rhs)
        nmat = len(cb) - self.N
        if self.T is F32:
            xpos, xzer = self.cond_inertia(vals, p[0])
        else:
            dr = np.asarray(vals)[self.r_dsrc]
            xpos, xzer = int((dr > p[0]).sum()), int((np.abs(dr) <= p[0]).sum())
        return cb[:nmat].copy(), cb[nmat:], xpos, xzer

    def _forward(self, b, inner, nvar, p, attempt, rho):
        key = (b, None if rho is None else self.T(rho).tobytes())
        if key not in self._walks:
            cv, crhs, xpos, xzer = inner
            L, npos, nzer = self.factor(cv, crhs, nvar, p[0], rho)
            assert sorted(self.trace) == list(range(self.ntasks))
            self._walks[key] = (L, npos + xpos == nvar and nzer + xzer == 0)
        L, ok = self._walks[key]
        if self.inertia_override and (b, attempt) in self.inertia_override:
            ok = self.inertia_override[b, attempt]
        return L, bool(ok)

    def call(self, vals, rhs, nvar, rho_old, params, R, memo=None):
        """vals [B][nnz] (its rho slots are rewritten as the commit and the climbers rewrite them), rhs [B][N], rho_old [B].
        memo: a dict that keeps the walks between calls on the SAME inputs (other R, other rhomax); None: nothing is kept.
        Returns dict(d [B][N] — NaN rows where no backward sweep ran —, ok, rho, ro, nf, slots [B] — the last rho tried, NaN: untouched)."""
        T = self.T
        p = np.asarray(params, T)
        B, S = len(vals), len(self.stage_ptr) - 1
        self._walks = {} if memo is None else memo
        inner = [self._inner(np.asarray(vals[b], T), np.asarray(rhs[b], T), p) for b in range(B)]
        everyone = list(range(B))
        self.passes = []
        Ls = [None] * B
        # the first attempt: S forward launches, the first decide
        first_ok = []
        for b in everyone:
            Ls[b], ok = self._forward(b, inner[b], nvar, p, 0, None)
            first_ok.append(ok)
        self.passes += [("forward", 0, everyone)] * S + [("decide", 0, everyone)]
        if R == 0:
            # the parent's sequence: backward stages of the successes, then the climbers — the complete sequential call of a failure
            st = [dict(done=DONE_FIRST if ok else DONE_CLIMBING, ok=ok, rho=T(0), ro=T(rho_old[b]), nf=1, wrote=None) for b, ok in zip(everyone, first_ok)]
            d = self._backward_stages(st, Ls, inner, vals, rhs, S)
            climbing = [b for b in everyone if not st[b]["ok"]]
            for b in climbing:
                def verdict(a, rho, b=b):
                    Ls[b], ok = self._forward(b, inner[b], nvar, p, a, rho)
                    return ok
                ok, rho, ro, nf, wrote = reference_ladder(verdict, rho_old[b], p, T)
                st[b].update(ok=ok, rho=rho, ro=ro, nf=nf, wrote=wrote)
                if ok:
                    d[b] = self._solution(Ls[b], vals[b], rhs[b])
            self.passes.append(("climbers", 0, climbing))
            return self._outputs(st, d, vals, nvar)
        st = [first_decide(ok, rho_old[b], p, T) for b, ok in zip(everyone, first_ok)]
        # the rungs: S forward launches and a rung decide each, whatever the batch needs
        for k in range(1, R + 1):
            active = [b for b in everyone if not st[b]["done"]]
            for b in active:
                Ls[b], ok = self._forward(b, inner[b], nvar, p, k, st[b]["next"])
                rung_decide(st[b], ok, k, p, T)
            self.passes += [("forward", k, active)] * S + [("decide", k, active)]
        # the backward stages behind the last rung, for every problem whose flag is 1
        d = self._backward_stages(st, Ls, inner, vals, rhs, S)
        # the commit: the rho slots of the problems that finished inside the rungs
        committed = [b for b in everyone if st[b]["done"] == DONE_RUNGS]
        self.passes.append(("commit", 0, committed))
        # the climbers skip on done and resume the others
        climbing = [b for b in everyone if not st[b]["done"]]
        for b in climbing:
            def verdict(a, rho, b=b):
                Ls[b], ok = self._forward(b, inner[b], nvar, p, a, rho)
                return ok
            resume(st[b], verdict, R, p, T)
            if st[b]["ok"]:
                d[b] = self._solution(Ls[b], vals[b], rhs[b])
        self.passes.append(("climbers", 0, climbing))
        return self._outputs(st, d, vals, nvar)

    def _solution(self, L, vals, rhs):
        d2 = self.backward(L)
        return self.expand(np.asarray(vals, self.T), np.asarray(rhs, self.T), d2) if self.ncond else d2

    def _backward_stages(self, st, Ls, inner, vals, rhs, S):
        n = self.Nout if self.ncond else self.N
        d = np.full((len(st), n), np.nan, self.T)
        have = [b for b in range(len(st)) if st[b]["ok"]]
        for b in have:
            d[b] = self._solution(Ls[b], vals[b], rhs[b])
        self.passes += [("backward", 0, have)] * S
        return d

    def _outputs(self, st, d, vals, nvar):
        T = self.T
        slots = np.full(len(st), np.nan, T)
        for b, s in enumerate(st):
            if s["wrote"] is not None:
                slots[b] = s["wrote"]
                vals[b][len(vals[b]) - nvar:] = s["wrote"]
        return dict(d=d, ok=np.array([s["ok"] for s in st], bool), rho=np.array([s["rho"] for s in st], T), ro=np.array([s["ro"] for s in st], T),
                    nf=np.array([s["nf"] for s in st], np.int64), slots=slots)


class SubtreeLadderSim(LadderSequence, GS.SubtreeSim):
    T = F64


class SubtreeLadderSimF32(LadderSequence, FS.SubtreeSimF32):
    T = F32


def classic_reference(sim, vals, rhs, nvar, nequ, ncon, rho_old, params, T=F64):
    """PlanSim.newton_system (the sequential walk over the classic table) on every problem of a batch, with the last rho it tried:
    the dict LadderSequence.call returns (d rows of failures NaN)"""
    B = len(vals)
    out = dict(d=[], ok=[], rho=[], ro=[], nf=[], slots=[])
    factor = sim.factor
    for b in range(B):
        tried = []

        def spy(v, r, n, tol, rho=None):
            tried.append(rho)
            return factor(v, r, n, tol, rho)
        sim.factor = spy
        try:
            d, ok, rho, ro, nf = sim.newton_system(np.array(vals[b], T), np.asarray(rhs[b], T), nvar, nequ, ncon, T(rho_old[b]), np.asarray(params, T))
        finally:
            del sim.factor
        assert tried[0] is None and len(tried) == nf
        out["d"].append(np.asarray(d, T) if ok else np.full(len(d), np.nan, T))
        out["ok"].append(bool(ok)); out["rho"].append(T(rho)); out["ro"].append(T(ro)); out["nf"].append(int(nf))
        out["slots"].append(T(tried[-1]) if nf > 1 else T(np.nan))
    return {k: np.array(v) for k, v in out.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


def assert_same_outputs(got, want, what=""):
    """two output dicts (d, ok, rho, ro, nf, slots) bit for bit"""
    for k in ("ok", "nf"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in ("rho", "ro", "slots", "d"):
        assert got[k].dtype == want[k].dtype and np.array_equal(bits(got[k]), bits(want[k])), (what, k, got[k], want[k])


# ---- the ends a problem can come to, from the oracle's results ----
def ends(c, R, f32=False):
    """the end of every problem of a case under subtree_ladder = R, from the ORACLE's results and the case's parameters alone:
    'first', 'rung' (success at rung k <= R, rho_old updated), 'rung-above-rhomax' (success at rho_1 > rhomax, rho_old kept),
    'exhausted-inside' (failure decided before rung R), 'exhausted-at-R' (failure decided by the decide of rung R, rho_{R+1} > rhomax),
    'resumed-ok', 'resumed-failed'"""
    p = np.asarray(c["p32"] if f32 else c["params"], F64)
    out = []
    for b in range(len(c["ok"])):
        ok, nf, rho, ro_in, ro_out = bool(c["ok"][b]), int(c["nf"][b]), float(c["rho"][b]), float(c["rho_old"][b]), float(c["ro"][b])
        if nf == 1:
            out.append("first")
        elif nf - 1 <= R:      # the last attempt is rung nf - 1
            if ok:
                out.append("rung" if rho <= p[6] and ro_out == rho else "rung-above-rhomax")
                assert out[-1] == "rung" or (nf == 2 and ro_out == ro_in)
            else:
                out.append("exhausted-at-R" if nf - 1 == R else "exhausted-inside")
        else:
            out.append("resumed-ok" if ok else "resumed-failed")
    return out
