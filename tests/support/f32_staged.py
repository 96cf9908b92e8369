"""What the tests of staged execution in Float32 share (tuning float32_general = 1, float32_staged = 1: a latency plan on direct
records, run stage by stage on the staged float instances of csrc/kernels2.hip, one launch per stage; the problems that fail the
first attempt climb the rho ladder in the classic float launch behind it).  The reference, tolerances and margin assertion are those
of tests/support/f32_general.py (oracle_newton / check_results, unchanged).

The shapes are the issue's; the task and stage counts are those of the FLOAT plan (lean_kernel = 0, rows_in_backward = 0), asserted
by tests/test_float32_staged_cpu.py.  Batches above 13 problems repeat 13 distinct problems (problem b is problem b % 13): one
oracle run per named input set, and every copy of a problem must give the bits of its first copy.

Run as a script (python -m tests.support.f32_staged) it computes four cases and prints one line of hexadecimal digests per case:
the test of what earlier kernels left behind runs it in child processes and compares the lines."""
import hashlib

import numpy as np

from tests.support import f32_general as G
from tests.support import f32_register_front as R

# band_kernel = 0: a band pattern goes to the band kernels first (cnl_create_f32_ex), and the shapes here are band patterns
KEYS = dict(float32_general=1, float32_staged=1, band_kernel=0)
# "the same options without the key": the keys it implies, written out
UNSTAGED = dict(float32_general=1, float32_register_front=1, float32_direct_records=1, band_kernel=0)
PLAN_KEYS = dict(float32_general=1, float32_staged=1)

SHAPES = {"hw2": (200, 4, 2), "hw3": (200, 4, 3), "cfg4": (1000, 10, 2), "late": (2600, 4, 2)}
# (shape, batch) -> (tasks, stages, fronts of class 16 / 32 / 64, v2_solve) of the float plan
PLANS = {("hw2", 1): (9, 3, (32, 0, 0), True), ("hw2", 13): (9, 3, (32, 0, 0), True), ("hw2", 256): (9, 3, (32, 0, 0), True),
         ("hw3", 13): (21, 6, (69, 2, 0), False), ("hw3", 64): (14, 4, (69, 2, 0), False),
         # [the issue's analysis, run with the Float64 tuning, gave 29 tasks in 5 stages at 32 problems too; the float plan has 55 in 6]
         ("cfg4", 32): (55, 6, (179, 0, 0), True), ("cfg4", 256): (29, 5, (179, 0, 0), True),
         ("cfg4", 4096): (3, 2, (100, 0, 0), True),   # the bidirectional chain: 100 fronts, too few for the late instance (late_rule)
         # [added: the smallest chain the rule gives the LATE instance — 960 groups of problems x 2 first-stage tasks, 260 >= 256 fronts]
         ("late", 3840): (3, 2, (260, 0, 0), True)}
NDISTINCT = 13
RHO_MAX_SMALL = 100.0   # with it a problem whose Hessian needs the rung behind 20.16 is hopeless (the next one is 1290 > 100)

mods = R.mods
bits = G.bits


def structure(syn, shape):
    n, p, hw = SHAPES[shape]
    return syn.band_structure(n, p, hw=hw)


def late_rule(B, stage_ptr, nsuper):
    """launch_newton2_staged's rule for the instance that stores its L rows one front late (csrc/kernels2.hip), from the host's facts"""
    nquads, ntask0 = (B + 3) // 4, int(stage_ptr[1] - stage_ptr[0])
    return nquads * ntask0 >= 1920 and nsuper >= 128 * ntask0


def params(hipldl, small_rhomax=False):
    p = hipldl.default_params(np.float32)
    if small_rhomax:
        p[6] = RHO_MAX_SMALL
    return p


def distinct_inputs(syn, s, kind):
    """13 problems: "clean" (every problem factorises at rho = 0), or "mixed": climbers at 1 and 2 (the wavefront of problems 0 - 3),
    a hopeless problem at 3 (same wavefront: its Hessian's negative diagonal is five times a climber's) and a climber at 9 (another
    wavefront); to be run with params(small_rhomax=True)"""
    vals, rhs = G.band_inputs(syn, s, range(4000, 4000 + NDISTINCT))
    if kind == "clean":
        return vals, rhs
    assert kind == "mixed"
    lv, lr = G.band_inputs(syn, s, range(7000, 7004), stress="ladder")
    off = s.offsets()
    h = lv[2, off[0]:off[1]]
    lv[2, off[0]:off[1]] = np.where(h == np.float32(-10.0), np.float32(-50.0), h)
    for at, k in ((1, 0), (2, 1), (3, 2), (9, 3)):
        vals[at], rhs[at] = lv[k], lr[k]
    return vals, rhs


CLIMBERS, HOPELESS = (1, 2, 9), 3


def tiled(a, B):
    return np.ascontiguousarray(a[np.arange(B) % NDISTINCT]) if B > NDISTINCT else np.ascontiguousarray(a[:B])


def handle(hipldl, s, B, staged=True, keys=KEYS, **opt):
    rows, cols = s.kkt_pattern()
    L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32, options=hipldl.Options(**keys, **opt))
    assert L.dtype == np.float32
    assert L.config["float32"] and not L.config["band"] and L.config["direct"], L.config
    assert L.config["kernel"] == ("v2-staged" if staged else "v2"), L.config
    assert L.info["ncond"] > 0 and not L.config["lean"], (L.info, L.config)
    return L


def newton(hipldl, s, L, vals, rhs, ro32, p32=None, fill=0.0):
    """the host entry; on a staged handle the register-front family counts ONE launch (the classic launch behind the staged
    attempt — the launches of the stages are not counted, as on a Float64 handle), the general kernel none"""
    B = vals.shape[0]
    p32 = params(hipldl) if p32 is None else p32
    v = vals.copy()
    c0 = hipldl.launch_counts()
    d, ok, rho, ro, nf = hipldl.newton_system_(np.full((B, s.N) if B > 1 else s.N, fill, np.float32), s.nvar, s.nequ, s.ncon,
                                               rhs if B > 1 else rhs[0], v if B > 1 else v[0], L, ro32 if B > 1 else ro32[0], p32)
    R.launches(hipldl, c0, register_front=1)
    return v, d, ok, rho, ro, nf


_refs = {}


def ref_of(O, hipldl, key, s, vals, rhs, ro32, p32):
    """one oracle run per named set of 13 problems (never modified); `expand` makes the reference of a tiled batch of it"""
    if key not in _refs:
        _refs[key] = G.oracle_newton(O, s, vals, rhs, ro32, p32)
    return _refs[key]


def expand(ref, B):
    return {k: tiled(v, B) for k, v in ref.items()}


def check(shape, kind, B, rho_old=0.0, L=None, **opt):
    """newton_system_ on a staged handle against the oracle; returns (d, ref, vals out, (ok, nf, rho))"""
    hipldl, syn, O = mods()
    s = structure(syn, shape)
    v13, r13 = distinct_inputs(syn, s, kind)
    p32 = params(hipldl, small_rhomax=kind == "mixed")
    ref = expand(ref_of(O, hipldl, (shape, kind, float(rho_old)), s, v13, r13, np.full(NDISTINCT, rho_old, np.float32), p32), B)
    vals, rhs = tiled(v13, B), tiled(r13, B)
    own = L is None
    if own:
        L = handle(hipldl, s, B, **opt)
    v, d, ok, rho, ro, nf = newton(hipldl, s, L, vals, rhs, np.full(B, rho_old, np.float32), p32, fill=5.0)
    if B == 1:
        assert isinstance(ok, bool) and isinstance(rho, float) and isinstance(ro, float) and isinstance(nf, int)
    d = np.asarray(d).reshape(B, s.N)
    be, fe = G.check_results(s, ref, v, rhs, d, ok, rho, ro, nf, rows=range(min(B, NDISTINCT)))
    okv = np.asarray(ok, bool).reshape(B)
    assert (d[~okv] == 5.0).all()            # a failed problem leaves d untouched
    if B > NDISTINCT:                         # every copy of a problem: the bits of its first copy
        assert np.array_equal(bits(d), bits(d[np.arange(B) % NDISTINCT]))
    print(f"{shape}/{kind}/B={B}: backward error {be / G.EPS32:.1f} eps32, forward error {fe:.2e}, nfact {sorted(set(ref['nf'].tolist()))}, "
          f"wpb {L.config['wpb']} lds {L.config['lds2_bytes']} v2_solve {L.config['v2_solve']}")
    out = (d.copy(), ref, v, (okv, np.asarray(nf).reshape(B), np.asarray(rho).reshape(B)))
    if own:
        L.close()
    return out


# ---- the numpy float32 model: decisions of newton_system! on an unpivoted LDL' in float32, in the plan's elimination order ----
def _inertia32(K32, eig_tol):
    """(npos, nzero) of the D of K = L D L' with every operation in float32; K32: dense, symmetric, already permuted"""
    A = K32.copy()
    n = A.shape[0]
    npos = nzer = 0
    for j in range(n):
        dj = A[j, j]
        npos += bool(dj > eig_tol)
        nzer += bool(abs(dj) <= eig_tol)
        nz = j + 1 + np.nonzero(A[j + 1:, j])[0]
        if nz.size:
            col = A[nz, j].copy()
            A[np.ix_(nz, nz)] -= np.outer(col / dj, col).astype(np.float32)
    return npos, nzer


def model_newton32(s, perm, vals32, rho_old, p32):
    """(success, nfact, rho, rho_old) of src/CaNNOLeS.jl:1023-1047 on the float32 model"""
    rows, cols = s.kkt_pattern()
    r, c = np.asarray(rows) - 1, np.asarray(cols) - 1
    inv = np.empty(s.N, np.int64)
    inv[np.asarray(perm, np.int64)] = np.arange(s.N)
    f = np.float32
    eig_tol, kdec, kinc, klarge, rho0, rhomax, rhomin = f(p32[0]), f(p32[2]), f(p32[3]), f(p32[4]), f(p32[5]), f(p32[6]), f(p32[7])
    vals = np.array(vals32, np.float32)

    def ok_at(rho):
        v = vals.copy()
        if rho is not None:
            v[-s.nvar:] = rho
        K = np.zeros((s.N, s.N), np.float32)
        np.add.at(K, (inv[r], inv[c]), v)
        K = K + np.tril(K, -1).T + np.triu(K, 1).T
        npos, nzer = _inertia32(K, eig_tol)
        return npos == s.nvar and nzer == 0

    rho_old = f(rho_old)
    rho, nfact = f(0.0), 1
    ok = ok_at(None)
    if not ok:
        rho = rho0 if rho_old == 0 else max(rhomin, f(kdec * rho_old))
        while True:
            ok = ok_at(rho)
            nfact += 1
            if ok or rho > rhomax:
                break
            rho = f(klarge * rho) if rho_old == 0 else f(kinc * rho)
            if rho > rhomax:
                break
        if rho <= rhomax:
            rho_old = rho
    return ok, nfact, float(rho), float(rho_old)


CASES = (("hw2", "clean", 13), ("hw2", "mixed", 13), ("hw3", "clean", 13), ("hw3", "mixed", 13))


def main():
    hipldl, syn, O = mods()
    for shape, kind, B in CASES:
        s = structure(syn, shape)
        v13, r13 = distinct_inputs(syn, s, kind)
        L = handle(hipldl, s, B)
        out = newton(hipldl, s, L, tiled(v13, B), tiled(r13, B), np.zeros(B, np.float32), params(hipldl, kind == "mixed"), fill=5.0)
        L.close()
        print(shape, kind, " ".join(hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16] for x in out))
    print("done")


if __name__ == "__main__":
    main()
