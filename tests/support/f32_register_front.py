"""What the tests of the Float32 register-front kernel share (tuning float32_general = 1, float32_register_front = 1: the float
instantiation of csrc/kernels2.hip between the float condensation passes): the handle, the one-launch assertion, the named cases,
and `check` — that of tests/test_float32_general_gpu.py with the reference, tolerances and margin assertion of
tests/support/f32_general.py (oracle_newton / check_results, unchanged).

Run as a script (python -m tests.support.f32_register_front) it computes the first four cases of the table and prints one line of
hexadecimal digests per case: the test of what earlier kernels left behind runs it in child processes and compares the lines."""
import hashlib

import numpy as np

from tests.support import f32_general as G

# the plan cnl_create_f32_ex builds for such a handle, as Plan options (the library forces the same switches internally)
RF_PLAN = dict(plan_kind=1, condense=1, register_front=1, direct_records=0, dense_backend=0, general_dense=0, staged=0, band_kernel=0,
               float32_general=1, float32_register_front=1)


def mods():
    import cannoles_jl_amd  # noqa: F401
    from cannoles_jl_amd import hipldl, synthetic as syn
    from oracle import oracle as O
    return hipldl, syn, O


def handle(hipldl, s, B, kernel="v2", **opt):
    rows, cols = s.kkt_pattern()
    L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32,
                            options=hipldl.Options(float32_general=1, float32_register_front=1, **opt))
    assert L.dtype == np.float32
    assert L.config["float32"] and not L.config["band"] and L.config["kernel"] == kernel, L.config
    assert L.info["ncond"] > 0, L.info
    return L


def launches(hipldl, c0, register_front=0, general=0):
    """exactly these launches of families 1 / 2 since c0, and none of family 0"""
    c1 = hipldl.launch_counts()
    got = (c1["band"] - c0["band"], c1["register_front"] - c0["register_front"], c1["general"] - c0["general"])
    assert got == (0, register_front, general), (c0, c1)


def newton(hipldl, s, L, vals, rhs, ro32, fill=0.0):
    B = vals.shape[0]
    p32 = hipldl.default_params(np.float32)
    v = vals.copy()
    c0 = hipldl.launch_counts()
    d, ok, rho, ro, nf = hipldl.newton_system_(np.full((B, s.N) if B > 1 else s.N, fill, np.float32), s.nvar, s.nequ, s.ncon,
                                               rhs if B > 1 else rhs[0], v if B > 1 else v[0], L, ro32 if B > 1 else ro32[0], p32)
    if L.config["kernel"] == "v2":
        launches(hipldl, c0, register_front=1)
    else:
        launches(hipldl, c0, general=1)
    return v, d, ok, rho, ro, nf


_refs = {}


def ref_of(O, hipldl, key, s, vals, rhs, ro32):
    """one oracle run per named input set, shared by the tests that use it (never modified)"""
    if key not in _refs:
        _refs[key] = G.oracle_newton(O, s, vals, rhs, ro32, hipldl.default_params(np.float32))
    return _refs[key]


def check(key, s, vals, rhs, rho_old=0.0, L=None, **opt):
    hipldl, syn, O = mods()
    B = vals.shape[0]
    ro32 = np.full(B, rho_old, np.float32)
    own = L is None
    if own:
        L = handle(hipldl, s, B, **opt)
    v, d, ok, rho, ro, nf = newton(hipldl, s, L, vals, rhs, ro32)
    if B == 1:   # the drop-in case: scalars, as the reference returns them
        assert isinstance(ok, bool) and isinstance(rho, float) and isinstance(ro, float) and isinstance(nf, int)
    ref = ref_of(O, hipldl, (key, float(rho_old)), s, vals, rhs, ro32)
    be, fe = G.check_results(s, ref, v, rhs, d, ok, rho, ro, nf)
    print(f"{key}: backward error {be / G.EPS32:.1f} eps32, forward error {fe:.2e}, nfact {sorted(set(ref['nf'].tolist()))}, "
          f"wpb {L.config['wpb']} lds {L.config['lds2_bytes']} v2 {L.info['v2']}")
    out = (np.asarray(d).reshape(B, s.N).copy(), ref, v, (np.asarray(ok).reshape(B), np.asarray(nf).reshape(B), np.asarray(rho).reshape(B)))
    if own:
        L.close()
    return out


# ---- the named cases of the table ----
def chain(syn):
    return syn.band_structure(60, 2, hw=3)


def chain_inputs(syn, s, ladder=False):
    return G.band_inputs(syn, s, range(7000, 7013), stress="ladder") if ladder else G.band_inputs(syn, s, range(4000, 4013))


def class32(syn):
    return syn.random_structure(30, 40, 2, 0.15, seed=1)


def class64(syn):
    return syn.random_structure(60, 80, 4, 0.1, seed=3)


def mixed_classes(syn):
    return syn.random_structure(40, 56, 2, 0.06, seed=3)


def mixed_batch(syn, s):
    """the class-64 posdef batch with problem 5 replaced by an indefinite one: a mixed ladder inside the wavefront of problems 4 - 7"""
    vals, rhs = G.random_inputs(syn, s, range(100, 124))
    v5, r5 = G.random_inputs(syn, s, [205], posdef=False)
    vals[5], rhs[5] = v5[0], r5[0]
    return vals, rhs


def first_four_cases(syn):
    """(key, structure, vals, rhs, options) of the first four rows of the table"""
    s = chain(syn)
    s32 = class32(syn)
    return [("chain", s) + chain_inputs(syn, s) + ({},),
            ("chain-ladder", s) + chain_inputs(syn, s, ladder=True) + ({},),
            ("chain-global-scratch", s) + chain_inputs(syn, s) + (dict(ubig=4),),
            ("class32", s32) + G.random_inputs(syn, s32, range(100, 113)) + ({},),
            ("class32-indefinite", s32) + G.random_inputs(syn, s32, range(200, 213), posdef=False) + ({},)]


def main():
    hipldl, syn, O = mods()
    for key, s, vals, rhs, opt in first_four_cases(syn):
        B = vals.shape[0]
        L = handle(hipldl, s, B, **opt)
        out = newton(hipldl, s, L, vals, rhs, np.zeros(B, np.float32))
        L.close()
        print(key, " ".join(hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16] for x in out))
    print("done")


if __name__ == "__main__":
    main()
