"""What the tests of the Float32 Direct route share (tuning float32_general = 1, float32_register_front = 1,
float32_direct_records = 1: the float instantiation of csrc/kernels2.hip on direct records — it condenses on the fly from the
caller's vals, a call is the launch and the post-pass): the plan options, the handle, and `check`.  The reference, tolerances and
margin assertion are those of tests/support/f32_general.py (oracle_newton / check_results, unchanged); the named cases, inputs,
the one-launch assertion and the shared oracle runs those of tests/support/f32_register_front.py.

Run as a script (python -m tests.support.f32_direct) it computes five cases and prints one line of hexadecimal digests per case:
the test of what earlier kernels left behind runs it in child processes and compares the lines."""
import hashlib

import numpy as np

from tests.support import f32_general as G
from tests.support import f32_register_front as R

KEYS = dict(float32_general=1, float32_register_front=1, float32_direct_records=1)
# the plan cnl_create_f32_ex builds for such a handle, as Plan options (the library forces the same switches internally)
DIRECT_PLAN = dict(plan_kind=1, condense=1, register_front=1, direct_records=1, lean_kernel=0, rows_in_backward=0, dense_backend=0,
                   general_dense=0, staged=0, band_kernel=0, **KEYS)
CONDENSED_PLAN = dict(DIRECT_PLAN, direct_records=0)

mods = R.mods
launches = R.launches
newton = R.newton


def handle(hipldl, s, B, direct=True, **opt):
    rows, cols = s.kkt_pattern()
    L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32, options=hipldl.Options(**KEYS, **opt))
    assert L.dtype == np.float32
    assert L.config["float32"] and not L.config["band"] and L.config["kernel"] == "v2", L.config
    assert L.config["direct"] == direct, L.config
    assert L.info["ncond"] > 0, L.info
    return L


def check(key, s, vals, rhs, rho_old=0.0, L=None, **opt):
    """newton_system_ on a direct handle against the oracle run `key` names (shared with the register-front tests' runs)"""
    hipldl, syn, O = mods()
    B = vals.shape[0]
    ro32 = np.full(B, rho_old, np.float32)
    own = L is None
    if own:
        L = handle(hipldl, s, B, **opt)
    v, d, ok, rho, ro, nf = newton(hipldl, s, L, vals, rhs, ro32)   # (asserts: one launch of family 1, none of the others)
    if B == 1:   # the drop-in case: scalars, as the reference returns them
        assert isinstance(ok, bool) and isinstance(rho, float) and isinstance(ro, float) and isinstance(nf, int)
    ref = R.ref_of(O, hipldl, (key, float(rho_old)), s, vals, rhs, ro32)
    be, fe = G.check_results(s, ref, v, rhs, d, ok, rho, ro, nf)
    print(f"{key}: backward error {be / G.EPS32:.1f} eps32, forward error {fe:.2e}, nfact {sorted(set(ref['nf'].tolist()))}, "
          f"wpb {L.config['wpb']} lds {L.config['lds2_bytes']} v2_solve {L.config['v2_solve']}")
    out = (np.asarray(d).reshape(B, s.N).copy(), ref, v, (np.asarray(ok).reshape(B), np.asarray(nf).reshape(B), np.asarray(rho).reshape(B)))
    if own:
        L.close()
    return out


def main():
    hipldl, syn, O = mods()
    for key, s, vals, rhs, opt in R.first_four_cases(syn):
        B = vals.shape[0]
        L = handle(hipldl, s, B, **opt)
        out = newton(hipldl, s, L, vals, rhs, np.zeros(B, np.float32))
        L.close()
        print(key, " ".join(hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16] for x in out))
    print("done")


if __name__ == "__main__":
    main()
