"""What the tests of the Float32 latency path share (tuning float32_general = 1, float32_latency = 1: the latency plan of
float32_staged shaped and run as a Float64 handle's — lean instances, dataflow, the fused in-kernel ladder — on the float instances
named last in csrc/kernels2.hip).  Inputs, shapes, the reference, the tolerances and the margin assertion are those of
tests/support/f32_staged.py and f32_general.py, unchanged; the handle helper is this module's own (a lean handle is what the key is for).

Run as a script (python -m tests.support.f32_latency) it computes two cases and prints one line of hexadecimal digests per case: the
test of what earlier kernels left behind runs it in child processes and compares the lines."""
import hashlib

import numpy as np

from tests.support import f32_staged as S
from tests.support.rec_sim import B_ROWS_FLAG, R_FLAGS, R_HDR, R_NPROD, R_RECLEN, RF_FS_GLOBAL, RF_ROWS

KEYS = dict(float32_general=1, float32_latency=1, band_kernel=0)
PLAN_KEYS = dict(float32_general=1, float32_latency=1)
# every part switched off: the plan and the handle of float32_staged = 1
ALL_OFF = dict(lean_kernel=0, rows_in_backward=0, dataflow=0, device_ladder=0)

# (shape, batch) -> (tasks, stages, fronts of class 16 / 32 / 64, lean) of the float plan WITH the key: hw2 and cfg4 are lean (every
# front takes the row form — cfg4's order has one front with more than 16 residual rows, cut in two: 180 fronts where the plan of
# float32_staged has 179 —, backward rows); hw3's two class-32 fronts keep it on the non-lean instances, and its plan is the plan
# of float32_staged
PLANS = {("hw2", 1): (9, 3, (32, 0, 0), True), ("hw2", 13): (9, 3, (32, 0, 0), True), ("hw2", 256): (9, 3, (32, 0, 0), True),
         ("hw3", 13): (21, 6, (69, 2, 0), False), ("hw3", 64): (14, 4, (69, 2, 0), False),
         ("cfg4", 32): (57, 6, (180, 0, 0), True), ("cfg4", 256): (29, 5, (180, 0, 0), True),
         # the smallest batch of cfg4's pattern whose 29 tasks do not fit 2 048 resident wavefronts in ONE fused launch: 71 groups of
         # four problems, 70 slots of 29 wavefronts (280 problems: 70 groups, one launch) — found by the search of the CPU test
         ("cfg4", 281): (29, 5, (180, 0, 0), True),
         ("cfg4", 4096): (3, 2, (100, 0, 0), True),
         # [added] the chain launch_newton2_staged's rule gives the LATE instance (S.late_rule): here the staged LEAN one in its LATE setting
         ("late", 3840): (3, 2, (260, 0, 0), True)}
MULTI_LAUNCH = ("cfg4", 281)
RESIDENT_FULL = 2048   # 256 CUs x 8 wavefronts


def listprod_fronts(plan_array, nsuper):
    """fast fronts whose condensation products come as lists (csrc/analysis.cpp: Plan::listprod_fronts), from the forward records"""
    rec = plan_array("rec").astype(np.int64)
    off = n = 0
    for _ in range(nsuper):
        H = rec[off:off + R_HDR]
        flags, cls = int(H[R_FLAGS]) & 0xff, int(H[R_FLAGS]) >> 8
        n += bool(cls == 16 and not (flags & RF_FS_GLOBAL) and not (flags & RF_ROWS) and (int(H[R_NPROD]) & 0xffff) > 0)
        off += int(H[R_RECLEN])
    return n


def back_rows(plan_array):
    return bool(plan_array("brec")[7] & B_ROWS_FLAG)


def fused_launches(ntasks, B, resident, fused=0):
    """setup_v2's ladder rule (csrc/capi_handle.cpp): (lad_mode, fused launches the batch needs); lad_mode 1 is the default — the
    fused ladder behind a staged first attempt —, 2 with device_ladder_fused = 1: the launch makes the first attempt too"""
    if resident < ntasks:
        return 0, 0
    slots, nq = resident // ntasks, (B + 3) // 4
    launches = (nq + slots - 1) // slots
    return ((2 if fused else 1) if launches == 1 or (launches <= 4 and ntasks >= 16) else 0), launches


def resident_waves(torch, config):
    """wavefronts of the register-front kernel the device holds at once, as setup_v2 counts them"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    by_lds = (160 * 1024 // config["lds2_bytes"]) * config["wpb"]
    return cus * max(1, min(8, by_lds))


def handle(hipldl, s, B, lean, df=True, lad_mode=None, **opt):
    rows, cols = s.kkt_pattern()
    L = hipldl.HIPLDLStruct(s.N, rows, cols, None, s.nvar, s.nequ, s.ncon, batch=B, dtype=np.float32, options=hipldl.Options(**KEYS, **opt))
    assert L.dtype == np.float32
    assert L.config["float32"] and not L.config["band"] and L.config["direct"] and L.config["kernel"] == "v2-staged", L.config
    assert L.info["ncond"] > 0
    assert L.config["lean"] == lean and L.config["dataflow"] == df, L.config
    assert L.config["lean"] == L.uses_lean_kernel()
    if lean:
        assert L.config["v2_solve"] and listprod_fronts(L.plan_array, L.info["nsuper"]) == 0
    if lad_mode is not None:
        assert L.config["lad_mode"] == lad_mode, L.config
    return L


def three_batches(hipldl, shape, B, L):
    """clean, mixed (climbers and a hopeless problem in one wavefront, a climber in another; RHO_MAX_SMALL), clean again — on one handle"""
    _, ref, _, _ = S.check(shape, "clean", B, L=L)
    assert ref["ok"].all() and (ref["nf"] == 1).all()
    _, ref, _, (ok, nf, _) = S.check(shape, "mixed", B, L=L)
    if B > S.HOPELESS:
        assert not ref["ok"][S.HOPELESS] and ref["nf"][S.HOPELESS] == 4 and ref["ok"][list(S.CLIMBERS[:2])].all() and (ref["nf"][1:3] == 4).all()
        assert int((~ok).sum()) == len(range(S.HOPELESS, B, S.NDISTINCT))
    S.check(shape, "clean", B, L=L)


CASES = (("hw2", "mixed", 13, True), ("hw3", "mixed", 13, False))


def main():
    hipldl, syn, O = S.mods()
    for shape, kind, B, lean in CASES:
        s = S.structure(syn, shape)
        v13, r13 = S.distinct_inputs(syn, s, kind)
        L = handle(hipldl, s, B, lean)
        out = S.newton(hipldl, s, L, S.tiled(v13, B), S.tiled(r13, B), np.zeros(B, np.float32), S.params(hipldl, kind == "mixed"), fill=5.0)
        L.close()
        print(shape, kind, " ".join(hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16] for x in out))
    print("done")


if __name__ == "__main__":
    main()
