"""Host-side mirror of the reference's linear-solver plugin surface, over the C ABI.

The reference's extension point is `abstract type LinearSolverStruct`
(/root/reference/src/solver_types.jl:1) with
  * a constructor `Backend(N, rows, cols, vals)`        (src/CaNNOLeS.jl:323,327)
  * `get_vals(LDLT)`                                      (src/solver_types.jl:25,67)
  * `try_to_factorize(LDLT, vals, nvar, nequ, ncon, eig_tol)::Bool` (solver_types.jl:79-98)
  * `solve_ldl!(rhs, LDLT.factor, d)::Bool`               (solver_types.jl:69-77)
and the driver `newton_system!` (src/CaNNOLeS.jl:1008-1052).  The same names
and argument meanings are kept here (`!` spelled `_`), so the parity tests read
like the reference's own code.  All arithmetic happens in libcannoles_hip.so
(HIP kernels); this module only marshals numpy / torch buffers through ctypes.
Julia would bind the same symbols with `ccall`.

There is no CPU fallback: if the shared library is missing, or no HIP device
is usable, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CANNOLES_HIP_LIB") or os.path.join(_HERE, "libcannoles_hip.so")  # same override as the Julia glue

_i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_lib = None

# symbols declared in include/cannoles_hip.h (checked by the CPU test-suite)
ABI_SYMBOLS = [
    "cnl_last_error", "cnl_version", "cnl_default_params",
    "cnl_options_init", "cnl_plan_create_ex", "cnl_create_ex", "cnl_dataflow_timeouts",
    "cnl_plan_create", "cnl_plan_create_for_batch", "cnl_plan_destroy", "cnl_plan_info", "cnl_plan_get", "cnl_plan_order_name",
    "cnl_create", "cnl_destroy", "cnl_get_plan",
    "cnl_factorize", "cnl_solve", "cnl_newton_system",
    "cnl_factorize_dev", "cnl_solve_dev", "cnl_newton_system_dev",
    "cnl_set_timing", "cnl_last_kernel_ms", "cnl_get_config", "cnl_launch_counts",
    "cnl_residual_vectors_dev", "cnl_trial_point_dev", "cnl_prepare_newton_system_dev",
    "cnl_cgls_multipliers_dev",
    "cnl_multi_create_ex", "cnl_multi_factorize_dev", "cnl_multi_solve_dev", "cnl_multi_newton_system_dev", "cnl_multi_synchronize",
    "cnl_multi_create", "cnl_multi_destroy", "cnl_multi_shards", "cnl_multi_factorize", "cnl_multi_solve", "cnl_multi_newton_system",
    "cnl_outer_begin_dev", "cnl_outer_newton_done_dev", "cnl_outer_extrapolated_dev", "cnl_outer_trial_done_dev", "cnl_outer_end_dev",
    "cnl_outer_ls_begin_dev", "cnl_outer_ls_test_dev", "cnl_outer_ls_step_dev", "cnl_outer_ls_take_dev",
    "cnl_layout_len", "cnl_interleave_dev", "cnl_deinterleave_dev", "cnl_residual_vectors_jac_dev", "cnl_cgls_multipliers_jac_dev",
    "cnl_default_params_f32", "cnl_create_f32", "cnl_create_f32_ex",
    "cnl_factorize_f32", "cnl_solve_f32", "cnl_newton_system_f32",
    "cnl_factorize_f32_dev", "cnl_solve_f32_dev", "cnl_newton_system_f32_dev", "cnl_interleave_f32_dev", "cnl_deinterleave_f32_dev",
    "cnl_prepare_newton_system_f32_dev", "cnl_residual_vectors_f32_dev", "cnl_residual_vectors_jac_f32_dev",
    "cnl_cgls_multipliers_f32_dev", "cnl_cgls_multipliers_jac_f32_dev", "cnl_trial_point_f32_dev",
    "cnl_outer_begin_f32_dev", "cnl_outer_newton_done_f32_dev", "cnl_outer_extrapolated_f32_dev", "cnl_outer_trial_done_f32_dev",
    "cnl_outer_end_f32_dev", "cnl_outer_ls_begin_f32_dev", "cnl_outer_ls_test_f32_dev", "cnl_outer_ls_step_f32_dev", "cnl_outer_ls_take_f32_dev",
    "cnl_set_active_batch", "cnl_get_active_batch", "cnl_outer_compact_dev", "cnl_outer_compact_f32_dev",
    "cnl_outer_begin_ex_dev", "cnl_outer_trial_done_ex_dev", "cnl_outer_ls_test_ex_dev", "cnl_outer_end_ex_dev", "cnl_outer_hess_mask_dev",
    "cnl_outer_begin_ex_f32_dev", "cnl_outer_trial_done_ex_f32_dev", "cnl_outer_ls_test_ex_f32_dev", "cnl_outer_end_ex_f32_dev",
    "cnl_outer_hess_mask_f32_dev",
    "cnl_kkt_residual_dev", "cnl_get_refine_norms",
    "cnl_subtree_stage_shape",
]

# status codes of the lockstep loop's `status` array (include/cannoles_hip.h, row f3); 7 is set by the caller, never by a kernel
OUTER_STATUS_NAMES = {0: "unknown", 1: "first_order", 2: "small_residual", 3: "exception", 4: "max_eval", 5: "stalled", 6: "max_iter",
                      7: "max_time"}


PLAN_AUTO, PLAN_THROUGHPUT, PLAN_LATENCY = 0, 1, 2
LAYOUT_PROBLEM_MAJOR, LAYOUT_INTERLEAVED = 0, 1   # cnl_options.batch_layout (include/cannoles_hip.h)
IL_GROUP = 32


def il_blocks(length):
    """blocks of eight doubles per problem of an interleaved array (one spare block; csrc/band.h: band_il_blocks)"""
    return (int(length) + 7) // 8 + 1


def il_len(batch, length):
    return (int(batch) + IL_GROUP - 1) // IL_GROUP * il_blocks(length) * IL_GROUP * 8


def il_index(p, e, length):
    """position of element e of problem p in an array interleaved over groups of 32 problems in blocks of eight doubles
    (CNL_LAYOUT_INTERLEAVED, csrc/band.h: band_il_index); p, e may be numpy arrays"""
    return ((p // IL_GROUP * il_blocks(length) + e // 8) * IL_GROUP + p % IL_GROUP) * 8 + e % 8


class cnl_options(C.Structure):
    """struct cnl_options of include/cannoles_hip.h (field order and types must match)"""
    _fields_ = [("struct_size", C.c_int32), ("plan_kind", C.c_int32), ("staged_max_batch", C.c_int64)] + [
        (k, C.c_int32) for k in ("verbose", "band_kernel", "dense_backend", "staged", "dataflow", "device_ladder", "host_ladder", "split_tail",
                                 "multi_share_plan", "batch_layout")] + [("force_order", C.c_char * 32), ("tuning", C.c_char * 192)]


_PUBLIC_OPTIONS = {f[0] for f in cnl_options._fields_} - {"struct_size", "tuning"}


class cnl_outer_state(C.Structure):
    """struct cnl_outer_state of include/cannoles_hip.h (row f3: bookkeeping of the batched outer loop); field order must match"""
    _fields_ = ([(k, C.c_int64) for k in ("B", "n", "m", "p", "P", "N", "nnzjF", "nnzjc", "max_inner")] +
                [(k, C.c_double) for k in ("dmin", "rhomax", "delta_dec", "smax")] +
                [(k, C.c_void_p) for k in (
                    "status", "it", "flags", "nf_new", "ok_new",
                    "inner", "nfact", "nlin",
                    "phase0", "act", "need", "brk", "ext", "lsm", "rej", "chk", "done_in", "tired", "small_res",
                    "normdual", "normprimal", "combined", "combined_hat", "delta", "ndh", "nph", "fx", "epsk", "epstol", "epsF", "epsc", "rho_old",
                    "d", "d_new", "ro_tmp", "rho_new",
                    "x", "r", "Fx", "cx", "Jv", "Jcv", "lam", "rhs_cur",
                    "xt", "rt", "Ft", "ct", "Jt", "Jct", "lamt", "rhs_t", "nrm_t",
                    "xt_e", "rt_e", "lamt_e")] +
                [(k, C.c_double) for k in ("gammaA", "eps2")] +
                [(k, C.c_void_p) for k in ("ls_g", "xl", "Fl", "cl", "lam_ls", "alpha", "Dphi", "phix", "eta", "nbk", "bt")])


class cnl_outer_state_f32(C.Structure):
    """struct cnl_outer_state_f32 of include/cannoles_hip.h: cnl_outer_state for a Float32 loop (float scalars; the arrays are float32)"""
    _fields_ = ([(k, C.c_int64) for k in ("B", "n", "m", "p", "P", "N", "nnzjF", "nnzjc", "max_inner")] +
                [(k, C.c_float) for k in ("dmin", "rhomax", "delta_dec", "smax")] +
                [(k, C.c_void_p) for k in (
                    "status", "it", "flags", "nf_new", "ok_new",
                    "inner", "nfact", "nlin",
                    "phase0", "act", "need", "brk", "ext", "lsm", "rej", "chk", "done_in", "tired", "small_res",
                    "normdual", "normprimal", "combined", "combined_hat", "delta", "ndh", "nph", "fx", "epsk", "epstol", "epsF", "epsc", "rho_old",
                    "d", "d_new", "ro_tmp", "rho_new",
                    "x", "r", "Fx", "cx", "Jv", "Jcv", "lam", "rhs_cur",
                    "xt", "rt", "Ft", "ct", "Jt", "Jct", "lamt", "rhs_t", "nrm_t",
                    "xt_e", "rt_e", "lamt_e")] +
                [(k, C.c_float) for k in ("gammaA", "eps2")] +
                [(k, C.c_void_p) for k in ("ls_g", "xl", "Fl", "cl", "lam_ls", "alpha", "Dphi", "phix", "eta", "nbk", "bt")])


class cnl_outer_ctl(C.Structure):
    """struct cnl_outer_ctl of include/cannoles_hip.h: the control block of the cnl_outer_*_ex_dev entry points, either element type"""
    _fields_ = [("struct_size", C.c_int32), ("always_accept_extrapolation", C.c_int32), ("max_iter", C.c_int64), ("max_eval", C.c_int64),
                ("evals_per_point", C.c_int64), ("neval", C.c_void_p), ("hess_upd", C.c_void_p)]


def outer_ctl(neval, evals_per_point, always_accept_extrapolation=False, max_iter=-1, max_eval=-1, hess_upd=None):
    """a filled cnl_outer_ctl; neval / hess_upd are device addresses (int64 [B], uint8 [B])"""
    return cnl_outer_ctl(C.sizeof(cnl_outer_ctl), int(bool(always_accept_extrapolation)), int(max_iter), int(max_eval), int(evals_per_point),
                         neval, hess_upd)


def Options(**kw):
    """cnl_options with the library's defaults (cnl_options_init), then the given switches: explicit arguments instead of
    environment variables — e.g. Options(plan_kind=PLAN_THROUGHPUT), Options(dataflow=0), Options(force_order="nd32+early").
    Fields of the public structure are set directly; any other switch of csrc/options.h (lean_kernel, band_form,
    band_problems_per_group, ...) goes into its `tuning` string as key=value — the library rejects an unknown key.
    The float32_* keys (float32_general, float32_condense, float32_register_front, float32_direct_records, float32_dense,
    float32_general_dense, float32_refine, and float32_staged = 1: latency plans of Float32 general handles run stage by stage on the
    float register-front kernel; float32_latency = 1: float32_staged plus the lean, dataflow and fused-ladder float instances, switched
    by lean_kernel, rows_in_backward, dataflow, dataflow_waves, dataflow_spin_limit, device_ladder and device_ladder_fused as on a
    Float64 handle) are described with HIPLDLStruct.  general_blocked = 1 (Float64 handles only): the general kernel eliminates fronts with
    16 pivots or more in panels of 16 with the trailing updates on the f64 matrix cores; config["general_blocked"] says whether the
    handle's launches are a blocked instance.  float32_blocked = 1 (only with float32_general = 1, not with float32_refine; 0 or 1): the
    same for a Float32 general handle, on the f32 matrix cores — where its newton_system / factorize launches are the general kernel in
    float with 256 threads per problem (a front above order 96 and no dense route; uncondensed, float32_condense, or
    float32_register_front fallen back to it); the key selects no route, 64 threads per problem run unblocked, and
    config["float32_blocked"] says whether the launches are a blocked instance.  Such a handle keeps the success flags of its last
    factorisation: solve leaves the rows of d of a failed problem untouched.  A Float64 handle without float32_refine reads nothing of
    the key (as of float32_condense).  general_subtrees = 1 (Float64 handles only; 0 or 1; combines with general_blocked): the
    elimination tree is cut into tasks — bottom subtrees of at most task_cap fronts (default 8), every front above on its own — and
    newton_system / factorize / solve run the general kernel stage by stage, one workgroup per problem and task, on a global work
    area of Plan.array("ginfo")[0] elements per problem.  It acts where the launch is the general kernel with one problem per
    workgroup of 256 or 1024 threads, the first stage has two tasks or more and batch x gwork x 8 <= 8e9 bytes;
    config["general_subtrees"] says whether it does, and every other handle is the one without the key.  Such a handle keeps the
    success flags of its last factorisation as a blocked one does.  float32_subtrees = 1 (only with float32_general = 1, not with
    float32_refine; 0 or 1; combines with float32_blocked and task_cap): the same for a Float32 general handle — where its launch is
    the general kernel in float (uncondensed, float32_condense, or float32_register_front fallen back to it) with one problem per
    workgroup of 256 threads, the first stage has two tasks or more and batch x gwork x 4 <= 8e9 bytes; config["float32_subtrees"] says
    whether it acts, every other handle is the one without the key, and general_subtrees stays refused at the Float32 creators.  A
    Float64 handle without float32_refine reads nothing of the key.  subtree_ladder = R (0 .. 64, default 0; only with general_subtrees = 1
    at a Float64 creator or float32_subtrees = 1 at a Float32 creator, never with float32_refine; else ValueError / CNL_ERR_ARG): where
    the subtree key acts, newton_system enqueues R rungs of the rho ladder behind the first attempt, each stage by stage with a decide
    launch behind it — (R + 2) S + R + 3 launches for S stages —, and the climbers' launch resumes only the problems still climbing after
    R rungs.  Every output is that of R = 0, bit for bit.  It selects no route and changes no plan; config["subtree_ladder"] is R where
    the rungs are enqueued and 0 everywhere else.  subtree_wide = W (0 .. 4096, default 0 = off) and subtree_lds_panels = M (0 = off, or
    16 .. 4096) shape the factorising forward launch of each stage of a subtree handle (newton_system, factorize, the rungs of
    subtree_ladder); both need the creator's own subtree key and refuse float32_refine, M also needs the creator's blocked key
    (general_blocked / float32_blocked); else ValueError / CNL_ERR_ARG.  With F_s the largest staging stride (word 7 of
    plan_array("gtasks")) of stage s: on a handle with 256 threads per workgroup a stage with F_s >= W and tasks_s x batch <= 2 x the
    device's CU count factorises with 1024 threads (in float the only way to a 1024-thread instance); on a blocked handle a stage with
    F_s <= M, a front of 16 pivots or more and (16 + 32 F_s) elements within the LDS of a workgroup eliminates its dependent pivot panels
    in LDS.  Backward stages, solve_ldl!, climbers and decide kernels are untouched; every output is that of the keys off, bit for
    bit; no plan, route or launch count changes.  config["subtree_wide"] / config["subtree_lds_panels"] say whether any stage is
    affected, subtree_stage_shape(LDLT) gives the table the launch loop reads.  subtree_solve_panels = P (a bit mask, 0 .. 3, default
    0 = off; needs the creator's own subtree key and refuses float32_refine, else ValueError / CNL_ERR_ARG) runs the solve sweeps of a
    subtree handle — blocked or not, 256 threads per workgroup or a 1024-thread Float64 handle — in panels of 16 pivots on kernel entries
    of their own, the front's vector in LDS and the stored panel read in place: bit 0 the backward stage launches of newton_system and
    solve (d agrees with P = 0 to rounding and is a fixed function of the front), bit 1 the forward stage launches of solve (every
    output bit-equal to P = 0).  A stage whose (round4(F_s) + 288) elements exceed the LDS of a workgroup keeps the unpanelled launch;
    factorising launches, rungs, decide / commit kernels and climbers are untouched; no plan, route, allocation or launch count
    changes.  config["subtree_solve_panels"] is the mask where it acts and 0 everywhere else.  band_cache_policy = M (0 or 7, default 7;
    any other mask ValueError / CNL_ERR_ARG at plan creation): the cache policy of the band kernel's mover-table instance — 1 typed vals
    loads, 2 typed factor loads, 4 record stores non-temporal; every output bit-equal to 0; config["band_cache_policy"] is the mask
    where that instance runs and 0 everywhere else."""
    o = cnl_options()
    lib().cnl_options_init(C.byref(o))
    assert o.struct_size == C.sizeof(cnl_options), "cnl_options layout differs from the library's"
    tun = []
    for k, v in kw.items():
        if k == "force_order":
            v = v.encode() if isinstance(v, str) else v
        if k == "tuning":
            tun.append(v.decode() if isinstance(v, bytes) else str(v))
        elif k in _PUBLIC_OPTIONS:
            setattr(o, k, v)
        else:
            tun.append(f"{k}={int(v)}")
    text = ",".join(t for t in tun if t)
    if len(text) >= 192:
        raise ValueError("cnl_options.tuning holds 191 characters")
    o.tuning = text.encode()
    return o


def _optref(options):
    if options is None:
        return None
    if isinstance(options, dict):
        options = Options(**options)
    return C.byref(options)


class CnlError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"cannoles_hip error {code}: {msg}")
        self.code = code


def loaded_hip_runtimes():
    """paths of the HIP runtimes (libamdhip64) mapped into this process"""
    try:
        with open("/proc/self/maps") as f:
            return sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    except OSError:
        return []


def _one_hip_runtime():
    """ONE HIP runtime per process, whatever the import order.  libcannoles_hip.so needs `libamdhip64.so.7`.  A PyTorch wheel
    bundles its own copy (same SONAME, found through torch's rpath under the name `libamdhip64.so`):
      * torch imported first: the loader satisfies our dependency with torch's copy (SONAME match) — one runtime;
      * our library first, torch later: ours would pull in the system ROCm's runtime, torch then its bundled copy — two runtimes,
        and the one that initialises second finds no device.
    So when this process has no HIP runtime yet and a torch wheel with a bundled runtime is INSTALLED (not imported here), that
    copy is loaded first: our library binds to it and a later `import torch` finds it already loaded.  Without torch (the Julia
    drop-in, a C caller) the system runtime is used as linked."""
    if loaded_hip_runtimes():
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass   # fall back to the runtime the library is linked against


def lib():
    """Load libcannoles_hip.so (built by __graft_entry__.build / csrc/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)")
        _one_hip_runtime()
        L = C.CDLL(LIB_PATH)
        vp, i64, dbl, i32 = C.c_void_p, C.c_int64, C.c_double, C.c_int32
        L.cnl_last_error.restype = C.c_char_p
        L.cnl_version.restype = i32
        L.cnl_default_params.argtypes = [vp]
        L.cnl_plan_create.argtypes = [C.POINTER(vp), i64, i64, _i64p, _i64p, i64, i64, i64]
        L.cnl_plan_create_for_batch.argtypes = [C.POINTER(vp), i64, i64, _i64p, _i64p, i64, i64, i64, i64]
        L.cnl_options_init.argtypes = [vp]
        L.cnl_options_init.restype = None
        L.cnl_plan_create_ex.argtypes = [C.POINTER(vp), i64, i64, _i64p, _i64p, i64, i64, i64, i64, vp]
        L.cnl_create_ex.argtypes = [C.POINTER(vp), i64, i64, _i64p, _i64p, i64, i64, i64, i64, C.c_int, vp]
        L.cnl_dataflow_timeouts.argtypes = [vp, C.POINTER(i64)]
        L.cnl_plan_destroy.argtypes = [vp]
        L.cnl_plan_destroy.restype = None
        L.cnl_plan_info.argtypes = [vp, _i64p]
        L.cnl_plan_get.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64)]
        L.cnl_plan_order_name.argtypes = [vp]
        L.cnl_plan_order_name.restype = C.c_char_p
        L.cnl_create.argtypes = [C.POINTER(vp), i64, i64, _i64p, _i64p, i64, i64, i64, i64, C.c_int]
        L.cnl_destroy.argtypes = [vp]
        L.cnl_get_plan.argtypes = [vp]
        L.cnl_get_plan.restype = vp
        L.cnl_factorize.argtypes = [vp, vp, dbl, vp, vp, vp]
        L.cnl_solve.argtypes = [vp, vp, vp]
        L.cnl_newton_system.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnl_factorize_dev.argtypes = [vp, vp, dbl, vp, vp]
        L.cnl_solve_dev.argtypes = [vp, vp, vp, vp]
        L.cnl_newton_system_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnl_residual_vectors_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnl_trial_point_dev.argtypes = [vp, vp, vp, vp, vp, dbl, vp, vp, vp, vp, vp]
        L.cnl_kkt_residual_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.cnl_get_refine_norms.argtypes = [vp, vp, C.POINTER(i64)]
        L.cnl_prepare_newton_system_dev.argtypes = [vp, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp]
        L.cnl_cgls_multipliers_dev.argtypes = [vp, vp, vp, vp, vp, dbl, dbl, i64, C.c_int, vp, vp]
        L.cnl_multi_create.argtypes = [C.POINTER(vp), i64, i64, _i64p, _i64p, i64, i64, i64, i64, vp, C.c_int]
        L.cnl_multi_create_ex.argtypes = [C.POINTER(vp), i64, i64, _i64p, _i64p, i64, i64, i64, i64, vp, C.c_int, vp]
        L.cnl_multi_factorize_dev.argtypes = [vp, vp, dbl, vp, vp]
        L.cnl_multi_solve_dev.argtypes = [vp, vp, vp, vp]
        L.cnl_multi_newton_system_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnl_multi_synchronize.argtypes = [vp, vp]
        L.cnl_multi_destroy.argtypes = [vp]
        L.cnl_multi_shards.argtypes = [vp, C.POINTER(i64), vp, vp, vp]
        L.cnl_multi_factorize.argtypes = [vp, vp, dbl, vp, vp, vp]
        L.cnl_multi_solve.argtypes = [vp, vp, vp]
        L.cnl_multi_newton_system.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnl_set_timing.argtypes = [vp, C.c_int]
        L.cnl_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.cnl_get_config.argtypes = [vp, _i64p]
        L.cnl_launch_counts.argtypes = [_i64p]
        L.cnl_layout_len.argtypes = [vp, C.c_int, C.POINTER(i64)]
        L.cnl_residual_vectors_jac_dev.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnl_cgls_multipliers_jac_dev.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, dbl, dbl, i64, C.c_int, vp, vp]
        L.cnl_interleave_dev.argtypes = [vp, C.c_int, vp, vp, vp]
        L.cnl_deinterleave_dev.argtypes = [vp, C.c_int, vp, vp, vp]
        flt = C.c_float
        L.cnl_default_params_f32.argtypes = [vp]
        L.cnl_default_params_f32.restype = None
        L.cnl_create_f32.argtypes = [C.POINTER(vp), i64, i64, _i64p, _i64p, i64, i64, i64, i64, C.c_int]
        L.cnl_create_f32_ex.argtypes = [C.POINTER(vp), i64, i64, _i64p, _i64p, i64, i64, i64, i64, C.c_int, vp]
        L.cnl_factorize_f32.argtypes = [vp, vp, flt, vp, vp, vp]
        L.cnl_solve_f32.argtypes = [vp, vp, vp]
        L.cnl_newton_system_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnl_factorize_f32_dev.argtypes = [vp, vp, flt, vp, vp]
        L.cnl_solve_f32_dev.argtypes = [vp, vp, vp, vp]
        L.cnl_newton_system_f32_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnl_interleave_f32_dev.argtypes = [vp, C.c_int, vp, vp, vp]
        L.cnl_deinterleave_f32_dev.argtypes = [vp, C.c_int, vp, vp, vp]
        L.cnl_prepare_newton_system_f32_dev.argtypes = [vp, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp]
        L.cnl_residual_vectors_f32_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnl_residual_vectors_jac_f32_dev.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnl_cgls_multipliers_f32_dev.argtypes = [vp, vp, vp, vp, vp, flt, flt, i64, C.c_int, vp, vp]
        L.cnl_cgls_multipliers_jac_f32_dev.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, flt, flt, i64, C.c_int, vp, vp]
        L.cnl_trial_point_f32_dev.argtypes = [vp, vp, vp, vp, vp, flt, vp, vp, vp, vp, vp]
        for fn in ("cnl_outer_begin_dev", "cnl_outer_extrapolated_dev", "cnl_outer_trial_done_dev", "cnl_outer_end_dev", "cnl_outer_ls_begin_dev",
                   "cnl_outer_ls_step_dev", "cnl_outer_ls_take_dev"):
            getattr(L, fn).argtypes = [vp, vp]
            getattr(L, fn.replace("_dev", "_f32_dev")).argtypes = [vp, vp]
        for sfx in ("_dev", "_f32_dev"):
            getattr(L, "cnl_outer_newton_done" + sfx).argtypes = [vp, C.c_int, vp]
            getattr(L, "cnl_outer_ls_test" + sfx).argtypes = [vp, C.c_int, vp]
            for k in ("begin_ex", "trial_done_ex", "end_ex", "hess_mask"):
                getattr(L, "cnl_outer_" + k + sfx).argtypes = [vp, vp, vp]
            getattr(L, "cnl_outer_ls_test_ex" + sfx).argtypes = [vp, C.c_int, vp, vp]
        L.cnl_set_active_batch.argtypes = [vp, i64]
        L.cnl_get_active_batch.argtypes = [vp, C.POINTER(i64)]
        L.cnl_subtree_stage_shape.argtypes = [vp, vp, vp, C.POINTER(i64)]
        for fn in ("cnl_outer_compact_dev", "cnl_outer_compact_f32_dev"):
            getattr(L, fn).argtypes = [vp, i64, vp, vp, i64, vp, vp, vp, vp]
        if L.cnl_version() < 200:
            raise RuntimeError(f"{LIB_PATH}: cnl_version() = {L.cnl_version()}, ABI version 0.2.0 or later required")
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise CnlError(rc, lib().cnl_last_error().decode())


def default_params(dtype=np.float64):
    """ParamCaNNOLeS(T) (src/CaNNOLeS.jl:48-62) as [eig_tol, dmin, kdec, kinc, klargeinc, rho0, rhomax, rhomin, gammaA];
    T = Float64 (cnl_default_params) or Float32 (cnl_default_params_f32)."""
    dt = np.dtype(dtype)
    if dt == np.float32:
        p = np.zeros(9, np.float32)
        lib().cnl_default_params_f32(p.ctypes.data)
        return p
    if dt != np.float64:
        raise TypeError(f"ParamCaNNOLeS({dt}): this backend serves Float64 and Float32 only")
    p = np.zeros(9)
    lib().cnl_default_params(p.ctypes.data)
    return p


def _i64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64).ravel())


_INFO_KEYS = ["N", "nnz", "nnzK", "nsuper", "nnzL", "nnzL_exact", "lsize", "fmax", "fwd_peak", "bwd_peak",
              "panel_max", "flops", "nasm", "v2_classes", "v2_lds", "ncond"]


def _plan_info(p):
    info = np.zeros(16, np.int64)
    _check(lib().cnl_plan_info(p, info))
    d = {k: int(info[i]) for i, k in enumerate(_INFO_KEYS)}
    d["order"] = lib().cnl_plan_order_name(p).decode()
    c, l = d.pop("v2_classes"), d.pop("v2_lds")
    if c >= 0:
        d["v2"] = {"fronts16": c & 0xfffff, "fronts32": (c >> 20) & 0xfffff, "fronts64": c >> 40,
                   "ustack": l & 0xfffff, "staging": (l >> 20) & 0xfffff, "reclen": l >> 40}
    else:
        d["v2"] = None
    return d


def _plan_array(p, name):
    n = C.c_int64(0)
    _check(lib().cnl_plan_get(p, name.encode(), None, C.byref(n)))
    out = np.zeros(max(n.value, 1), np.int32)
    cnt = C.c_int64(out.size)
    _check(lib().cnl_plan_get(p, name.encode(), out.ctypes.data, C.byref(cnt)))
    return out[:n.value]


class Plan:
    """Host-only symbolic analysis (what `ldl_analyze` is to the reference).
    Needs no GPU; used by the CPU test-suite and for sizing."""

    def __init__(self, N, rows, cols, nvar, nequ, ncon, batch=None, options=None):
        self.rows, self.cols = _i64(rows), _i64(cols)
        p = C.c_void_p()
        if options is not None:   # explicit options (batch None: the large-batch analysis unless the options say otherwise)
            _check(lib().cnl_plan_create_ex(C.byref(p), int(N), len(self.rows), self.rows, self.cols, int(nvar), int(nequ), int(ncon),
                                            int(batch or 0), _optref(options)))
        elif batch is None:  # the large-batch analysis
            _check(lib().cnl_plan_create(C.byref(p), int(N), len(self.rows), self.rows, self.cols, int(nvar), int(nequ), int(ncon)))
        else:              # what cnl_create(batch) runs
            _check(lib().cnl_plan_create_for_batch(C.byref(p), int(N), len(self.rows), self.rows, self.cols, int(nvar), int(nequ),
                                                   int(ncon), int(batch)))
        self._p = p
        self.info = _plan_info(p)

    def array(self, name):
        return _plan_array(self._p, name)

    def __del__(self):
        if getattr(self, "_p", None):
            lib().cnl_plan_destroy(self._p)
            self._p = None


class _Factor:
    """What `LDLT.factor` is to the reference: the object `solve_ldl!` dispatches on."""

    def __init__(self, owner):
        self._owner = owner


class HIPLDLStruct:
    """`struct HIPLDLStruct <: LinearSolverStruct` — drop-in for LDLFactStruct
    (src/solver_types.jl:45-65).  `batch > 1` is the batched twin: one shared
    pattern, problem-major values `vals[b, :]`.

    The element type comes from `vals`, as `LDLFactStruct(N, rows, cols, vals)` takes T from it (`dtype` when vals is None):
    float64, or float32 — a Float32 handle (cnl_create_f32), which by default exists for band-structured patterns only (CnlError
    CNL_ERR_ARG otherwise: the caller stays on the CPU backend); Options(float32_general=1) serves every other pattern on the
    general multifrontal kernel in float (config["kernel"] == "v1"), and Options(float32_general=1, float32_condense=1) runs that
    kernel on the condensed system — the -I block eliminated by the condensation passes in float — which info["ncond"] > 0 identifies
    (config["cond_resident"]: the resident condense kernel serves it).  Options(float32_general=1, float32_register_front=1) implies
    float32_condense and runs newton_system! / try_to_factorize on the register-front kernel in float between those passes
    (config["kernel"] == "v2", config["wpb"] / config["lds2_bytes"] its wavefronts per workgroup and LDS bytes; solve_ldl! runs on the
    general kernel, on the same panels); where a front exceeds order 64 the handle is the float32_condense handle ("v1").  Adding
    float32_direct_records=1 puts that handle on the Direct route of the Float64 default handle (config["direct"]): the float
    register-front kernel condenses on the fly, a call is that launch and the post-pass, and solve_ldl! stays on the same kernel where
    every front is of the fast class (config["v2_solve"]); patterns whose direct records the analysis refuses keep the handle without
    the key.  Options(float32_general=1, float32_dense=1) puts a pattern whose residual block is DENSE (every residual row holds one
    entry per variable plus its diagonal: what the Float64 dense backend takes) on the dense backend in float, at any batch size
    (config["kernel"] == "dense" and config["float32"]: J'WJ and the trailing updates on the f32 matrix cores, the rho ladder decided
    on the device); every other pattern, and every pattern with dense_backend=0, gets the handle it gets without the key;
    float32_dense=1 without float32_general is CNL_ERR_ARG.  Options(float32_general=1, float32_general_dense=1) (implies
    float32_condense) puts an IRREGULAR pattern whose condensed plan has a front above order 64, condensed order 96 .. 4096, on the
    general form of that backend: the float condensation passes around one dense LDL' of the whole condensed system
    (config["kernel"] == "dense", config["float32"] and info["ncond"] > 0), while batch <= 16 or the tiles stay within 8 GB; 2:
    whatever the fronts; every other pattern gets the handle it gets without the key, and the key without float32_general is
    CNL_ERR_ARG.  Options(float32_general=1, float32_staged=1) (implies float32_register_front, float32_direct_records and
    float32_condense; band patterns need band_kernel=0 to get past the band kernels) plans a batch for latency where a Float64 handle
    would be (plan_kind, 1 <= batch <= staged_max_batch) and runs that plan stage by stage on the staged float instances of the
    register-front kernel, one launch per stage (config["kernel"] == "v2-staged", config["float32"], config["direct"]); the problems
    that fail the first attempt climb the rho ladder in one classic launch behind the stages; solve_ldl! runs staged too where
    config["v2_solve"].  Such a handle refuses set_active_batch (CnlError code 5).  Every other batch or pattern gets the handle it
    gets with float32_register_front=1, float32_direct_records=1 in place of the key; the key without float32_general, with a value
    other than 0 / 1 or with float32_refine is CNL_ERR_ARG.  Options(float32_general=1, float32_latency=1) (implies float32_staged)
    is that handle with the switches a Float64 latency handle honours — lean_kernel, rows_in_backward, dataflow, dataflow_waves,
    dataflow_spin_limit, device_ladder, device_ladder_fused, Float64 defaults and rules — on the lean, dataflow and fused-ladder
    float instances: config["lean"], config["dataflow"] and config["lad_mode"] say which run; the same fallbacks and refusals.
    A condensed or direct
    handle of either kind reads the Jacobian values of `vals` again in solve_ldl!: the array given to try_to_factorize must stay alive
    and unmodified until the last solve on that factor.

    Mixed precision: HIPLDLStruct(..., dtype=float64, options=Options(float32_general=1, ..., float32_refine=k)), k = 1 .. 4, is a
    FLOAT64 handle (config["float32"] False, config["refine"] == k) on a Float32 factor: it owns the Float32 general handle the other
    float32_* keys select (band kernels never: they keep no factor), and config["kernel"], config["direct"] and info["ncond"]
    describe that inner handle.  A call factorises the demoted values in float — the rho ladder, nfact and success are the Float32
    handle's, with eig_tol raised to eps(Float32) at least — and corrects d k times with a Float64 residual rhs + K d
    (kkt_residual_dev is that kernel on its own) and a solve on the kept factor; refine_norms(LDLT) returns the residual norms in
    front of each correction, which do not fall where the system is too ill-conditioned for a Float32 factor.  solve_ldl! reads the
    `vals` of the last factorisation again: the rule above binds this handle too.  float32_refine without float32_general, k outside
    0 .. 4, the key on a float32 handle or a MultiHIPLDLStruct, and batch_layout=LAYOUT_INTERLEAVED are CNL_ERR_ARG."""

    def __init__(self, N, rows, cols, vals, nvar=None, nequ=None, ncon=None, batch=1, device=0, options=None, dtype=np.float64):
        self.N = int(N)
        self.rows, self.cols = _i64(rows), _i64(cols)
        self.nnz = len(self.rows)
        self.batch = int(batch)
        if nvar is None:
            raise ValueError("nvar/nequ/ncon are required (the Julia glue passes them from the solver)")
        self.nvar, self.nequ, self.ncon = int(nvar), int(nequ), int(ncon)
        self.dtype = np.dtype(np.asarray(vals).dtype if vals is not None else dtype)
        if self.dtype not in (np.float64, np.float32):
            raise TypeError(f"element type {self.dtype}: this backend serves Float64 and Float32 (band patterns) only; other element types "
                            "stay on LDLFactStruct")
        f32 = self.dtype == np.float32
        # `vals` is aliased, not copied: the driver mutates the array returned by get_vals
        self.vals = vals if vals is not None else np.ones((self.batch, self.nnz) if self.batch > 1 else self.nnz, self.dtype)
        h = C.c_void_p()
        if options is None:
            _check((lib().cnl_create_f32 if f32 else lib().cnl_create)(C.byref(h), self.N, self.nnz, self.rows, self.cols, self.nvar, self.nequ,
                                                                        self.ncon, self.batch, int(device)))
        else:
            _check((lib().cnl_create_f32_ex if f32 else lib().cnl_create_ex)(C.byref(h), self.N, self.nnz, self.rows, self.cols, self.nvar,
                                                                              self.nequ, self.ncon, self.batch, int(device), _optref(options)))
        self._h = h
        self.factor = _Factor(self)
        self.info = _plan_info(lib().cnl_get_plan(h))
        cfg = np.zeros(8, np.int64)
        _check(lib().cnl_get_config(h, cfg))
        self.config = {"tpp": int(cfg[0]), "ppb": int(cfg[1]), "lds_bytes": int(cfg[2]), "lds_work": int(cfg[3]), "grid": int(cfg[4]),
                       "kernel": {2: "v2", 3: "dense", 4: "v2-staged"}.get(int(cfg[5]) & 15, "v1"), "wpb": int(cfg[6]), "lds2_bytes": int(cfg[7]),
                       "lean": bool(int(cfg[5]) & 16), "tail": bool(int(cfg[5]) & 32), "band": bool(int(cfg[5]) & 64), "f1_tiles": bool(int(cfg[5]) & 128),
                       "band_nl": (int(cfg[5]) >> 8) & 255, "band_parts": (int(cfg[5]) >> 16) & 3, "band_cache_policy": (int(cfg[5]) >> 18) & 31,"band_resident": bool((int(cfg[5]) >> 24) & 1),
                       "band_mover_table": bool((int(cfg[5]) >> 34) & 1), "cond_resident": bool((int(cfg[5]) >> 35) & 1),
                       "batch_layout": (int(cfg[5]) >> 25) & 1, "rhs_interleaved": bool((int(cfg[5]) >> 26) & 1),
                       "float32": bool((int(cfg[5]) >> 27) & 1), "band_pieces": (int(cfg[5]) >> 28) & 63,
                       "direct": bool((int(cfg[5]) >> 36) & 1), "v2_solve": bool((int(cfg[5]) >> 37) & 1),
                       "refine": (int(cfg[5]) >> 39) & 7 if (int(cfg[5]) >> 38) & 1 else 0,
                       # staged handles: dataflow counters present; the in-kernel ladder (0 none, 1, 2 fused)
                       "dataflow": bool((int(cfg[5]) >> 42) & 1), "lad_mode": (int(cfg[5]) >> 43) & 3,
                       "cgls_wide": (int(cfg[5]) >> 45) & 3,
                       # newton_system / factorize run a blocked instance of the general kernel (Options(general_blocked=1))
                       "general_blocked": bool((int(cfg[5]) >> 47) & 1),
                       # ... of the general kernel in float, on a Float32 general handle (Options(float32_blocked=1))
                       "float32_blocked": bool((int(cfg[5]) >> 48) & 1),
                       # the three calls run the general kernel's subtree instances stage by stage (Options(general_subtrees=1), where
                       # it acts: plan_array("gtasks") / ("gstage_ptr") / ("gfronts") / ("ginfo") describe the cut and its work area)
                       "general_subtrees": bool((int(cfg[5]) >> 49) & 1),
                       # ... in float, on a Float32 general handle (Options(float32_subtrees=1), where it acts)
                       "float32_subtrees": bool((int(cfg[5]) >> 50) & 1),
                       # ... with this many rungs of the rho ladder enqueued behind the first attempt of newton_system
                       # (Options(subtree_ladder=R), where the subtree key acts; 0 everywhere else)
                       "subtree_ladder": (int(cfg[5]) >> 51) & 127,
                       # at least one stage factorises with 1024 threads per workgroup at the created batch (Options(subtree_wide=W))
                       "subtree_wide": bool((int(cfg[5]) >> 58) & 1),
                       # at least one stage eliminates its dependent pivot panels in LDS (Options(subtree_lds_panels=M))
                       "subtree_lds_panels": bool((int(cfg[5]) >> 59) & 1),
                       # the solve sweeps that run in panels of 16 pivots (Options(subtree_solve_panels=P)): bit 0 backward stages, bit 1 forward stages of solve
                       "subtree_solve_panels": (int(cfg[5]) >> 60) & 3}
        if self.config["float32"] and self.config["band"]:   # (a Float32 handle off the band kernels — tuning float32_general — is "v1")
            self.config["kernel"] = "band"

    def plan_array(self, name):
        return _plan_array(lib().cnl_get_plan(self._h), name)

    def close(self):
        if getattr(self, "_h", None):
            lib().cnl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_timing(self, on=True):
        _check(lib().cnl_set_timing(self._h, 1 if on else 0))

    def uses_lean_kernel(self):
        """True when newton_system / factorize of this handle run the kernels' LEAN instantiation (cnl_get_config, cfg[5] bit 4)"""
        cfg = np.zeros(8, np.int64)
        _check(lib().cnl_get_config(self._h, cfg))
        return bool(int(cfg[5]) & 16)

    def dataflow_timeouts(self):
        n = C.c_int64(0)
        _check(lib().cnl_dataflow_timeouts(self._h, C.byref(n)))
        return int(n.value)

    def last_kernel_ms(self):
        ms = C.c_float(0)
        _check(lib().cnl_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)


def set_active_batch(LDLT, nb):
    """cnl_set_active_batch: the handle's device-pointer entry points work on its first nb problems from here on (arrays keep the
    addressing of the created batch).  Raises CnlError — code 5 (CNL_ERR_STATE) on a handle that cannot (staged, split, dense)."""
    _check(lib().cnl_set_active_batch(LDLT._h, int(nb)))


def subtree_stage_shape(LDLT):
    """cnl_subtree_stage_shape: (tpp, lds_bytes), two int32 arrays with one entry per stage of a subtree handle — threads per workgroup
    and dynamic LDS bytes of the stage's factorising forward launch at the handle's current active batch (Options(subtree_wide=W,
    subtree_lds_panels=M)).  Raises CnlError (CNL_ERR_ARG) on a handle that is no subtree handle."""
    n = C.c_int64(0)
    _check(lib().cnl_subtree_stage_shape(LDLT._h, None, None, C.byref(n)))
    tpp, lds = np.zeros(int(n.value), np.int32), np.zeros(int(n.value), np.int32)
    _check(lib().cnl_subtree_stage_shape(LDLT._h, tpp.ctypes.data, lds.ctypes.data, C.byref(n)))
    return tpp, lds


def get_active_batch(LDLT):
    n = C.c_int64(0)
    _check(lib().cnl_get_active_batch(LDLT._h, C.byref(n)))
    return int(n.value)


def outer_compact_dev(state, extras, min_finished, orig_ptr, counts_ptr, work_ptr, stream=0):
    """cnl_outer_compact_dev / cnl_outer_compact_f32_dev (by the type of `state`, a cnl_outer_state or cnl_outer_state_f32): the
    active problems become the first rows of every per-problem array of the state, of the `extras` — (device address, row bytes)
    pairs — and of orig [B] int32; counts [2] int32 receives (active rows, rows the caller goes on with); work: int32 [B + 2]."""
    fn = lib().cnl_outer_compact_f32_dev if isinstance(state, cnl_outer_state_f32) else lib().cnl_outer_compact_dev
    k = len(extras)
    ptrs = (C.c_void_p * max(k, 1))(*[int(p) for p, _ in extras])
    rows = (C.c_int64 * max(k, 1))(*[int(b) for _, b in extras])
    _check(fn(C.byref(state), k, ptrs, rows, int(min_finished), _int_ptr(orig_ptr), _int_ptr(counts_ptr), _int_ptr(work_ptr), stream))


def launch_counts():
    """launches per kernel family since the library was loaded: {"band", "register_front", "general"} (cnl_launch_counts)"""
    c = np.zeros(3, np.int64)
    _check(lib().cnl_launch_counts(c))
    return {"band": int(c[0]), "register_front": int(c[1]), "general": int(c[2])}


def get_vals(LDLT):
    """get_vals(LDLT::LinearSolverStruct) = LDLT.vals (src/solver_types.jl:67)."""
    return LDLT.vals


def _f64c(a, shape=None):
    a = np.asarray(a)
    if a.dtype != np.float64 or not a.flags.c_contiguous:
        raise TypeError("expected a C-contiguous float64 array (Float64 only; other element types stay on LDLFactStruct)")
    return a


def _is_f32(LDLT):
    return getattr(LDLT, "dtype", np.float64) == np.float32


def _valsc(LDLT, a):
    """a C-contiguous array of the handle's element type (float64, or float32 on a Float32 handle); mixing types is a TypeError"""
    if not _is_f32(LDLT):
        return _f64c(a)
    a = np.asarray(a)
    if a.dtype != np.float32 or not a.flags.c_contiguous:
        raise TypeError(f"expected a C-contiguous float32 array on a Float32 handle, got {a.dtype}")
    return a


def _dev_ptr(LDLT, x):
    """device address of a `_dev` argument: an int, or a tensor (torch) whose element type must be the handle's"""
    if hasattr(x, "data_ptr"):
        want = "float32" if _is_f32(LDLT) else "float64"
        if str(x.dtype).rsplit(".", 1)[-1] != want:
            raise TypeError(f"expected a {want} tensor on this handle, got {x.dtype}")
        return x.data_ptr()
    return x


def _int_ptr(x):
    return x.data_ptr() if hasattr(x, "data_ptr") else x


def try_to_factorize(LDLT, vals, nvar, nequ, ncon, eig_tol, return_inertia=False):
    """success = try_to_factorize(LDLT, vals, nvar, nequ, ncon, eig_tol) (src/solver_types.jl:79-98).
    Batched handles return arrays."""
    assert (nvar, nequ, ncon) == (LDLT.nvar, LDLT.nequ, LDLT.ncon)
    vals = _valsc(LDLT, vals)
    assert vals.size == LDLT.batch * LDLT.nnz
    B = LDLT.batch
    succ = np.zeros(B, np.int32)
    npos = np.zeros(B, np.int64)
    nzer = np.zeros(B, np.int64)
    fn = lib().cnl_factorize_f32 if _is_f32(LDLT) else lib().cnl_factorize
    _check(fn(LDLT._h, vals.ctypes.data, float(eig_tol), succ.ctypes.data, npos.ctypes.data, nzer.ctypes.data))
    if B == 1:
        return (bool(succ[0]), int(npos[0]), int(nzer[0])) if return_inertia else bool(succ[0])
    return (succ.astype(bool), npos, nzer) if return_inertia else succ.astype(bool)


def solve_ldl_(rhs, factor, d):
    """solve_ldl!(rhs, factor, d): d = -(K^-1 rhs), returns true (src/solver_types.jl:69-77)."""
    LDLT = factor._owner
    rhs = _valsc(LDLT, rhs)
    d = _valsc(LDLT, d)
    assert rhs.size == LDLT.batch * LDLT.N and d.size == rhs.size
    _check((lib().cnl_solve_f32 if _is_f32(LDLT) else lib().cnl_solve)(LDLT._h, rhs.ctypes.data, d.ctypes.data))
    return True


def newton_system_(d, nvar, nequ, ncon, rhs, vals, LDLT, rho_old, params):
    """d, solve_success, rho, rho_old, nfact = newton_system!(d, nvar, nequ, ncon, rhs, vals, LDLT, rho_old, params)
    (src/CaNNOLeS.jl:1008-1052), fused on the device.  `vals` is mutated (rho slots).
    Batched handles take/return arrays for rho_old / success / rho / nfact."""
    assert (nvar, nequ, ncon) == (LDLT.nvar, LDLT.nequ, LDLT.ncon)
    B = LDLT.batch
    vals = _valsc(LDLT, vals)
    rhs = _valsc(LDLT, rhs)
    d = _valsc(LDLT, d)
    assert vals.size == B * LDLT.nnz and rhs.size == B * LDLT.N and d.size == B * LDLT.N
    T = np.float32 if _is_f32(LDLT) else np.float64
    ro = np.ascontiguousarray(np.broadcast_to(np.asarray(rho_old, dtype=T), (B,)))
    params = np.ascontiguousarray(params, dtype=T)
    rho = np.zeros(B, T)
    ro_out = np.zeros(B, T)
    nfact = np.zeros(B, np.int32)
    succ = np.zeros(B, np.int32)
    _check((lib().cnl_newton_system_f32 if T == np.float32 else lib().cnl_newton_system)(LDLT._h, vals.ctypes.data, rhs.ctypes.data, d.ctypes.data, ro.ctypes.data,
                                   params.ctypes.data, rho.ctypes.data, ro_out.ctypes.data, nfact.ctypes.data,
                                   succ.ctypes.data))
    if B == 1:
        return d, bool(succ[0]), float(rho[0]), float(ro_out[0]), int(nfact[0])
    return d, succ.astype(bool), rho, ro_out, nfact.astype(np.int64)


def newton_system_dev(LDLT, vals_ptr, rhs_ptr, d_ptr, rho_old_ptr, rho_ptr, nfact_ptr, success_ptr, params, stream=0):
    """Device-resident twin (cnl_newton_system_dev): all *_ptr are device addresses
    (e.g. torch.Tensor.data_ptr(), or the tensors themselves: their element type is checked against the handle's);
    asynchronous on `stream` (a hipStream_t value).  Float32 handles: cnl_newton_system_f32_dev, float32 arrays and params."""
    f32 = _is_f32(LDLT)
    params = np.ascontiguousarray(params, dtype=np.float32 if f32 else np.float64)
    v, r, dd, ro, rh = (_dev_ptr(LDLT, x) for x in (vals_ptr, rhs_ptr, d_ptr, rho_old_ptr, rho_ptr))
    _check((lib().cnl_newton_system_f32_dev if f32 else lib().cnl_newton_system_dev)(LDLT._h, v, r, dd, ro, rh, _int_ptr(nfact_ptr),
                                                                                    _int_ptr(success_ptr), params.ctypes.data, stream))


def factorize_dev(LDLT, vals_ptr, eig_tol, success_ptr, stream=0):
    """try_to_factorize on device-resident vals (cnl_factorize_dev / cnl_factorize_f32_dev by the handle's element type)"""
    fn = lib().cnl_factorize_f32_dev if _is_f32(LDLT) else lib().cnl_factorize_dev
    _check(fn(LDLT._h, _dev_ptr(LDLT, vals_ptr), float(eig_tol), _int_ptr(success_ptr), stream))


def solve_dev(LDLT, rhs_ptr, d_ptr, stream=0):
    """solve_ldl! on device-resident rhs / d (cnl_solve_dev / cnl_solve_f32_dev by the handle's element type)"""
    fn = lib().cnl_solve_f32_dev if _is_f32(LDLT) else lib().cnl_solve_dev
    _check(fn(LDLT._h, _dev_ptr(LDLT, rhs_ptr), _dev_ptr(LDLT, d_ptr), stream))


def residual_vectors_dev(LDLT, vals_ptr, r_ptr, lambda_ptr, Fx_ptr, cx_ptr, rhs_ptr, norms_ptr, stream=0):
    """rhs = [dual; primal] with dual = Jx' r - Jc' lambda, primal = [F - r; c], and their infinity norms
    (src/CaNNOLeS.jl:507-508,519-524,528-529,631-632), batched and device-resident (cnl_residual_vectors_dev, or
    cnl_residual_vectors_f32_dev on a Float32 handle).  All *_ptr are device addresses (or tensors of the handle's element type);
    norms_ptr receives [batch][2] values."""
    fn = lib().cnl_residual_vectors_f32_dev if _is_f32(LDLT) else lib().cnl_residual_vectors_dev
    _check(fn(LDLT._h, *(_dev_ptr(LDLT, x) for x in (vals_ptr, r_ptr, lambda_ptr, Fx_ptr, cx_ptr, rhs_ptr, norms_ptr)), stream))


def kkt_residual_dev(LDLT, vals_ptr, rhs_ptr, d_ptr, g_ptr, norms_ptr, stream=0):
    """g = rhs + K(vals) d and norms = max |g| per problem, in Float64 on device-resident arrays (cnl_kkt_residual_dev): the residual
    of the Newton system, K the full symmetric matrix of the pattern with the rho slots as they stand in vals.  Float64 handles with
    problem-major vals; norms_ptr may be None.  Deterministic: two calls give the same bits."""
    v, r, d, g = (_dev_ptr(LDLT, x) for x in (vals_ptr, rhs_ptr, d_ptr, g_ptr))
    _check(lib().cnl_kkt_residual_dev(LDLT._h, v, r, d, g, None if norms_ptr is None else _dev_ptr(LDLT, norms_ptr), stream))


def refine_norms(LDLT):
    """[batch][k] residual norms max |rhs + K d_j| in front of correction j of the handle's last newton_system! / solve_ldl! call
    (cnl_get_refine_norms; d_0 is the raw Float32 solution, -1 marks a problem without a factor).  Synchronises the device.
    CnlError code 5 on a handle made without float32_refine."""
    k = max(1, int(LDLT.config.get("refine", 0)))
    out = np.full((LDLT.batch, k), np.nan)
    steps = C.c_int64(0)
    _check(lib().cnl_get_refine_norms(LDLT._h, out.ctypes.data, C.byref(steps)))
    return out[:, :int(steps.value)]


def residual_vectors_jac_dev(LDLT, nnzjF, nnzjc, Jx_ptr, Jcx_ptr, r_ptr, lambda_ptr, Fx_ptr, cx_ptr, rhs_ptr, norms_ptr, stream=0):
    """residual_vectors_dev with the Jacobian values read from the model's arrays Jx [batch][nnzjF], Jcx [batch][nnzjc] instead of
    from the J segments of vals (cnl_residual_vectors_jac_dev / cnl_residual_vectors_jac_f32_dev): no prepare pass in front, any
    batch_layout"""
    fn = lib().cnl_residual_vectors_jac_f32_dev if _is_f32(LDLT) else lib().cnl_residual_vectors_jac_dev
    _check(fn(LDLT._h, int(nnzjF), int(nnzjc), *(_dev_ptr(LDLT, x) for x in (Jx_ptr, Jcx_ptr, r_ptr, lambda_ptr, Fx_ptr, cx_ptr, rhs_ptr,
                                                                               norms_ptr)), stream))


def trial_point_dev(LDLT, x_ptr, r_ptr, lambda_ptr, d_ptr, max_dlambda, xt_ptr, rt_ptr, lambdat_ptr, dlambda_ptr, stream=0):
    """xt = x + dx, rt = r + dr, dlambda = -d[n+m+1:N] capped at max_dlambda in the 2-norm, lambdat = lambda + dlambda
    (src/CaNNOLeS.jl:654,661-668), batched and device-resident (cnl_trial_point_dev / cnl_trial_point_f32_dev)."""
    fn = lib().cnl_trial_point_f32_dev if _is_f32(LDLT) else lib().cnl_trial_point_dev
    x, r, lam, d, xt, rt, lt, dl = (_dev_ptr(LDLT, a) for a in (x_ptr, r_ptr, lambda_ptr, d_ptr, xt_ptr, rt_ptr, lambdat_ptr, dlambda_ptr))
    _check(fn(LDLT._h, x, r, lam, d, float(max_dlambda), xt, rt, lt, dl, stream))


def layout_len(LDLT, which):
    """elements of the interleaved array of the handle's batch; which = 0: vals, 1: an N-vector per problem (cnl_layout_len)"""
    n = C.c_int64(0)
    _check(lib().cnl_layout_len(LDLT._h, int(which), C.byref(n)))
    return int(n.value)


def interleave_dev(LDLT, which, src_ptr, dst_ptr, stream=0):
    """problem-major -> CNL_LAYOUT_INTERLEAVED on the device, out of place (cnl_interleave_dev / cnl_interleave_f32_dev)"""
    fn = lib().cnl_interleave_f32_dev if _is_f32(LDLT) else lib().cnl_interleave_dev
    _check(fn(LDLT._h, int(which), _dev_ptr(LDLT, src_ptr), _dev_ptr(LDLT, dst_ptr), stream))


def deinterleave_dev(LDLT, which, src_ptr, dst_ptr, stream=0):
    """CNL_LAYOUT_INTERLEAVED -> problem-major on the device, out of place (cnl_deinterleave_dev / cnl_deinterleave_f32_dev)"""
    fn = lib().cnl_deinterleave_f32_dev if _is_f32(LDLT) else lib().cnl_deinterleave_dev
    _check(fn(LDLT._h, int(which), _dev_ptr(LDLT, src_ptr), _dev_ptr(LDLT, dst_ptr), stream))


def prepare_newton_system_dev(LDLT, nnzhF, nnzhc, nnzjF, nnzjc, hF_ptr, hc_ptr, Jx_ptr, Jcx_ptr, delta_ptr, vals_ptr, stream=0):
    """prepare_newton_system! (src/CaNNOLeS.jl:947-981) for a batch on the device (cnl_prepare_newton_system_dev /
    cnl_prepare_newton_system_f32_dev): hF / -hc / Jx / Jcx / -delta / 0 into the segments of vals; hF_ptr = 0 leaves H_F alone
    (Gauss-Newton variants)."""
    fn = lib().cnl_prepare_newton_system_f32_dev if _is_f32(LDLT) else lib().cnl_prepare_newton_system_dev
    _check(fn(LDLT._h, int(nnzhF), int(nnzhc), int(nnzjF), int(nnzjc), *(_dev_ptr(LDLT, x) for x in (hF_ptr, hc_ptr, Jx_ptr, Jcx_ptr, delta_ptr,
                                                                                                    vals_ptr)), stream))


def _cgls_tols(LDLT, atol, rtol):
    """Krylov.jl's defaults sqrt(eps(T)) for the handle's element type T"""
    eps = float(np.finfo(np.float32 if _is_f32(LDLT) else np.float64).eps)
    return (np.sqrt(eps) if atol is None else atol), (np.sqrt(eps) if rtol is None else rtol)


def cgls_multipliers_dev(LDLT, vals_ptr, r_ptr, lambda_ptr, Jxtr_ptr=0, atol=None, rtol=None, itmax=0, ones_if_zero=True, iters_ptr=0,
                         stream=0):
    """Least-squares multipliers min ||Jc' lambda - Jx' r|| by CGLS (src/CaNNOLeS.jl:507-518), batched and device-resident
    (cnl_cgls_multipliers_dev / cnl_cgls_multipliers_f32_dev).  Default tolerances: sqrt(eps) of the handle's element type, as
    Krylov.jl's.  More than 1024 constraints: CnlError (CNL_ERR_DIM) unless the handle was created with Options(cgls_wide=1) (the
    instance with its ncon-vectors in the handle's workspace where ncon > 1024; 2: always; config["cgls_wide"]); bit-equal results."""
    atol, rtol = _cgls_tols(LDLT, atol, rtol)
    fn = lib().cnl_cgls_multipliers_f32_dev if _is_f32(LDLT) else lib().cnl_cgls_multipliers_dev
    v, r, lam, jx = (_dev_ptr(LDLT, x) for x in (vals_ptr, r_ptr, lambda_ptr, Jxtr_ptr))
    _check(fn(LDLT._h, v, r, lam, jx, float(atol), float(rtol), int(itmax), 1 if ones_if_zero else 0, _int_ptr(iters_ptr), stream))


def cgls_multipliers_jac_dev(LDLT, nnzjF, nnzjc, Jx_ptr, Jcx_ptr, r_ptr, lambda_ptr, Jxtr_ptr=0, atol=None, rtol=None, itmax=0,
                             ones_if_zero=True, iters_ptr=0, stream=0):
    """cgls_multipliers_dev with the Jacobian values read from the model's arrays (cnl_cgls_multipliers_jac_dev /
    cnl_cgls_multipliers_jac_f32_dev)"""
    atol, rtol = _cgls_tols(LDLT, atol, rtol)
    fn = lib().cnl_cgls_multipliers_jac_f32_dev if _is_f32(LDLT) else lib().cnl_cgls_multipliers_jac_dev
    jx, jc, r, lam, jt = (_dev_ptr(LDLT, x) for x in (Jx_ptr, Jcx_ptr, r_ptr, lambda_ptr, Jxtr_ptr))
    _check(fn(LDLT._h, int(nnzjF), int(nnzjc), jx, jc, r, lam, jt, float(atol), float(rtol), int(itmax), 1 if ones_if_zero else 0,
              _int_ptr(iters_ptr), stream))


class MultiHIPLDLStruct:
    """One solver object over several devices (cnl_multi_*): the batch is cut into contiguous balanced shards, one handle and
    one host thread per device, no collective.  Same call surface as a batched HIPLDLStruct for the host-pointer calls."""

    def __init__(self, N, rows, cols, nvar, nequ, ncon, batch, devices, options=None):
        self.N, self.nvar, self.nequ, self.ncon, self.batch = int(N), int(nvar), int(nequ), int(ncon), int(batch)
        self.rows, self.cols = _i64(rows), _i64(cols)
        self.nnz = len(self.rows)
        dv = np.ascontiguousarray(devices, dtype=np.int32)
        m = C.c_void_p()
        _check(lib().cnl_multi_create_ex(C.byref(m), self.N, self.nnz, self.rows, self.cols, self.nvar, self.nequ, self.ncon, self.batch,
                                         dv.ctypes.data, len(dv), _optref(options)))
        self._m = m
        n = C.c_int64(0)
        _check(lib().cnl_multi_shards(m, C.byref(n), None, None, None))
        st, ct, dd = np.zeros(n.value, np.int64), np.zeros(n.value, np.int64), np.zeros(n.value, np.int32)
        _check(lib().cnl_multi_shards(m, C.byref(n), st.ctypes.data, ct.ctypes.data, dd.ctypes.data))
        self.shards = [(int(a), int(b), int(c)) for a, b, c in zip(st, ct, dd)]  # (first problem, problems, device)

    def close(self):
        if getattr(self, "_m", None):
            lib().cnl_multi_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def try_to_factorize(self, vals, eig_tol):
        vals = _f64c(vals)
        succ = np.zeros(self.batch, np.int32)
        _check(lib().cnl_multi_factorize(self._m, vals.ctypes.data, float(eig_tol), succ.ctypes.data, None, None))
        return succ.astype(bool)

    def solve_ldl_(self, rhs, d):
        _check(lib().cnl_multi_solve(self._m, _f64c(rhs).ctypes.data, _f64c(d).ctypes.data))
        return True

    def newton_system_(self, d, rhs, vals, rho_old, params):
        B = self.batch
        vals, rhs, d = _f64c(vals), _f64c(rhs), _f64c(d)
        ro = np.ascontiguousarray(np.broadcast_to(np.asarray(rho_old, dtype=np.float64), (B,)))
        params = np.ascontiguousarray(params, dtype=np.float64)
        rho, ro_out = np.zeros(B), np.zeros(B)
        nfact, succ = np.zeros(B, np.int32), np.zeros(B, np.int32)
        _check(lib().cnl_multi_newton_system(self._m, vals.ctypes.data, rhs.ctypes.data, d.ctypes.data, ro.ctypes.data, params.ctypes.data,
                                             rho.ctypes.data, ro_out.ctypes.data, nfact.ctypes.data, succ.ctypes.data))
        return d, succ.astype(bool), rho, ro_out, nfact.astype(np.int64)

    # ---- device-resident twins: one list entry per shard (data_ptr of that shard's array on its device) ----
    @staticmethod
    def _ptrs(ptrs):
        return (C.c_void_p * len(ptrs))(*[int(p) for p in ptrs])

    def newton_system_dev(self, vals_ptrs, rhs_ptrs, d_ptrs, rho_old_ptrs, rho_ptrs, nfact_ptrs, success_ptrs, params, streams=None):
        params = np.ascontiguousarray(params, dtype=np.float64)
        st = self._ptrs(streams) if streams is not None else None
        _check(lib().cnl_multi_newton_system_dev(self._m, self._ptrs(vals_ptrs), self._ptrs(rhs_ptrs), self._ptrs(d_ptrs),
                                                 self._ptrs(rho_old_ptrs), self._ptrs(rho_ptrs), self._ptrs(nfact_ptrs),
                                                 self._ptrs(success_ptrs), params.ctypes.data, st))

    def factorize_dev(self, vals_ptrs, eig_tol, success_ptrs, streams=None):
        st = self._ptrs(streams) if streams is not None else None
        _check(lib().cnl_multi_factorize_dev(self._m, self._ptrs(vals_ptrs), float(eig_tol), self._ptrs(success_ptrs), st))

    def solve_dev(self, rhs_ptrs, d_ptrs, streams=None):
        st = self._ptrs(streams) if streams is not None else None
        _check(lib().cnl_multi_solve_dev(self._m, self._ptrs(rhs_ptrs), self._ptrs(d_ptrs), st))

    def synchronize(self, streams=None):
        st = self._ptrs(streams) if streams is not None else None
        _check(lib().cnl_multi_synchronize(self._m, st))
