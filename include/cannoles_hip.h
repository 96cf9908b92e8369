/*
 * cannoles_hip.h — C ABI of the MI355X-native Newton-system backend for CaNNOLeS.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Every entry point cites the reference interface it replaces
 * (paths under /root/reference).  The Julia binding a maintainer would add
 * is shown in INTEGRATION.md and shipped in cannoles.jl_amd/julia/.
 *
 * Conventions
 *   - Index arrays are int64, 1-based, exactly as Julia holds `rows`/`cols`
 *     (src/CaNNOLeS.jl:276-315).  Values are double (Float64).  Float32 is
 *     served by handles of its own, cnl_create_f32 and the `_f32` entry
 *     points below: on band-structured patterns by the band kernels
 *     (csrc/band.h), on any other pattern by the general multifrontal kernel
 *     where the caller asks for it (tuning "float32_general=1"; without it
 *     such a pattern is refused and stays on the reference's LDLFactStruct,
 *     as every other element type does).
 *   - The COO pattern is the lower triangle of the KKT matrix in the
 *     reference's 7-segment order [H_F | H_c | J_F | J_c | -I | -dI | rI];
 *     duplicates are summed in COO order (src/solver_types.jl:53-59); the
 *     LAST nvar entries are the rho slots (src/CaNNOLeS.jl:1027).
 *   - A handle serves a batch of `batch` independent problems that share the
 *     pattern (batch = 1 is the reference's one-solver-one-problem case).
 *     Batched arrays are problem-major: vals[b*nnz + k], rhs[b*N + i].
 *   - Host-pointer entry points copy in/out and keep no pointer afterwards.
 *   - cnl_solve / cnl_solve_dev use the LAST factorisation of the handle, whichever call made it (cnl_factorize or
 *     cnl_newton_system, with the rho it ended on).  The `_dev` twins keep the caller's d_vals pointer for that
 *     (sparse backends re-read the Jacobian entries during the solve): d_vals must stay alive and unmodified between a
 *     `_dev` factorisation and the `_dev` solves that use it.  The dense backend snapshots what it needs.
 *     `_dev` entry points take device pointers (HBM-resident data) and a
 *     hipStream_t passed as void*; they are asynchronous on that stream.
 *   - Return value: 0 = OK, otherwise one of CNL_ERR_*; cnl_last_error()
 *     describes the last failure on the calling thread.  Numerical failure
 *     (wrong inertia, zero pivot) is NOT an error: it is reported through
 *     `success`, like the reference's Bool (src/solver_types.jl:96-97).
 *   - There is no CPU fallback: without a usable HIP device every call that
 *     needs one fails with CNL_ERR_HIP.
 */
#ifndef CANNOLES_HIP_H
#define CANNOLES_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNL_OK 0
#define CNL_ERR_ARG 1      /* null pointer / bad handle / bad size              */
#define CNL_ERR_DIM 2      /* inconsistent or unsupported dimensions            */
#define CNL_ERR_PATTERN 3  /* malformed COO pattern (range, upper triangle)     */
#define CNL_ERR_HIP 4      /* HIP runtime error or no device                    */
#define CNL_ERR_STATE 5    /* call sequence error (solve before factorize)      */
#define CNL_ERR_INTERNAL 9

typedef struct cnl_plan cnl_plan;     /* host-only symbolic analysis            */
typedef struct cnl_handle cnl_handle; /* plan + device state for one batch      */

const char* cnl_last_error(void);
/* library / ABI version: major*10000 + minor*100 + patch (0.3.0: cnl_set_active_batch, cnl_outer_compact_dev;
 * 0.3.1: tuning "float32_general", no new symbol; 0.4.0: cnl_outer_ctl, the cnl_outer_*_ex_dev entry points, cnl_outer_hess_mask_dev;
 * 0.4.1: tuning "float32_register_front", no new symbol; 0.4.2: tuning "float32_direct_records", cnl_get_config bits 36 / 37, no new
 * symbol; 0.4.3: tuning "float32_dense", no new symbol; 0.4.4: tuning "float32_general_dense", no new symbol;
 * 0.5.0: tuning "float32_refine" / "refine_rows", cnl_kkt_residual_dev, cnl_get_refine_norms, cnl_plan_get "kkt_row_*",
 * cnl_get_config bits 38 .. 41; 0.5.1: tuning "float32_staged", no new symbol; 0.5.2: tuning "float32_latency", cnl_get_config
 * bits 42 .. 44, no new symbol; 0.5.3: tuning "cgls_wide", cnl_get_config bits 45 / 46, no new symbol;
 * 0.5.4: tuning "general_blocked", cnl_get_config bit 47, no new symbol; 0.5.5: tuning "float32_blocked", cnl_get_config bit 48,
 * no new symbol; 0.5.6: tuning "general_subtrees", cnl_get_config bit 49, cnl_plan_get "gtasks" / "gstage_ptr" / "gfronts" / "ginfo",
 * no new symbol; 0.5.7: tuning "float32_subtrees", cnl_get_config bit 50, no new symbol; 0.5.8: tuning "subtree_ladder", cnl_get_config
 * bits 51 .. 57, no new symbol; 0.5.9: tuning "subtree_wide" and "subtree_lds_panels", cnl_get_config bits 58 / 59,
 * cnl_subtree_stage_shape; 0.5.10 (510): tuning "subtree_solve_panels", cnl_get_config bits 60 / 61, no new symbol) */
int32_t cnl_version(void);

/* ParamCaNNOLeS(Float64) defaults, src/CaNNOLeS.jl:48-62, in the order
 * [eig_tol, delta_min, kappa_dec, kappa_inc, kappa_largeinc, rho0, rho_max, rho_min, gamma_A] */
void cnl_default_params(double params[9]);

/* ---- options ----------------------------------------------------------------------------------------------------------
 * Everything that selects a plan or an execution is an ARGUMENT: the library reads no environment variable that changes what it
 * computes (CNL_VERBOSE only adds log lines on stderr; the debugging aids CNL_DBG_LDSFILL / CNL_DBG_SCRATCHFILL — read once per process —
 * launch kernels that leave a byte pattern in LDS, scratch and registers in front of every launch, CNL_DBG_GUARD surrounds every device
 * allocation with filled guard zones — the library's results must not, and do not, depend on either).  cnl_options_init fills the
 * defaults — the choices cnl_create makes by itself; the `_ex` entry points take a modified copy.  A drop-in caller never needs it (the
 * reference has no counterpart: `ldl_analyze` takes no options, src/solver_types.jl:63).
 * The structure holds the switches that select a plan kind or allow / forbid a kernel family or an execution; everything finer
 * (orderings, thresholds, ablation switches of single kernels, measured-slower experiments) is reachable through `tuning`, a string of
 * "key=value" pairs whose keys are listed in cannoles.jl_amd/csrc/options.h — used by the measurement tools and the randomised
 * option fuzz of the test-suite; an unknown key is CNL_ERR_ARG.                                                                   */
#define CNL_PLAN_AUTO 0        /* by batch size: latency plan up to staged_max_batch problems, throughput plan above           */
#define CNL_PLAN_THROUGHPUT 1  /* least total work, one sequential record stream per four problems                             */
#define CNL_PLAN_LATENCY 2     /* bushy elimination tree cut into tasks (staged execution)                                      */
#define CNL_LAYOUT_PROBLEM_MAJOR 0   /* vals[b * nnz + k]: problem after problem, the reference's vector per problem               */
#define CNL_LAYOUT_INTERLEAVED 1     /* groups of 32 problems interleaved in blocks of eight doubles:
                                        vals[((b / 32 * (nnz_blocks) + k / 8) * 32 + b % 32) * 8 + k % 8], nnz_blocks = (nnz + 7) / 8 + 1;
                                        cnl_layout_len gives the array's length, cnl_interleave_dev / cnl_deinterleave_dev convert,
                                        cnl_prepare_newton_system_dev (row f2) writes it directly.  For device-resident callers of
                                        band-structured batches: every load of the band kernels then moves 512 contiguous bytes
                                        (16 384 problems of the headline pattern: 12.5 -> 11.0 ms; nothing to gain below 8 193
                                        problems).  rhs and d are problem-major in both layouts.  cnl_create fails (CNL_ERR_ARG) when
                                        the band kernels do not serve the handle.                                                   */
typedef struct cnl_options {
  int32_t struct_size;         /* sizeof(cnl_options), set by cnl_options_init (ABI evolution)                                  */
  int32_t plan_kind;           /* CNL_PLAN_*                                                                                    */
  int64_t staged_max_batch;    /* CNL_PLAN_AUTO: largest batch planned for latency (default 4096)                              */
  int32_t verbose;             /* 1: log plan decisions on stderr                                                               */
  int32_t band_kernel;         /* 1 (default): a throughput handle whose pattern is a band in the natural order of the variables
                                  (every residual row and Hessian entry within five consecutive variables, every constraint row a
                                  run of its own) runs on the band kernels (csrc/band.h: one lane per problem and half of the chain,
                                  operands streamed through LDS) — newton_system, try_to_factorize (the forward sweep alone) and
                                  solve_ldl! (which factorises the values of the last factorisation again and sweeps the new
                                  right-hand side in the same launch); 2: the same with the chain in one part; 0: the register-front
                                  kernel.  The band program moves its operands in 15 pieces of eight elements per epoch; the pattern
                                  of a CONSTRAINED model, whose H_c segment has the model's whole Hessian structure (every Hessian
                                  position twice), needs up to 18 and gets the WIDE form of the program and of the kernels (20
                                  pieces).  Float32 handles take it automatically; Float64 handles keep the register-front kernel
                                  for such a pattern, which measured faster, unless tuning "band_pieces=20" asks for the wide form
                                  ("band_pieces=15": never build it; 20 on a pattern 15 pieces serve: the wide kernels, bit-equal
                                  outputs).  cnl_get_config reports the piece count                                              */
  int32_t dense_backend;       /* 1: dense residual blocks (BASELINE config 2) go to the dense backend (fp64 MFMA)              */
  int32_t staged;              /* 1: latency plans run stage by stage (tasks of the elimination tree on different wavefronts)   */
  int32_t dataflow;            /* 1: smallest batches run all tasks in one launch per phase, waiting on device counters         */
  int32_t device_ladder;       /* 1: cnl_newton_system(_dev) on staged handles climbs the rho ladder inside ONE launch in which every
                                  task of the elimination tree has a wavefront of its own; 0: the sequential launch              */
  int32_t host_ladder;         /* 1: where the in-kernel ladder is not available (device_ladder = 0, split handles, the dense backend)
                                  the host-pointer cnl_newton_system drives the rho ladder from the host, every rung a staged
                                  try_to_factorize; 0: the sequential launch                                                    */
  int32_t split_tail;          /* 1: the remainder of a batch above a machine-filling one runs on a handle of its own, with the plan
                                  cnl_create picks for a batch of that size, behind the rest on the caller's stream             */
  int32_t multi_share_plan;    /* 1: cnl_multi_create analyses the pattern once for all shards of equal plan kind               */
  int32_t batch_layout;        /* layout of the `vals` arrays of the DEVICE-pointer entry points (CNL_LAYOUT_*; host-pointer calls take
                                  the reference's arrays, one problem after the other, always).  CNL_LAYOUT_INTERLEAVED: see below  */
  char force_order[32];        /* name of an ordering candidate to force ("" = none)                                            */
  char tuning[192];            /* "key=value[,key=value...]": any switch of csrc/options.h (measurement / test use)             */
} cnl_options;
void cnl_options_init(cnl_options* opt);

/* ---- symbolic analysis (host only; replaces `ldl_analyze`, ------------------
 *      src/solver_types.jl:61-65: sparse()+triu()+ldl_analyze) ---------------- */
int cnl_plan_create(cnl_plan** plan, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1,
                    int64_t nvar, int64_t nequ, int64_t ncon);
/* The analysis cnl_create(batch) runs: batches too small to give every CU a wavefront get an order with a bushy elimination
 * tree, cut into tasks that run on different wavefronts (plan arrays "tasks", "stage_ptr"); large batches get the order with
 * the least total work (one sequential record stream per four problems).  cnl_plan_create is the large-batch analysis.      */
int cnl_plan_create_for_batch(cnl_plan** plan, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1,
                              int64_t nvar, int64_t nequ, int64_t ncon, int64_t batch);
/* the same with explicit options (opt == NULL: defaults).  batch <= 0 with CNL_PLAN_AUTO means the large-batch analysis. */
int cnl_plan_create_ex(cnl_plan** plan, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1,
                       int64_t nvar, int64_t nequ, int64_t ncon, int64_t batch, const cnl_options* opt);
void cnl_plan_destroy(cnl_plan* plan);
/* info[0]=N [1]=nnz [2]=unique nnz(K) [3]=nsuper [4]=nnz(L) stored (strictly lower, with relaxed zeros)
 * [5]=nnz(L) of the ordering without relaxation [6]=factor storage doubles/problem [7]=largest front order
 * [8]=forward work-stack doubles [9]=backward work-stack doubles [10]=largest panel doubles
 * [11]=FMAs per factorisation [12]=assembly entries
 * [13]=fronts per class of the register-front kernel, packed (order<=16 | <=32 << 20 | <=64 << 40), -1 if unused
 * [14]=its LDS need, packed (update stack doubles | staging doubles << 20 | record words << 40), -1 if unused
 * [15]=residual nodes eliminated by static condensation (csrc/condense.h).  [4],[5] include their L rows. */
int cnl_plan_info(const cnl_plan* plan, int64_t info[16]);
/* Copy a named int32 index array of the plan.  "perm": elimination order in the reference's numbering
 * (0-based; condensed residual nodes first).  Multifrontal plan of the (condensed) system: "inner_perm",
 * "fronts" (16 int32 per front, struct FrontHdr in csrc/plan.h), "seg_ptr", "asm_pos", "asm_src",
 * "child_idx", "rel_idx".  Condensation lists (csrc/condense.h): "c_ptr", "c_a", "c_b", "c_d", "orig_of",
 * "r_orig", "r_dsrc", "r_ptr", "r_jsrc", "r_jx"; "cond_info" = {1 if the LDS-tiled condense kernel serves the plan (0: the plain slot
 * kernel), largest tile in elements, largest contribution and slot count of a chunk, chunks}, empty without condensation.  Record streams of the register-front kernel (csrc/plan.h; empty when that
 * kernel does not serve the plan): "rec", "brec".  Staged plans: "tasks" (8 int32 per task, struct Task in csrc/plan.h: stage,
 * first front, end front, record offset, backward record offset, 1 if a root, parent task or -1, number of child tasks),
 * "stage_ptr".  With out == NULL only *count is set.
 * Used by the tests' plan simulator and to hand the ordering to the oracle.                          */
int cnl_plan_get(const cnl_plan* plan, const char* name, int32_t* out, int64_t* count);
const char* cnl_plan_order_name(const cnl_plan* plan);

/* ---- solver object (replaces LDLFactStruct(N, rows, cols, vals), ---------------
 *      src/solver_types.jl:45-51,61-65; called at src/CaNNOLeS.jl:327) --------- */
int cnl_create(cnl_handle** h, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1,
               int64_t nvar, int64_t nequ, int64_t ncon, int64_t batch, int device);
/* cnl_create with explicit options (opt == NULL: defaults = cnl_create) */
int cnl_create_ex(cnl_handle** h, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1,
                  int64_t nvar, int64_t nequ, int64_t ncon, int64_t batch, int device, const cnl_options* opt);
int cnl_destroy(cnl_handle* h);
/* Number of dataflow waits that gave up since the handle was created (see cnl_options.dataflow_spin_limit).  Every such call
 * was redone by the sequential execution, so results are right; a non-zero count says the device did not run the workgroups
 * of a launch concurrently / in index order (time-slicing, a debugger).  Synchronises the handle's last call.                 */
int cnl_dataflow_timeouts(cnl_handle* h, int64_t* count);
const cnl_plan* cnl_get_plan(const cnl_handle* h);

/* try_to_factorize(LDLT, vals, nvar, nequ, ncon, eig_tol) — src/solver_types.jl:79-98.
 * vals: batch*nnz values (rho slots as given).  success[b] = 1 iff the factorisation completed
 * with #{d > eig_tol} == nvar and #{|d| <= eig_tol} == 0.  npos/nzero (optional, batch each)
 * return the two counts.                                                                      */
int cnl_factorize(cnl_handle* h, const double* vals, double eig_tol, int32_t* success, int64_t* npos, int64_t* nzero);

/* solve_ldl!(rhs, factor, d) — src/solver_types.jl:69-77: d = -(K^-1 rhs); rhs untouched.
 * Requires a preceding cnl_factorize / cnl_newton_system.  The reference never solves after a failed factorisation
 * (src/CaNNOLeS.jl:1049); here: with batch = 1 that call sequence returns CNL_ERR_STATE (nothing is written); in a batch the rows of
 * d that belong to problems whose last host-pointer factorisation failed are left untouched.  After a device-pointer
 * factorisation the flags are not known to the host: cnl_solve / cnl_solve_dev then write unspecified (finite or not) values for
 * the problems that failed — the caller holds d_success and must not use those rows.                                          */
int cnl_solve(cnl_handle* h, const double* rhs, double* d);

/* newton_system!(d, nvar, nequ, ncon, rhs, vals, LDLT, rho_old, params) — src/CaNNOLeS.jl:1008-1052,
 * one call: factorise at rho=0, climb the rho ladder per problem on failure, solve.  Both entries decide the ladder on the device:
 * the single stream of large batches inside its one launch, latency plans (small and mid-size batches) inside one fused launch in
 * which every task of the elimination tree has a wavefront of its own (cnl_options.device_ladder; kernels2.hip, phase 2).  Only where
 * that launch cannot hold a batch's tasks at once — and on the dense backend — the ladder of THIS (host-pointer) entry is driven from
 * the host, every rung a parallel try_to_factorize of the batch (cnl_options.host_ladder), and the device-pointer twin falls back
 * to the sequential launch.
 * vals (batch*nnz) is mutated: the rho slots receive the last rho tried, as the reference leaves them.
 * rho_old: batch inputs.  Outputs (batch each): rho, rho_old_out, nfact, success (= solve_success).  */
int cnl_newton_system(cnl_handle* h, double* vals, const double* rhs, double* d, const double* rho_old,
                      const double params[9], double* rho, double* rho_old_out, int32_t* nfact, int32_t* success);

/* Device-resident twins.  d_vals/d_rhs/d_d are device pointers with the layouts above.
 * d_rho_old is read and updated in place (rho_old_out); d_rho, d_nfact, d_success are outputs. */
int cnl_factorize_dev(cnl_handle* h, const double* d_vals, double eig_tol, int32_t* d_success, void* stream);
/* (cnl_solve_dev on a handle made with tuning "float32_refine" — below — reads the d_vals of the last factorisation again, for its
 *  Float64 residuals: they must stay alive and UNMODIFIED until the last cnl_solve_dev on that factor.) */
int cnl_solve_dev(cnl_handle* h, const double* d_rhs, double* d_d, void* stream);
int cnl_newton_system_dev(cnl_handle* h, double* d_vals, const double* d_rhs, double* d_d, double* d_rho_old,
                          double* d_rho, int32_t* d_nfact, int32_t* d_success, const double params[9], void* stream);

/* ---- vectors either side of the Newton system, device-resident ------------------
 * They let `rhs` and `d` stay in HBM between inner iterations instead of crossing PCIe every call.
 *
 * cnl_residual_vectors_dev: rhs = [dual ; primal] and their infinity norms, as src/CaNNOLeS.jl computes them at
 * :507-508, :519-524, :528-529 (start), :722-726, :730-731 (trial point) and assembles at :631-632:
 *     dual = Jx' r - Jc' lambda,   primal = [F - r ; c],   norms[2b] = ||dual||_inf, norms[2b+1] = ||primal||_inf.
 * The Jacobian values are read from the J_F / J_c segments of `vals` (prepare_newton_system!, :953-967).  Both
 * products are accumulated per column in COO order (the order of the reference's COO mul!) and then subtracted.
 * Batched layouts: r, Fx [batch][nequ]; lambda, cx [batch][ncon] (may be NULL when ncon == 0); rhs [batch][N].   */
int cnl_residual_vectors_dev(cnl_handle* h, const double* d_vals, const double* d_r, const double* d_lambda, const double* d_Fx,
                             const double* d_cx, double* d_rhs, double* d_norms, void* stream);

/* The same two rows with the Jacobian values read from the MODEL's arrays Jx [batch][nnzjF], Jcx [batch][nnzjc] — what
 * prepare_newton_system! copies into the J_F / J_c segments of vals, and what the reference's own products use (`mul!(Jxtr, Jx', r)`,
 * src/CaNNOLeS.jl:507: the Jx operator is built on Jx_vals) — instead of from `vals`: no prepare pass is needed in front of them, and they
 * serve handles of either batch_layout.  Results bit-identical to the `vals` variants (same kernels, another base pointer).  The pattern's
 * J_F and J_c entries must be one run of COO slots each (the reference's 7-segment layout; CNL_ERR_STATE otherwise).               */
int cnl_residual_vectors_jac_dev(cnl_handle* h, int64_t nnzjF, int64_t nnzjc, const double* d_Jx, const double* d_Jcx, const double* d_r,
                                 const double* d_lambda, const double* d_Fx, const double* d_cx, double* d_rhs, double* d_norms, void* stream);
int cnl_cgls_multipliers_jac_dev(cnl_handle* h, int64_t nnzjF, int64_t nnzjc, const double* d_Jx, const double* d_Jcx, const double* d_r,
                                 double* d_lambda, double* d_Jxtr, double atol, double rtol, int64_t itmax, int ones_if_zero,
                                 int32_t* d_iters, void* stream);

/* cnl_prepare_newton_system_dev: prepare_newton_system!(meth, vals, nls, x, lambda, r, Jx_vals, Jcx_vals, delta, Fx) —
 * src/CaNNOLeS.jl:947-981 — for a batch whose model values already live on the device: the value
 * arrays are copied into the segments of `vals` ([H_F | H_c | J_F | J_c | -I | -delta I | rho I], sizes nnzhF, nnzhc,
 * nnzjF, nnzjc, nequ, ncon, nvar):  H_F <- hF (skipped when d_hF == NULL: the Gauss-Newton variants do not touch it),
 * H_c <- -hc, J_F <- Jx, J_c <- Jcx, -delta I <- -delta[b], rho I <- 0; the -I segment is never written.
 * Layouts: hF [batch][nnzhF], hc [batch][nnzhc], Jx [batch][nnzjF], Jcx [batch][nnzjc], delta [batch].          */
int cnl_prepare_newton_system_dev(cnl_handle* h, int64_t nnzhF, int64_t nnzhc, int64_t nnzjF, int64_t nnzjc, const double* d_hF,
                                  const double* d_hc, const double* d_Jx, const double* d_Jcx, const double* d_delta, double* d_vals,
                                  void* stream);
/* On a handle created with cnl_options.batch_layout = CNL_LAYOUT_INTERLEAVED, cnl_prepare_newton_system_dev WRITES d_vals interleaved
 * (the model's arrays stay problem-major), and cnl_factorize_dev / cnl_newton_system_dev read — the rho slots: write — d_vals in that
 * layout; d_rhs and d_d are problem-major.  cnl_residual_vectors_dev and cnl_cgls_multipliers_dev read problem-major vals only
 * (CNL_ERR_STATE on such a handle: use their `_jac` twins above), the host-pointer entry points likewise.
 *   cnl_layout_len: doubles of the interleaved array for the handle's batch, which = 0: vals, 1: an N-vector per problem;
 *   cnl_interleave_dev / cnl_deinterleave_dev: problem-major -> interleaved / back (out of place; pads are written as zeros).     */
int cnl_layout_len(const cnl_handle* h, int which, int64_t* doubles);
int cnl_interleave_dev(cnl_handle* h, int which, const double* d_src, double* d_dst, void* stream);
int cnl_deinterleave_dev(cnl_handle* h, int which, const double* d_src, double* d_dst, void* stream);

/* cnl_cgls_multipliers_dev: least-squares multiplier estimate  min || Jc' lambda - Jx' r ||  (SURVEY 8 row f4), what the
 * reference obtains with `mul!(Jxtr, Jx', r); krylov_solve!(cgls_workspace, Jcx', Jxtr)` at src/CaNNOLeS.jl:507-518 and
 * :880-882: CGLS started at 0, stopped when ||Jc res|| <= atol + rtol ||Jc b|| or after itmax steps (itmax <= 0: nvar + ncon,
 * Krylov.jl's default; its default tolerances are sqrt(eps)).  ones_if_zero != 0 applies `if norm(lambda) == 0: lambda .= 1`
 * (:515-517).  d_Jxtr (optional) receives Jx' r, d_iters (optional) the iteration counts.
 * Number of constraints, tuning "cgls_wide" (all four entry points, cnl_cgls_multipliers[_jac][_f32]_dev; cnl_get_config bits 45 / 46 of
 * cfg[5] report the value): 0 (the default) the kernel keeps its three ncon-vectors in LDS and ncon > 1024 is CNL_ERR_DIM with nothing
 * launched; 1 a handle with ncon > 1024 runs the wide instance, whose ncon-vectors live in the handle's workspace (any ncon), every other
 * handle the LDS instance; 2 the wide instance always.  The two instances do the same operations in the same order: bit-equal results.
 * Any other value is CNL_ERR_ARG at creation.
 * itmax: any int64_t; <= 0 selects the default nvar + ncon, a value above INT_MAX (typemax(Int64) for "no limit") counts as INT_MAX. */
int cnl_cgls_multipliers_dev(cnl_handle* h, const double* d_vals, const double* d_r, double* d_lambda, double* d_Jxtr, double atol,
                             double rtol, int64_t itmax, int ones_if_zero, int32_t* d_iters, void* stream);

/* cnl_trial_point_dev: the extrapolation step's trial point, src/CaNNOLeS.jl:654,661-668:
 *     xt = x + d[1:n],  rt = r + d[n+1:n+m],  dlambda = -d[n+m+1:N], scaled by max_dlambda/||dlambda||_2 when that
 *     norm exceeds max_dlambda (the reference uses 1e4),  lambdat = lambda + dlambda.                               */
/* cnl_kkt_residual_dev: g[b] = rhs[b] + K(vals[b]) d[b] and norms[b] = max_i |g[b][i]| for the problems the handle works on — the
 *   residual of the Newton system, K the symmetric matrix of the lower-triangular COO pattern (duplicates summed, strict-lower entries
 *   mirrored, the rho slots read as they stand in vals).  The only way a device-resident caller can check a Newton step without
 *   leaving the device.  Any Float64 handle with problem-major vals (batch_layout = CNL_LAYOUT_INTERLEAVED: CNL_ERR_STATE).  Sums run
 *   in double along the rows of the full matrix (cnl_plan_get "kkt_row_ptr" / "kkt_row_slot" / "kkt_row_col": for every row its
 *   (slot, column) pairs in ascending slot order; built and uploaded on first use), without atomics: two calls give the same bits.
 *   d_g [batch][N] must not overlap an input; d_norms [batch] may be null.  Tuning "refine_rows" (0 by the pattern, 1 a row per
 *   lane, 2 a row per wavefront) picks the kernel instance. */
int cnl_kkt_residual_dev(cnl_handle* h, const double* d_vals, const double* d_rhs, const double* d_d, double* d_g, double* d_norms,
                         void* stream);

int cnl_trial_point_dev(cnl_handle* h, const double* d_x, const double* d_r, const double* d_lambda, const double* d_d,
                        double max_dlambda, double* d_xt, double* d_rt, double* d_lambdat, double* d_dlambda, void* stream);

/* ---- one caller, several devices -------------------------------------------------------------------------
 * The path shards only across independent problems: `batch` problems are cut into contiguous balanced shards, one per entry
 * of `devices` (the first batch % ndev shards hold one problem more; with batch < ndev the surplus devices stay idle), each
 * shard with a handle of its own on its device.  The calls below take the arrays of the WHOLE batch (problem-major, as the
 * single-handle calls), run every shard from a host thread of its own and return when all are done; there is no collective
 * and no traffic between the devices.  This is what a single `cannoles()`-style caller (one backend object selected at
 * src/CaNNOLeS.jl:322-332) uses to drive all GPUs of a node without becoming one process per GPU.                          */
typedef struct cnl_multi cnl_multi;
int cnl_multi_create(cnl_multi** m, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar, int64_t nequ,
                     int64_t ncon, int64_t batch, const int* devices, int ndev);
/* the same with explicit options (opt == NULL: defaults).  The pattern is analysed ONCE for all shards (cnl_options.multi_share_plan). */
int cnl_multi_create_ex(cnl_multi** m, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar, int64_t nequ,
                        int64_t ncon, int64_t batch, const int* devices, int ndev, const cnl_options* opt);
int cnl_multi_destroy(cnl_multi* m);
/* shards actually created: *nshards, and (optional arrays of that length) first problem, problems, device index */
int cnl_multi_shards(const cnl_multi* m, int64_t* nshards, int64_t* start, int64_t* count, int32_t* device);
int cnl_multi_factorize(cnl_multi* m, const double* vals, double eig_tol, int32_t* success, int64_t* npos, int64_t* nzero);
int cnl_multi_solve(cnl_multi* m, const double* rhs, double* d);
int cnl_multi_newton_system(cnl_multi* m, double* vals, const double* rhs, double* d, const double* rho_old, const double params[9],
                            double* rho, double* rho_old_out, int32_t* nfact, int32_t* success);

/* Device-resident twins: entry i of every pointer array is shard i's device array on shard i's device (problem-major,
 * count[i] problems; cnl_multi_shards).  The calls enqueue every shard's work on streams[i] (NULL: the shard handle's own
 * stream) from the calling thread and return; nothing crosses PCIe or xGMI.  cnl_multi_synchronize waits for all shards.   */
int cnl_multi_factorize_dev(cnl_multi* m, const double* const* d_vals, double eig_tol, int32_t* const* d_success, void* const* streams);
int cnl_multi_solve_dev(cnl_multi* m, const double* const* d_rhs, double* const* d_d, void* const* streams);
int cnl_multi_newton_system_dev(cnl_multi* m, double* const* d_vals, const double* const* d_rhs, double* const* d_d,
                                double* const* d_rho_old, double* const* d_rho, int32_t* const* d_nfact, int32_t* const* d_success,
                                const double params[9], void* const* streams);
int cnl_multi_synchronize(cnl_multi* m, void* const* streams);

/* ---- bookkeeping of the batched outer / inner loop, device-resident -----------------------------------------
 * A caller that runs `solve!` (src/CaNNOLeS.jl:612-864) for a batch of problems in lockstep keeps the loop's state as [batch, ...]
 * arrays in HBM and every branch as a per-problem mask (cannoles.jl_amd/device_loop.py).  The four entry points below do the
 * masks and the masked state updates of one global step IN PLACE on that state, one launch each (the reference's tests in the
 * reference's operation order; minimum / maximum propagate NaN).  `cnl_outer_state` is plain device pointers and sizes; every
 * array is problem-major.  Status codes: 0 unknown (active), 1 first_order, 2 small_residual, 3 exception,
 * 4 max_eval (the evaluation count neval > max_eval; produced by cnl_outer_end_ex_dev only: the plain calls have no evaluation counter),
 * 5 stalled (inner > max_inner, src/CaNNOLeS.jl:846), 6 max_iter (outer iterations > max_iter; cnl_outer_end_ex_dev only), 7 max_time
 * (never written by a kernel: reserved for the caller, who owns the clock and sets it in `status` for the problems still active).  Where
 * several causes hold at once the lowest of 1, 2, 3, 4, 6, 5 in that order is reported (get_status, :836-847).  The entry points
 * take no handle: they launch on the calling thread's CURRENT device, which must be the one the arrays live on, and are asynchronous on
 * `stream`; they return CNL_ERR_ARG for a null state / missing array and CNL_ERR_HIP when the launch fails.  Every array is required
 * — the multiplier / constraint arrays lam, cx, ct, lamt, lamt_e (cl, lam_ls for the line search) have rows of P = max(p, 1) entries and
 * are required also when p == 0 —; only Jcv / Jct may be NULL when nnzjc == 0.
 *   cnl_outer_begin_dev        :612-626  start of an outer iteration for the problems in phase0; act, need (a Newton system is due);
 *                                        flags[0..3] = any active / any need / any extrapolation step / any line-search step
 *   cnl_outer_newton_done_dev  :633-659  did_newton != 0: d, rho_old, nfact, nlin from the Newton call's outputs (d_new, ro_tmp,
 *                                        nf_new, rho_new, ok_new) where `need`; brk (`broken`); then ext / lsm and eps_k where ext
 *   cnl_outer_extrapolated_dev :661-668  xt, rt, lamt <- the trial point cnl_trial_point_dev left in xt_e, rt_e, lamt_e, where ext
 *   cnl_outer_trial_done_dev   :722-800  optimality measures at the trial point (nrm_t = the norms of cnl_residual_vectors_dev),
 *                                        acceptance, x / r / Fx / cx / Jv / Jcv / lam / rhs_cur / fx / delta / inner updates, end-of-
 *                                        inner-loop tests; rej, chk, done_in; flags[4] = any rejected, flags[5] = any small-residual check
 *   cnl_outer_end_dev          :800-857  statuses, outer-iteration counters, phase0
 *   cnl_outer_compact_dev      (no counterpart: one problem has no batch) the active problems to the front of every array, below
 * The keywords of `solve!` beyond max_inner and the tolerances (:418-437) come through a control block, `cnl_outer_ctl` below, and the
 * `_ex` twins of begin / trial_done / ls_test / end; cnl_outer_hess_mask_dev serves method = :Newton_vanishing.                       */
typedef struct cnl_outer_state {
  int64_t B, n, m, p, P /* max(p, 1): row length of lam, cx, ct, lamt */, N, nnzjF, nnzjc, max_inner;
  double dmin, rhomax, delta_dec, smax;
  int32_t *status, *it, *flags /* [8] */, *nf_new, *ok_new;
  int64_t *inner, *nfact, *nlin;
  uint8_t *phase0, *act, *need, *brk, *ext, *lsm, *rej, *chk, *done_in, *tired, *small_res;
  double *normdual, *normprimal, *combined, *combined_hat, *delta, *ndh, *nph, *fx, *epsk, *epstol, *epsF, *epsc, *rho_old;
  double *d, *d_new, *ro_tmp, *rho_new;
  double *x, *r, *Fx, *cx, *Jv, *Jcv, *lam, *rhs_cur;
  double *xt, *rt, *Ft, *ct, *Jt, *Jct, *lamt, *rhs_t, *nrm_t /* [B][2] */;
  double *xt_e, *rt_e, *lamt_e;
  /* Armijo line search (src/CaNNOLeS.jl:1054-1112): ls_g = the [dual; primal] vector of cnl_residual_vectors_dev at (Fx, lam_ls) —
   * its first n entries are the gradient of the merit function; xl / Fl / cl = trial point, F and c there (the caller evaluates
   * the model); lam_ls = lam - c / delta; per problem: alpha, Dphi, phix, eta, nbk; bt = still backtracking; flags[6] = any bt  */
  double gammaA, eps2;
  double *ls_g, *xl, *Fl, *cl, *lam_ls, *alpha, *Dphi, *phix, *eta;
  int64_t* nbk;
  uint8_t* bt;
} cnl_outer_state;
int cnl_outer_begin_dev(const cnl_outer_state* st, void* stream);
int cnl_outer_newton_done_dev(const cnl_outer_state* st, int did_newton, void* stream);
int cnl_outer_extrapolated_dev(const cnl_outer_state* st, void* stream);
int cnl_outer_trial_done_dev(const cnl_outer_state* st, void* stream);
/* line search of the problems in lsm: ls_begin (Dphi, eta, phi(x), alpha = 1, xl = x + dx) -> [caller: Fl, cl = F(xl), c(xl)] ->
 * ls_test(first = 1) -> while flags[6]: ls_step (alpha / 4, xl, nbk) -> [caller: Fl, cl] -> ls_test(0); then ls_take (xt, rt, lamt)   */
int cnl_outer_ls_begin_dev(const cnl_outer_state* st, void* stream);
int cnl_outer_ls_test_dev(const cnl_outer_state* st, int first, void* stream);
int cnl_outer_ls_step_dev(const cnl_outer_state* st, void* stream);
int cnl_outer_ls_take_dev(const cnl_outer_state* st, void* stream);
int cnl_outer_end_dev(const cnl_outer_state* st, void* stream);
/* Control block of the `_ex` entry points: the keywords always_accept_extrapolation, max_iter and max_eval of `solve!` (:418-437).
 * Integers only, so one structure serves both element types.  neval[b] is the number of model evaluations problem b has made, as its
 * single-problem run counts them: the caller sets it to evals_per_point for the evaluation at the start point, and the kernels add
 * evals_per_point for every point they know was evaluated for the problem — the extrapolation's trial point (trial_done_ex, the problems
 * of `ext`) and each candidate of the line search (ls_test_ex: the problems of `lsm` when first != 0, else those of `bt`).  Evaluations
 * a batched caller makes for its own convenience on rows that did not need them are not the problem's and are not counted.
 *   cnl_outer_begin_ex_dev       need = act && (inner != 1 || always_accept_extrapolation)                                   (:627)
 *   cnl_outer_trial_done_ex_dev  the state is accepted where act && (inner > 0 || always_accept_extrapolation || good)       (:735);
 *                                neval += evals_per_point where ext; tired = inner > max_inner || (max_eval >= 0 && neval > max_eval)
 *   cnl_outer_ls_test_ex_dev     neval += evals_per_point for every candidate of the call
 *   cnl_outer_end_ex_dev         statuses 4 (max_eval >= 0 && neval > max_eval) and 6 (max_iter >= 0 && it > max_iter, `it` already
 *                                incremented) in the chain 1, 2, 3, 4, 6, 5
 *   cnl_outer_hess_mask_dev      hess_upd[b] = dot(Fx_b, Fx_b) > 1e-8 (hessian_approx.jl:55-60; the dot product accumulated in double,
 *                                rounded to the element type once, compared with the double literal); one workgroup per problem
 * ctl == NULL: exactly the plain call (cnl_outer_hess_mask_dev needs a block).  CNL_ERR_ARG with nothing launched for a struct_size other
 * than sizeof(cnl_outer_ctl), a null neval, evals_per_point outside {1, 2}, and for cnl_outer_hess_mask_dev a null hess_upd.           */
typedef struct cnl_outer_ctl {
  int32_t struct_size;                   /* sizeof(cnl_outer_ctl) */
  int32_t always_accept_extrapolation;   /* :627, :735 */
  int64_t max_iter;                      /* < 0: no limit */
  int64_t max_eval;                      /* < 0: no limit */
  int64_t evals_per_point;               /* 1, or 2 when p > 0: residual + constraints (eval_fun, :559) */
  int64_t* neval;                        /* [B] device: evaluations per problem, updated in place */
  uint8_t* hess_upd;                     /* [B] device, optional: out of cnl_outer_hess_mask*_dev */
} cnl_outer_ctl;
int cnl_outer_begin_ex_dev(const cnl_outer_state* st, const cnl_outer_ctl* ctl, void* stream);
int cnl_outer_trial_done_ex_dev(const cnl_outer_state* st, const cnl_outer_ctl* ctl, void* stream);
int cnl_outer_ls_test_ex_dev(const cnl_outer_state* st, int first, const cnl_outer_ctl* ctl, void* stream);
int cnl_outer_end_ex_dev(const cnl_outer_state* st, const cnl_outer_ctl* ctl, void* stream);
int cnl_outer_hess_mask_dev(const cnl_outer_state* st, const cnl_outer_ctl* ctl, void* stream);
/* cnl_outer_compact_dev: the active problems (status == 0) become the first rows of the state, so that the caller can go on with
 * st->B = their number (and cnl_set_active_batch on its handle) instead of running every kernel of a step over finished problems.
 * Like its siblings: no handle, the current device, asynchronous on `stream`, CNL_ERR_ARG with nothing launched for a null state,
 * B <= 0, a missing array, a null d_orig / d_counts / d_work, min_finished < 1, nextra outside [0, 24] or a null / empty extra array.
 * With Bc = st->B and A = the number of rows b < Bc with status[b] == 0:
 *   Bc - A < min_finished: nothing moves, d_counts = {A, Bc};
 *   otherwise the k-th finished row below A (ascending) and the k-th active row at or above A (ascending) change places, for every k,
 *   and d_counts = {A, A}: rows 0 .. A-1 then hold exactly the active problems.
 * The swap applies to every per-problem array of the state that is there (all element, counter and mask members, nrm_t with its two
 * entries per row; `flags` is global and stays; an array given under two members, as Jcv / Jct may be, moves once), to the nextra
 * arrays d_extra[i] with rows of extra_row_bytes[i] bytes (the model's per-problem data) and to d_orig, int32 [B]: the original index
 * of the problem in each row, which the caller sets to 0 .. B-1 at the start.  Rows change places in place; all B rows stay a
 * permutation of what they were.  d_extra and extra_row_bytes are HOST arrays (of device pointers / sizes), d_counts is int32 [2] and
 * d_work int32 [B + 2] on the device (the pair list; nothing is allocated per call).  Two launches, no host synchronisation.      */
int cnl_outer_compact_dev(const cnl_outer_state* st, int64_t nextra, void* const* d_extra, const int64_t* extra_row_bytes, int64_t min_finished,
                          int32_t* d_orig, int32_t* d_counts, int32_t* d_work, void* stream);

/* ---- a handle on the first problems of its batch -------------------------------------------------------------------------------
 * cnl_set_active_batch(h, nb): from here on every DEVICE-pointer entry point of the handle treats it as a batch of the problems
 * 0 .. nb-1 — cnl_factorize*_dev, cnl_solve*_dev, cnl_newton_system*_dev, cnl_prepare_newton_system*_dev, cnl_residual_vectors*_dev,
 * cnl_cgls_multipliers*_dev (and their `_jac` twins), cnl_trial_point*_dev, cnl_interleave*_dev, cnl_deinterleave*_dev, either element
 * type.  Only the launch extent changes: every array keeps the addressing of the CREATED batch (problem-major rows, the groups of 32 of
 * an interleaved `vals`, cnl_layout_len), what is written for a problem < nb is bit-equal to what the full-batch call writes for it, and
 * nothing that belongs to a problem >= nb is written (its rows, its elements of an interleaved array — also inside a group of 32 that
 * is active in part).  A caller whose problems finish at different times (the lockstep loop below, cnl_outer_compact_dev) keeps the
 * active ones in front and stops paying for the others.
 *   nb outside [1, created batch]: CNL_ERR_ARG.  nb = created batch restores the handle exactly and is accepted by every handle.
 *   Served: band handles (Float64 and Float32, both layouts, 15- and 20-piece programs, the resident form) and handles whose calls are
 *   the one classic launch of the register-front or the general kernel, with or without condensation.  CNL_ERR_STATE, the handle
 *   unchanged and cnl_last_error naming the case: handles that run staged / dataflow, handles that run their batch split (tail handle,
 *   halves, concurrent parts), the dense backend.  cnl_multi has no counterpart.
 *   While nb is below the created batch the host-pointer entry points return CNL_ERR_STATE (they take the whole batch's arrays), and
 *   cnl_solve*_dev needs a last factorisation that covered at least nb problems (CNL_ERR_STATE otherwise).                        */
/*   (A refined handle — tuning "float32_refine" — forwards to its inner handle and returns its answer.) */
int cnl_set_active_batch(cnl_handle* h, int64_t nb);
int cnl_get_active_batch(const cnl_handle* h, int64_t* nb);

/* Device time, in milliseconds, of the multifrontal kernel (the dominant kernel) of the last call,
 * measured with HIP events on the call's stream.  Enabling timing makes every call synchronise on
 * its stream, so it is meant for measurement loops, not for production (0 if not enabled).      */
int cnl_set_timing(cnl_handle* h, int enable);
int cnl_last_kernel_ms(cnl_handle* h, float* ms);

/* Kernel configuration actually chosen: cfg[0]=threads per problem, [1]=problems per workgroup,
 * [2]=LDS bytes per workgroup, [3]=1 if the work stack lives in LDS else 0 (global scratch),
 * [4]=grid size (those five describe the general kernel, kernels.hip), [5]=2 if the register-front
 * kernel (kernels2.hip) serves newton_system/factorize (4: with staged execution of the first attempt), 3 dense backend, else 1;
 * + 16 when newton_system / factorize run the LEAN instantiation (fast-class fronts with row-form products only), [6]=its wavefronts per workgroup,
 * [7]=its LDS bytes per workgroup; [5] + 32 when the remainder of the batch runs on a handle of its own (cnl_options.split_tail),
 * + 64 when cnl_newton_system runs on the band kernels (then bits 8-15 = problems per workgroup, bits 16-17 = parts of the chain (one or two),
 *   bits 18-22 = the cache policy mask of the mover-table instance (tuning "band_cache_policy", below; 0 on every other instance),
 *   bit 24 = the RESIDENT form of the 15-piece program runs (aligned blocks of `vals` kept in LDS: Float64, batch_layout = 1, 32 problems
 *   per workgroup; tuning "band_resident=0" keeps the 15-piece program — bit-equal outputs either way),
 *   bits 25-26 = cnl_options.batch_layout / rhs interleaved, bits 28-33 = operand pieces per epoch of the band program: 15, or 20
 *   for the wide form, bit 34 = the resident program's mover follows the host-built mover table (csrc/band.h; tuning
 *   "band_mover_table=0" keeps the resident instance that decodes piece descriptors — bit-equal outputs either way)),
 * + 128 when cnl_residual_vectors_dev runs on column tiles,
 * bit 36 = the handle runs on the Direct route: the register-front kernel condenses on the fly from the caller's vals (no
 *   stand-alone condensation pass in front of the launch), either element type,
 * bit 37 = ... and cnl_solve* runs on the register-front kernel too (every front of the fast class),
 * bit 47 = cnl_newton_system* / cnl_factorize* run a BLOCKED instance of the general kernel (tuning "general_blocked=1", below).
 *
 * Tuning "band_cache_policy" (7 default; 0 or 7, any other value CNL_ERR_ARG at plan creation): the cache policy of the band kernel's
 * mover-table instance (bit 34), a bit mask over the streams it touches once per sweep — 1 typed `vals` loads non-temporal, 2 typed
 * factor loads non-temporal, 4 factor-record stores non-temporal, 8 the same stores written through (never with 4), 16 `d` stores
 * non-temporal.  Only the masks the library has an instance for are accepted: 0 (every access plain) and 7.  Every output is bit for
 * bit that of 0; 7 measured 5 % faster at 16 384 problems (tools/time_band_policy.py).  A handle that runs another
 * instance ignores the key and reports 0 in bits 18-22.
 *
 * Tuning "general_blocked" (0 default, 1; any other value CNL_ERR_ARG): on a Float64 handle whose newton_system / factorize launches
 * are the general kernel's (cfg[5] & 15 == 1) with 256 or 1024 threads per problem and one problem per workgroup, a front with 16
 * pivots or more is eliminated in panels of 16 pivots — the pivots of a panel one by one against the rows of the panel, then ONE
 * update of everything below the panel on the f64 matrix cores — instead of one sweep over the whole front per pivot.  Same
 * factor layout and solve sweeps, same inertia rule; such a handle keeps the success flags of its last factorisation, and cnl_solve*
 * leaves the rows of d of a problem whose factorisation failed untouched (without the key the general kernel overwrites them);
 * the sums of an update are formed in another order, so d agrees with the key off to rounding, not bit for bit.  The work area grows by 14 rows of the largest front (it may move from LDS
 * to global scratch: cfg[3]).  A handle whose configuration has no blocked instance (64 threads per problem or fewer, the
 * register-front kernel, the band kernels, the dense backend) runs as without the key and reports bit 47 clear.  There are no
 * Float32 instances behind THIS key: cnl_create_f32* with the key, and the key together with "float32_refine", are CNL_ERR_ARG
 * (a Float32 general handle has "float32_blocked", next).  cnl_multi shards inherit it.  Measured: DESIGN section 3.1.
 *
 * bit 48 = cnl_newton_system_f32* / cnl_factorize_f32* of a Float32 general handle run a BLOCKED float instance of the general kernel
 * (tuning "float32_blocked=1"); bit 47 keeps its Float64-only meaning.
 *
 * Tuning "float32_blocked" (0 default, 1): "general_blocked" for a Float32 general handle, with the trailing updates on the f32
 * matrix cores (v_mfma_f32_16x16x4_f32).  Rules, all answered before a device is looked for: only together with
 * "float32_general=1" (alone: CNL_ERR_ARG); any value other than 0 / 1 is CNL_ERR_ARG; together with "float32_refine" it is
 * CNL_ERR_ARG at cnl_create_ex and at cnl_plan_create_ex (no refined handle over a blocked Float32 factor), as "float32_staged" is.
 * A Float64 creator without "float32_refine" reads nothing of the key, neither its value nor its rules — exactly as it reads
 * nothing of "float32_condense".  The key selects no route: every handle gets the route it gets without it (band kernels,
 * register-front kernel, staged / latency, "float32_dense", "float32_general_dense"), and it acts only where that route launches
 * the general kernel in float for newton_system / factorize with one problem per workgroup and 256 threads — the uncondensed
 * Float32 general handle and the "float32_condense" one (also a "float32_register_front" handle that fell back to it because a
 * front is above order 64) whose largest front is above order 96, or with "v1_tpp=256".  With 64 threads per problem (largest
 * front of order <= 96 without "v1_tpp") there is no blocked instance: the handle runs unblocked and reports bit 48 clear.  The work
 * area grows by 14 rows of the largest front, in 4-byte elements, and is placed in LDS or global scratch with that size (cfg[3]).
 * As in Float64 the handle keeps the success flags of its last factorisation and cnl_solve_f32* leaves the rows of d of a failed
 * problem untouched; decisions (success, nfact, rho, rho_old, the rho slots) are those of the handle without the key wherever the
 * pivots keep the project's Float32 margin from eig_tol, d agrees to Float32 rounding, not bit for bit.  Measured: DESIGN
 * section 9.10.
 *
 * bit 49 = cnl_newton_system* / cnl_factorize* / cnl_solve* run the general kernel's SUBTREE instances stage by stage (tuning
 * "general_subtrees=1").
 *
 * Tuning "general_subtrees" (0 default, 1; any other value CNL_ERR_ARG; at cnl_create_f32* and together with "float32_refine" — at
 * cnl_create_ex and cnl_plan_create_ex — CNL_ERR_ARG, answered before a device is looked for): the elimination tree is cut into
 * tasks — maximal bottom subtrees of at most "task_cap" fronts (default 8), every front above on its own, a task's stage = 1 + the
 * latest stage of its children's tasks — and each of the three calls runs the general kernel as one launch per stage with one
 * workgroup per (problem, task): S forward launches, where the call factorises a decide kernel (inertia test over the tasks' pivot
 * counts), where it solves S backward launches in reverse, and for newton_system one launch more in which the problems that failed
 * the first attempt run the whole rho ladder sequentially (the others leave at once).  Launches per call: newton_system 2 S + 2,
 * factorize S + 1, solve 2 S (cnl_launch_counts counts them in its general-kernel slot).  Dependencies are the order of the launches
 * on the stream alone.  The key selects no route and changes no ordering, front or factor layout; it acts where the launch is the
 * general kernel ([5] & 15 == 1, condensed or not) with one problem per workgroup of 256 or 1024 threads, the first stage holds at
 * least two tasks, and batch x gwork x 8 <= 8e9 bytes, gwork = cnl_plan_get "ginfo"[0] elements: every task owns a region of the
 * per-problem work area (global memory; cfg[3] = 0), never reused within a call.  Every other handle is the one without the key and
 * reports bit 49 clear.  It combines with "general_blocked" (subtrees for the walk over the small fronts, panels for the separator
 * fronts).  As a blocked handle it keeps the success flags of its last factorisation: cnl_solve* leaves the rows of d of a failed
 * problem untouched.  Decisions and d are those of the handle without the key, bit for bit on every tested case (the per-front
 * arithmetic is the same code).  cnl_plan_get: "gtasks" (8 words per task: stage, first front, end front, parent task, region
 * base, panel buffer offset, staging offset, staging stride), "gstage_ptr", "gfronts" (the front table with foff / ubase / xoff inside
 * the task regions), "ginfo" = {gwork, tasks, stages, tasks of the first stage, cap}; all empty without the key.  cnl_multi shards
 * inherit it.  Measured: DESIGN section 3.2.
 *
 * bit 50 = cnl_newton_system_f32* / cnl_factorize_f32* / cnl_solve_f32* of a Float32 general handle run the general kernel's SUBTREE
 * instances in float stage by stage (tuning "float32_subtrees=1"); bit 49 keeps its Float64-only meaning.
 *
 * Tuning "float32_subtrees" (0 default, 1): "general_subtrees" for a Float32 general handle.  Rules, all answered before a device is
 * looked for: only together with "float32_general=1" (alone: CNL_ERR_ARG); any value other than 0 / 1 is CNL_ERR_ARG; together with
 * "float32_refine" it is CNL_ERR_ARG at cnl_create_ex and at cnl_plan_create_ex (no refined handle over a subtree Float32 factor), as
 * "float32_blocked" is.  A Float64 creator without "float32_refine" reads nothing of the key, neither its value nor its rules.
 * "general_subtrees" and "general_blocked" themselves stay refused at the Float32 creators.  With the key the forced analysis of the
 * handle cuts the tree ("task_cap" as above; the classic tables are those of the key-off plan, bit for bit) and lays the task regions
 * out with the staging rows of the handle (16 with "float32_blocked=1", else 2); gwork and every offset count 4-byte elements.  The
 * key selects no route.  It acts where the Newton / factorise launch is the general kernel in float — the uncondensed handle, the
 * "float32_condense" one, a "float32_register_front" handle that fell back to it — with one problem per workgroup of 256 threads
 * (there is no 1 024-thread float instance), the first stage holds at least two tasks and batch x gwork x 4 <= 8e9 bytes.  Band,
 * register-front, staged / latency, "float32_dense" and "float32_general_dense" handles, 64 threads per problem and single-task cuts
 * are the handles they are without the key and report bit 50 clear.  Launches per call as in Float64 (2 S + 2, S + 1, 2 S), the float
 * condensation passes around them unchanged; the handle keeps the success flags of its last factorisation whether or not it is
 * blocked, and cnl_solve_f32* leaves the rows of d of a failed problem untouched.  It combines with "float32_blocked" (the intended
 * pairing).  Decisions are those of the handle without the key.  Measured: DESIGN section 9.11.
 *
 * bits 51 .. 57 = R, the rungs of the rho ladder a subtree handle (bit 49 or bit 50 set) enqueues behind the first attempt of
 * cnl_newton_system* (tuning "subtree_ladder=R"); 0 on every other handle, whatever the key said.
 *
 * Tuning "subtree_ladder" (0 default, 0 .. 64): a subtree handle of either element type climbs the rho ladder stage by stage.  Rules,
 * all answered before a device is looked for, at the creators and at cnl_plan_create_ex: a value outside 0 .. 64 is CNL_ERR_ARG; so is
 * the key without a subtree key, at a Float64 creator (cnl_create_ex, cnl_multi_create_ex) without "general_subtrees=1", at a
 * Float32 creator (cnl_create_f32*) without "float32_subtrees=1", and together with "float32_refine".  The key selects no route and
 * changes no plan: it acts exactly where the subtree key of the handle acts, and a handle on which that key does not act is the one
 * without either key, allocation for allocation.  With R > 0 cnl_newton_system* enqueues, behind the S forward launches and the decide
 * of the first attempt, R RUNGS: the S forward launches again — a workgroup (task, problem) leaves at once if its problem is done,
 * else assembles and eliminates its task at the problem's rho_k — and one rung-decide launch, one thread per problem, which applies
 * the inertia rule, sets nfact = k + 1 and either finishes the problem (success: rho = rho_k, rho_old = rho_k only if rho_k <= rhomax;
 * or the ladder is exhausted: rho = the first value above rhomax, which is never tried, rho_old unchanged) or forms rho_{k+1} by the
 * reference's recurrence, in the handle's element type.  rho_1 is tried whatever its relation to rhomax, as the reference does.  Then
 * the S backward launches of every problem that holds a factor, one commit launch (the last rho tried into the rho slots of vals of
 * the problems that finished inside the rungs) and the climbers' launch, which skips every problem that is done and RESUMES a problem
 * still climbing after R rungs at rho_{R+1} with nfact = R + 1 — it does not repeat the attempts already made.  (R + 2) S + R + 3
 * launches, all counted in the general-kernel slot of cnl_launch_counts and bracketed by the events of a timed call; the order on
 * the stream is the only dependency (no spin wait, no device counter, no atomic, no host synchronisation in a _dev call).  The host
 * never reads how many rungs a batch needs: rungs beyond every problem's ladder are empty launches, so R = 64 is harmless on any
 * parameters.  cnl_factorize* and cnl_solve* are untouched (S + 1, 2 S).  Every output — success, nfact, rho, rho_old, the rho slots
 * of vals, d of the successes; rows of d of the failures untouched — is that of the same handle with R = 0, bit for bit in both element
 * types.  The ladder state (a done flag and two rho values per problem) is written by the first decide of every call; sub-batch views
 * and cnl_set_active_batch move and shorten it with every per-problem array.  cnl_multi shards inherit the key.  Measured: DESIGN
 * section 3.3.
 *
 * bit 58 = at least one stage of a subtree handle runs its factorising forward launch with 1 024 threads per workgroup at the created
 * batch (tuning "subtree_wide"); bit 59 = at least one stage runs it on the LPAN instance, dependent pivot panels in LDS (tuning
 * "subtree_lds_panels").  Both clear on every handle on which the key does not act.
 *
 * Tuning "subtree_wide" (W, 0 default = off, 1 .. 4096) and "subtree_lds_panels" (M, 0 default = off, 16 .. 4096) shape the
 * FACTORISING FORWARD launch of each stage of a subtree handle of either element type: phase 0 of cnl_newton_system* and
 * cnl_factorize*, and the rung launches of "subtree_ladder".  Rules, all answered before a device is looked for, at the creators
 * and at cnl_plan_create_ex: a value out of range is CNL_ERR_ARG; so is either key without the creator's own subtree key
 * ("general_subtrees=1" at cnl_create_ex / cnl_multi_create_ex, "float32_subtrees=1" at cnl_create_f32*), either key together with
 * "float32_refine", and "subtree_lds_panels" without the creator's own blocked key ("general_blocked=1", "float32_blocked=1").
 * Neither changes a plan, a layout, a route or the number of launches.  With F_s = the largest "gtasks" staging stride (word 7) of
 * the tasks of stage s:
 *   "subtree_wide=W" acts on a subtree handle with 256 threads per workgroup (cfg[0] == 256): stage s factorises with 1 024 threads
 *   where F_s >= W and tasks_s x batch <= 2 x the device's CU count, batch being the launch's own (the active prefix, a sub-batch
 *   view).  The backward stages, every launch of cnl_solve*, the climbers and the decide / commit kernels keep 256.  In float these
 *   are the only 1 024-thread instances of the general kernel: "v1_tpp=1024" at a Float32 creator stays CNL_ERR_ARG.
 *   "subtree_lds_panels=M" acts on a subtree handle that is blocked (bit 47 / 48): stage s runs the LPAN instance where F_s <= M, the
 *   stage has a front of at least 16 pivots and (16 + 32 F_s) elements fit the device's LDS per workgroup (at most 160 KB); the launch
 *   requests that much dynamic LDS.  A dependent pivot panel's rows are copied to LDS, eliminated there by the statements of the
 *   global-memory loop in their order, handed to the matrix-core trailing update from there and written back.
 * Both combine.  The operations on every element of a front and their order are unchanged, so every output is that of the handle
 * without the keys, bit for bit.  cnl_subtree_stage_shape (below) returns the table the launch loop reads.  Measured: DESIGN section 3.4.
 *
 * bits 60 / 61 = the mask of tuning "subtree_solve_panels" on a subtree handle; both clear on every handle that is no subtree handle.
 *
 * Tuning "subtree_solve_panels" (P, a bit mask 0 .. 3, default 0 = off) runs the SOLVE SWEEPS of a subtree handle of either element
 * type — blocked or not, 256 threads per workgroup or a 1 024-thread Float64 handle — in panels of 16 pivots, on kernel entries of
 * their own with the front's vector in dynamic LDS and the stored panel read in place:
 *   bit 0: the backward stage launches of cnl_newton_system* and cnl_solve* (with "subtree_ladder" those behind the rungs).  Per
 *   panel the part of the 16 rows outside the panel is 16 dot products on lane groups, reduced by cross-lane shuffles, and the
 *   panel's triangle is solved by one wavefront: two workgroup barriers per panel.  The order of summation differs from the
 *   unpanelled sweep's: d agrees with P = 0 to rounding, and is a fixed function of the front (no atomic, nothing that depends on
 *   the batch, the grid, the active prefix or on what LDS held);
 *   bit 1: the forward stage launches of cnl_solve*.  Every element receives the operations of the unpanelled loop in their order:
 *   every output is that of P = 0, bit for bit.
 * A stage whose (round4(F_s) + 288) elements exceed the device's LDS per workgroup (at most 160 KB) keeps the unpanelled launch.
 * The factorising forward launches, the rungs, the decide / commit kernels and the climbers are untouched: a problem that climbs keeps
 * the unpanelled sweep.  No plan, route, layout, allocation or launch count changes.  Rules, answered before a device is looked for:
 * a value outside 0 .. 3, the key without the creator's own subtree key, or together with "float32_refine", is CNL_ERR_ARG.
 * Measured: DESIGN section 3.5. */
int cnl_get_config(const cnl_handle* h, int64_t cfg[8]);
/* The factorising forward launch of every stage of a subtree handle (bit 49 or 50 of cnl_get_config [5]) at the handle's current
 * active batch: tpp[s] = threads per workgroup, lds_bytes[s] = dynamic LDS bytes (16 elements without LDS panels), *nstages = S.
 * tpp and lds_bytes hold S entries each, or are null: the count alone.  A handle that is no subtree handle: CNL_ERR_ARG. */
int cnl_subtree_stage_shape(const cnl_handle* h, int32_t* tpp, int32_t* lds_bytes, int64_t* nstages);
/* (bit 38 = a refined handle — tuning "float32_refine", below —, bits 39-41 = its refinement steps k; every other word and bit
 *  describes its inner Float32 handle, with bit 27 clear: the handle is a Float64 handle.) */
/* ([5] + (1 << 27) on a Float32 handle.  On the band kernels: bits 7-26 as above, cfg[0..4], [6], [7] are 0.  On the general kernel
 *  (tuning "float32_general=1"): cfg[0..4] describe that kernel's float instance as they do for a Float64 handle — [2] counts 4-byte
 *  elements — and [5] = 1 + (1 << 27) with bit 6 clear (+ 128 as above; + (1 << 35) where tuning "float32_condense=1" has the
 *  resident condense kernel form the condensed system); [6], [7] are 0.  With tuning "float32_register_front=1" where the
 *  register-front kernel's float instance serves the handle: [5] = 2 + (1 << 27) (+ (1 << 35) as above), [6], [7] = its wavefronts
 *  per workgroup and LDS bytes per workgroup; + bits 36 / 37 as above with tuning "float32_direct_records=1".) */
/* Launches of the Newton-system kernels since the library was loaded, per kernel family: counts[0] band kernels (csrc/band.hip),
 * [1] register-front kernel (csrc/kernels2.hip, staged launches not included), [2] general kernel (csrc/kernels.hip).  Lets a test
 * pin WHICH kernel served a call sequence (e.g. that solve_ldl! behind a band factorisation launches no second kernel family). */
int cnl_launch_counts(int64_t counts[3]);

/* ---- Float32 (LDLFactorization{Float32}, ParamCaNNOLeS(Float32)) on the band kernels ------------------------------------
 * A Float32 handle stores values, rhs, d, rho, rho_old and the factor records as float and computes in float (fmaf, float
 * compares, the inertia test against eig_tol = eps(Float32)): what the reference computes with T = Float32
 * (src/solver_types.jl:79-98, src/CaNNOLeS.jl:1008-1052).  It serves the plugin surface — try_to_factorize, solve_ldl!,
 * newton_system! — in host-pointer and `_dev` forms, in either cnl_options.batch_layout, always on the band kernels (any batch,
 * 1 included), and the device-resident passes around it (rows f1 / f2 / f4 and the trial point, `_f32_dev` below).
 * cnl_create_f32 / cnl_create_f32_ex take the arguments of cnl_create / cnl_create_ex and fail with CNL_ERR_ARG
 * (cnl_last_error names the reason) when the pattern is not a band or cnl_options.band_kernel = 0: the caller stays on the CPU.
 * Accepted: the band patterns of cnl_options.band_kernel, the pattern of a constrained model included (H_c with the model's whole
 * Hessian structure: the wide form of the band program, csrc/band.h) — half-widths up to 2, one live multiplier at a time.
 *   tuning "float32_general=1" (default 0: everything above, unchanged): where the band kernels do not serve the handle — the
 * pattern is no such band, the program does not fit them, or cnl_options.band_kernel = 0 — it runs on the general multifrontal
 * kernel (csrc/kernels.hip) instantiated for float, whatever the pattern, as ONE launch per call (cnl_launch_counts: family 2).  Its
 * plan is the throughput analysis without condensation, register-front records, dense routes or staged execution, whatever the other
 * options say.  Such a handle keeps a real factor: cnl_solve_f32 / cnl_solve_f32_dev are the two sweeps on the stored panels, no
 * refactorisation, and — unlike a band handle, whose solve factorises the values of the last factorisation again — the caller's
 * d_vals need not stay alive (or unchanged) between cnl_factorize_f32_dev and cnl_solve_f32_dev.  cnl_set_active_batch serves it.
 * batch_layout = CNL_LAYOUT_INTERLEAVED on it is CNL_ERR_ARG (the layout is the band kernels'; the conversions cnl_interleave_f32_dev /
 * cnl_deinterleave_f32_dev work on any Float32 handle).  Tuning v1_tpp / v1_ppb / v1_lds may name only a configuration compiled
 * for float (csrc/kernels.hip, CNL_F32_CASES; CNL_ERR_ARG otherwise); a work area that fits neither LDS nor a global-scratch
 * instance is CNL_ERR_DIM, cnl_last_error naming the order of the largest front.
 *   tuning "float32_condense=1" (default 0; takes effect only where "float32_general=1" lets the general kernel serve the handle —
 * every other handle ignores it, and without "float32_general" a non-band pattern is still CNL_ERR_ARG): that plan WITH static
 * condensation of the residual block.  The -I block is eliminated by the condensation passes (csrc/kernels_aux.hip) instantiated
 * for float — every load, product, correctly rounded quotient, sum and compare a float operation, a slot's contributions summed
 * in list order — and the general kernel factorises the system of order nvar + ncon: a call is condense -> ONE launch of family 2
 * -> post-pass (the passes are not counted by cnl_launch_counts, as for Float64).  cnl_plan_info / cnl_get_plan: ncond > 0.
 * cnl_set_active_batch serves it; batch_layout = CNL_LAYOUT_INTERLEAVED stays CNL_ERR_ARG.  ("float32_condense=2": the same with
 * the list-driven condense kernels only, never the resident one — for measurements and tests; bit-equal results.)
 *   CONTRACT of cnl_solve_f32 / cnl_solve_f32_dev on such a handle: the `vals` / d_vals given to cnl_factorize_f32 /
 * cnl_factorize_f32_dev (or cnl_newton_system_f32*) must stay alive and UNMODIFIED until the last solve on that factor — the
 * condensation of every new right-hand side and the post-pass read the Jacobian values and the -I entries from it (host-pointer
 * calls: the handle's own staged copy, nothing for the caller to keep).  The uncondensed Float32 general handle does not need
 * this.  The kept factor still serves any number of right-hand sides without refactorising.
 *   tuning "float32_register_front=1" (default 0; takes effect only where "float32_general=1" lets a general handle serve the
 * pattern — a band handle ignores it, and without "float32_general" a non-band pattern is still CNL_ERR_ARG): implies
 * "float32_condense", and cnl_newton_system_f32* / cnl_factorize_f32* run ONE launch of the register-front kernel
 * (csrc/kernels2.hip) instantiated for float between the float condensation passes (cnl_launch_counts: family 1, none of family
 * 2); cnl_solve_f32* is one launch of the general kernel's float instance (family 2) on the panels the register-front kernel
 * stored.  The plan is the throughput analysis of the condensed system with register-front records that are never direct, whatever
 * the other options say.  Every operation is a float operation (correctly rounded quotients, subnormals kept).  Where a front
 * exceeds order 64, or the kernel's LDS block or 32-bit offsets do not fit, the handle is exactly the "float32_condense=1"
 * handle.  cnl_set_active_batch serves it; batch_layout = CNL_LAYOUT_INTERLEAVED stays CNL_ERR_ARG.  The CONTRACT above holds
 * unchanged: `vals` / d_vals of the factorisation stay alive and unmodified until the last solve on that factor.
 *   tuning "float32_direct_records=1" (default 0; takes effect only with "float32_general=1" AND "float32_register_front=1" — every
 * other handle ignores it): the same forced plan with DIRECT records, i.e. the Direct route of the Float64 default handle in float
 * (cnl_get_config bit 36).  The register-front kernel's float instance forms the condensation products itself from the caller's
 * vals / rhs and writes the kept components of d itself: cnl_newton_system_f32* is ONE launch of family 1 and the post-pass,
 * cnl_factorize_f32* that launch alone.  Where every front is of the fast class (order <= 16; bit 37) cnl_solve_f32* is one launch
 * of family 1 and the post-pass as well; with fronts of class 32 / 64 it stays the condensation of the right-hand side, one
 * launch of family 2 and the post-pass.  The plan is never shaped for a lean or solve-only instance (none exists for float).
 * Direct and condensed handles sum the condensation products in different orders: decisions agree, d agrees within the Float32
 * tolerances, not bit for bit.  Where the analysis cannot write direct records (a fast front with more than 128 raw values, a
 * front with more than 1 023 — patterns with a dense Jacobian block), or the larger LDS block of the direct records does not fit,
 * the handle is exactly the "float32_register_front=1" handle (bit 36 clear), and where even that does not apply the
 * "float32_condense=1" handle.  cnl_set_active_batch serves it; batch_layout = CNL_LAYOUT_INTERLEAVED stays CNL_ERR_ARG.
 *   tuning "float32_dense=1" (default 0; only with "float32_general=1" — "float32_dense=1" without it is CNL_ERR_ARG, and the message
 * names both keys): a pattern whose residual block is DENSE — every residual row holds one entry per variable plus its diagonal,
 * what the dense backend of a Float64 handle takes — gets a Float32 handle on that backend in float, at any batch size:
 * cnl_get_config reports cfg[5] & 7 == 3 with bit 27 set.  J'WJ and the trailing updates run on the f32 matrix instructions, the
 * rho ladder is decided on the device (rho, rho_old and the rho slots are the Float64 ladder's values on the float inputs, rounded
 * to float); cnl_newton_system_f32 / cnl_factorize_f32 / cnl_solve_f32 are the device entries behind an upload.  Every other
 * pattern (band, irregular, half-widths 3 - 4), and every pattern with cnl_options.dense_backend = 0, gets exactly the handle it
 * gets without the key.  As on every dense handle cnl_set_active_batch is CNL_ERR_STATE; skip_done / only_if_status calls and a
 * Newton call without rhs are CNL_ERR_STATE as on every Float32 general handle; batch_layout = CNL_LAYOUT_INTERLEAVED stays
 * CNL_ERR_ARG.  The handle keeps its own factor: the CONTRACT below does not bind it.
 *   tuning "float32_general_dense=1" (default 0; only with "float32_general=1" — without it the call is CNL_ERR_ARG, and the message
 * names both keys; implies "float32_condense"): an IRREGULAR pattern whose fill makes a front of the condensed throughput plan
 * larger than order 64 — what the register-front kernel refuses — runs as ONE dense matrix on the general form of the dense backend
 * in float, as a Float64 default handle's does in double: the float condensation passes around a dense LDL' of the whole condensed
 * system in 64 x 64 tiles on the f32 matrix instructions, the rho ladder decided on the device.  Taken where the pattern has no band
 * program, "float32_dense" did not take it, the condensed order is 96 .. 4096, and batch <= 16 or 3 x 16 384 x ceil(order / 64)^2 x
 * batch <= 8e9 bytes (the Float64 handle's rule with 4-byte elements); "=2" takes it whatever the fronts (measurement, tests).  Every
 * other pattern gets exactly the handle it gets without the key ("float32_condense=1", or the register-front kernel where
 * "float32_register_front=1" serves the plan).  cnl_get_config reports cfg[5] & 7 == 3 with bit 27 set; a condensed plan
 * (cnl_plan_info: ncond > 0) tells it from the "float32_dense" handle.  cnl_set_active_batch, skip_done / only_if_status calls and
 * a Newton call without rhs are CNL_ERR_STATE, batch_layout = CNL_LAYOUT_INTERLEAVED stays CNL_ERR_ARG, the host-pointer entries are
 * the device entries behind an upload.  The solve condenses each new right-hand side from the factorisation's vals: the CONTRACT
 * below binds this handle.  Measured standing (README): opt-in.
 *   tuning "float32_staged=1" (default 0; only with "float32_general=1" — without it the call is CNL_ERR_ARG and the message names
 * the key; values other than 0 and 1, and the key together with "float32_refine", are CNL_ERR_ARG too, at cnl_plan_create_ex,
 * cnl_create_ex, cnl_create_f32_ex and cnl_multi_create_ex alike; implies "float32_register_front", "float32_direct_records" and
 * "float32_condense"): STAGED execution of latency plans in float.  Where a Float64 handle would be planned for latency —
 * plan_kind = CNL_PLAN_LATENCY, or CNL_PLAN_AUTO with 1 <= batch <= staged_max_batch — the analysis is the latency analysis (bushy
 * order, elimination tree cut into tasks) with direct records, never shaped for a lean instance, without split or tail plans, and
 * the handle runs cnl_newton_system_f32* / cnl_factorize_f32* stage by stage on the staged float instances of the register-front
 * kernel: ONE launch per stage and phase (no dataflow execution, no in-kernel ladder, no host-driven ladder: nothing waits on a
 * device counter), the inertia rule on the counts the tasks sum.  The problems that fail the first attempt of cnl_newton_system_f32*
 * (rare) climb the rho ladder from its first rung in ONE classic launch of the float register-front kernel behind the stages, which
 * walks the latency plan's fronts sequentially (cnl_launch_counts: family 1 counts that launch alone, as on a staged Float64
 * handle; family 2 nothing).  cnl_get_config reports cfg[5] & 15 == 4 with bits 27 and 36 set.  cnl_solve_f32* runs staged too
 * where every front is of the fast class (bit 37); with fronts of class 32 / 64 it is the condensation of the right-hand side, one
 * launch of family 2 and the post-pass, as on the "float32_direct_records" handle.  The host-pointer calls are the device entries
 * behind an upload.  Staged and unstaged handles sum in different orders: decisions agree, d agrees within the Float32 tolerances.
 * "float32_dense" and "float32_general_dense" keep the patterns they serve, and a band pattern goes to the band kernels first
 * (cnl_options.band_kernel = 0 brings it here).  Everywhere else — a batch planned for throughput, a plan without tasks, a latency
 * order whose direct records the analysis refuses, an LDS block or 32-bit offsets that do not fit — the handle is EXACTLY the
 * handle the same options give with "float32_register_front=1, float32_direct_records=1" in place of the key.  As every staged
 * handle it refuses cnl_set_active_batch (CNL_ERR_STATE); batch_layout = CNL_LAYOUT_INTERLEAVED stays CNL_ERR_ARG.  The CONTRACT
 * below binds it.  Measured standing (README): opt-in.
 *   tuning "float32_latency=1" (default 0; only with "float32_general=1" — without it the call is CNL_ERR_ARG and the message names
 * the key; values other than 0 and 1, and the key together with "float32_refine", are CNL_ERR_ARG too, at cnl_plan_create_ex,
 * cnl_create_ex, cnl_create_f32_ex and cnl_multi_create_ex alike; implies "float32_staged" and what that implies): the LATENCY PATH
 * of a Float64 handle in float.  The handle is the "float32_staged" handle, and its latency plan honours the switches a Float64
 * handle honours, with their Float64 defaults and rules: lean_kernel and rows_in_backward (the analysis gives every front the row
 * form where that makes the plan lean, cuts fronts with more than 16 residual rows and writes backward rows: the lean float
 * instances, no post-pass behind a call), cnl_options.dataflow, dataflow_waves and dataflow_spin_limit (one launch per phase in which
 * tasks wait for each other on device counters; a wait that gives up is counted — cnl_dataflow_timeouts — and the call is redone
 * sequentially), cnl_options.device_ladder and device_ladder_fused (the problems that fail the first attempt climb the rho ladder of
 * ParamCaNNOLeS(Float32), in float, inside fused launches; rho_old and the rho slots of vals are committed by the launch behind
 * them).  cnl_get_config reports which of them run: bit 4 (lean), and for staged handles of either element type bit 42 (dataflow
 * counters present) and bits 43 .. 44 (the in-kernel ladder: 0 none, 1 behind a staged first attempt, 2 the first attempt inside
 * the fused launch too).  With every one of them switched off the handle is the "float32_staged" handle, bit for bit; dataflow and
 * the ladder do not change a bit of any result.  cnl_launch_counts: family 1 counts the one launch behind the attempt (commit, redo
 * or the sequential ladder), also for cnl_factorize_f32* / cnl_solve_f32* where dataflow counters are present.  The fallbacks, the
 * refusals (cnl_set_active_batch: CNL_ERR_STATE; CNL_LAYOUT_INTERLEAVED: CNL_ERR_ARG) and the CONTRACT are those of
 * "float32_staged", and every fallback is EXACTLY the handle without either key.  Measured standing (README):
 * faster than "float32_staged" for the smallest batches and for batches with ladder climbers, no gain from 256 problems on, slower
 * than the Float64 default handle for cnl_newton_system_f32* everywhere: opt-in.
 *   CONTRACT (the Direct handles' contract, restated): the `vals` / d_vals given to cnl_factorize_f32* (or
 * cnl_newton_system_f32*) must stay alive and UNMODIFIED until the last cnl_solve_f32* on that factor — the solve reads the
 * Jacobian values and the residual pivots of the factorisation's vals (host-pointer calls: the handle's own staged copy).
 * The semantics of every call are those of its Float64 twin above.  Mixing element types is CNL_ERR_STATE and does nothing:
 * a Float64 entry point on a Float32 handle (cnl_factorize..., the row f1 / f2 / f4 / trial-point passes, cnl_interleave_dev...)
 * and an `_f32` entry point on a Float64 handle.  cnl_layout_len counts elements, so it serves both types.
 *   cnl_default_params_f32: ParamCaNNOLeS(Float32), src/CaNNOLeS.jl:48-62, in the order of cnl_default_params.       */
void cnl_default_params_f32(float params[9]);

/* ---- Float64 handles on a Float32 factor: tuning "float32_refine=k" (k = 1 .. 4; default 0; only with "float32_general=1") ----
 * Read by cnl_create_ex and cnl_plan_create_ex.  cnl_create_ex then returns a FLOAT64 handle — every Float64 entry point takes it,
 * every _f32 entry point refuses it (CNL_ERR_STATE) — that owns an inner Float32 general handle, made as cnl_create_f32_ex makes it
 * from the same options with band_kernel forced to 0: "float32_condense", "float32_register_front", "float32_direct_records",
 * "float32_dense" and "float32_general_dense" choose the inner route as they do there.  cnl_get_plan returns the inner handle's plan.
 * A call demotes its inputs to float (a value beyond FLT_MAX becomes inf, and the Float32 factorisation then reports success = 0 for
 * that problem), runs the inner handle's call — the rho ladder, nfact and success are the Float32 handle's; rho and rho_old come back
 * widened, and the rho tail of the caller's Float64 vals receives the widened rho where the ladder wrote it —, and then corrects d
 * k times:  g = rhs + K d  in Float64 (cnl_kkt_residual_dev's kernel, g written as float),  e = the inner solve of g,  d += e.
 * Everything is enqueued on the caller's stream; nothing is read back.  d is written where success != 0 only.
 *   The one deliberate deviation in decisions from a Float64 handle: eig_tol of the inner factorisation is
 * max((float)eig_tol, eps(Float32)) — a pivot below Float32 rounding is noise in a Float32 factor.
 *   CONTRACT: cnl_solve* refines against the vals of the last factorisation: the d_vals given to cnl_factorize_dev /
 * cnl_newton_system_dev must stay alive and unmodified until the last cnl_solve_dev on that factor (host-pointer calls: the handle's
 * own staged copy).
 *   Refused, CNL_ERR_ARG: the key without "float32_general=1"; k outside 0 .. 4; the key at cnl_create_f32_ex or cnl_multi_create_ex;
 * batch_layout = CNL_LAYOUT_INTERLEAVED.  The host-pointer entry points are the device entries behind an upload (no pipelined, pinned
 * or host-ladder route).  Measured standing: README, DESIGN section 9.7 — opt-in.
 *   cnl_get_refine_norms: norms[b * k + j] = max_i |rhs + K d_j|_i in front of correction j of the handle's last cnl_newton_system* or
 * cnl_solve* call (d_0: the raw Float32 solution; [created batch][k] doubles), -1 for a problem without a factor; *steps = k.
 * Synchronises the device, as cnl_dataflow_timeouts does.  A system too ill-conditioned for a Float32 factor shows here as norms
 * that do not fall.  CNL_ERR_STATE on a handle without the key, and before the first such call. */
int cnl_get_refine_norms(cnl_handle* h, double* norms, int64_t* steps);

int cnl_create_f32(cnl_handle** h, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1,
                   int64_t nvar, int64_t nequ, int64_t ncon, int64_t batch, int device);
int cnl_create_f32_ex(cnl_handle** h, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1,
                      int64_t nvar, int64_t nequ, int64_t ncon, int64_t batch, int device, const cnl_options* opt);
int cnl_factorize_f32(cnl_handle* h, const float* vals, float eig_tol, int32_t* success, int64_t* npos, int64_t* nzero);
int cnl_solve_f32(cnl_handle* h, const float* rhs, float* d);
int cnl_newton_system_f32(cnl_handle* h, float* vals, const float* rhs, float* d, const float* rho_old,
                          const float params[9], float* rho, float* rho_old_out, int32_t* nfact, int32_t* success);
int cnl_factorize_f32_dev(cnl_handle* h, const float* d_vals, float eig_tol, int32_t* d_success, void* stream);
int cnl_solve_f32_dev(cnl_handle* h, const float* d_rhs, float* d_d, void* stream);
int cnl_newton_system_f32_dev(cnl_handle* h, float* d_vals, const float* d_rhs, float* d_d, float* d_rho_old,
                              float* d_rho, int32_t* d_nfact, int32_t* d_success, const float params[9], void* stream);
int cnl_interleave_f32_dev(cnl_handle* h, int which, const float* d_src, float* d_dst, void* stream);
int cnl_deinterleave_f32_dev(cnl_handle* h, int which, const float* d_src, float* d_dst, void* stream);

/* Rows f1 / f2 / f4 and the trial point on a Float32 handle: the arguments of the Float64 twins with double replaced by float
 * (norms: float [batch][2]; atol, rtol, max_dlambda: float), the same layout rules (prepare writes `vals` interleaved on a
 * CNL_LAYOUT_INTERLEAVED handle; the `vals`-reading f1 / f4 calls refuse such a handle: use the `_jac` twins), all arithmetic in
 * float as the reference's with T = Float32 — f1 and Jx'r with per-column COO-order sums, multiply and add rounded separately;
 * CGLS (Krylov.jl with T = Float32; defaults sqrt(eps(Float32))).  One deviation: the trial point sums the squares of dlambda in
 * double and rounds ||dlambda||_2 to float once (squares of |dlambda| >= 1.8e19 overflow float; BLAS snrm2 scales and does not).
 *   cnl_prepare_newton_system_f32_dev  src/CaNNOLeS.jl:947-981
 *   cnl_residual_vectors_f32_dev, cnl_residual_vectors_jac_f32_dev  :507-508, :519-524, :528-529, :722-726, :730-731, :631-632
 *   cnl_cgls_multipliers_f32_dev, cnl_cgls_multipliers_jac_f32_dev  :507-518, :880-882
 *   cnl_trial_point_f32_dev            :654, :661-668                                                                         */
int cnl_prepare_newton_system_f32_dev(cnl_handle* h, int64_t nnzhF, int64_t nnzhc, int64_t nnzjF, int64_t nnzjc, const float* d_hF,
                                      const float* d_hc, const float* d_Jx, const float* d_Jcx, const float* d_delta, float* d_vals,
                                      void* stream);
int cnl_residual_vectors_f32_dev(cnl_handle* h, const float* d_vals, const float* d_r, const float* d_lambda, const float* d_Fx,
                                 const float* d_cx, float* d_rhs, float* d_norms, void* stream);
int cnl_residual_vectors_jac_f32_dev(cnl_handle* h, int64_t nnzjF, int64_t nnzjc, const float* d_Jx, const float* d_Jcx, const float* d_r,
                                     const float* d_lambda, const float* d_Fx, const float* d_cx, float* d_rhs, float* d_norms, void* stream);
int cnl_cgls_multipliers_f32_dev(cnl_handle* h, const float* d_vals, const float* d_r, float* d_lambda, float* d_Jxtr, float atol,
                                 float rtol, int64_t itmax, int ones_if_zero, int32_t* d_iters, void* stream);
int cnl_cgls_multipliers_jac_f32_dev(cnl_handle* h, int64_t nnzjF, int64_t nnzjc, const float* d_Jx, const float* d_Jcx, const float* d_r,
                                     float* d_lambda, float* d_Jxtr, float atol, float rtol, int64_t itmax, int ones_if_zero,
                                     int32_t* d_iters, void* stream);
int cnl_trial_point_f32_dev(cnl_handle* h, const float* d_x, const float* d_r, const float* d_lambda, const float* d_d,
                            float max_dlambda, float* d_xt, float* d_rt, float* d_lambdat, float* d_dlambda, void* stream);

/* ---- bookkeeping of the batched outer / inner loop for T = Float32 (row f3; `solve!` is generic in T) --------------------------
 * The nine entry points of the Float64 section (cnl_outer_begin_dev ... cnl_outer_end_dev) on a Float32 state: `cnl_outer_state_f32`
 * has the members of `cnl_outer_state` in the same order, float* where that has double* and float for dmin, rhomax, delta_dec, smax,
 * gammaA, eps2; the integer and mask arrays keep their types.  Same semantics, status codes, flags and argument rules (CNL_ERR_ARG
 * for a null state, B <= 0 or a missing array, with nothing launched).  The C side cannot tell a Float64 array from a Float32 one:
 * handing a state of the other element type over is the caller's error.  With a Float32 handle's `_f32_dev` passes around them
 * (above) they run the whole lockstep loop in Float32 (cannoles.jl_amd/device_loop.py, dtype = float32).
 * Arithmetic: every decision and update is in float, each operation rounded separately and every literal rounded to float first,
 * as the reference's T(0.99), T(1e3), T(100.0) (src/CaNNOLeS.jl:532, 623, 659, 664, 736, 750, 760-761, 1106).  Two points differ
 * from a textual float copy of the Float64 kernels:
 *   * T(1e60) (:638, 647) is Inf32, so the `broken` test on the objective is fx >= infinity: a finite fx never breaks a Float32
 *     problem (3e38 does not, inf does);
 *   * the reductions — |Ft|^2, the three sums of the merit function, g'dx, the count of non-finite entries of d, sum |lambda| and
 *     sum c^2 — accumulate in double from the exactly widened float operands and are rounded to float once.  The reference's Float32
 *     dot products have no prescribed order and such a sum is within one rounding of any of them; the decisions do not depend on
 *     the summation order.                                                                                                        */
typedef struct cnl_outer_state_f32 {
  int64_t B, n, m, p, P /* max(p, 1) */, N, nnzjF, nnzjc, max_inner;
  float dmin, rhomax, delta_dec, smax;
  int32_t *status, *it, *flags /* [8] */, *nf_new, *ok_new;
  int64_t *inner, *nfact, *nlin;
  uint8_t *phase0, *act, *need, *brk, *ext, *lsm, *rej, *chk, *done_in, *tired, *small_res;
  float *normdual, *normprimal, *combined, *combined_hat, *delta, *ndh, *nph, *fx, *epsk, *epstol, *epsF, *epsc, *rho_old;
  float *d, *d_new, *ro_tmp, *rho_new;
  float *x, *r, *Fx, *cx, *Jv, *Jcv, *lam, *rhs_cur;
  float *xt, *rt, *Ft, *ct, *Jt, *Jct, *lamt, *rhs_t, *nrm_t /* [B][2] */;
  float *xt_e, *rt_e, *lamt_e;
  float gammaA, eps2;
  float *ls_g, *xl, *Fl, *cl, *lam_ls, *alpha, *Dphi, *phix, *eta;
  int64_t* nbk;
  uint8_t* bt;
} cnl_outer_state_f32;
int cnl_outer_begin_f32_dev(const cnl_outer_state_f32* st, void* stream);
int cnl_outer_newton_done_f32_dev(const cnl_outer_state_f32* st, int did_newton, void* stream);
int cnl_outer_extrapolated_f32_dev(const cnl_outer_state_f32* st, void* stream);
int cnl_outer_trial_done_f32_dev(const cnl_outer_state_f32* st, void* stream);
int cnl_outer_ls_begin_f32_dev(const cnl_outer_state_f32* st, void* stream);
int cnl_outer_ls_test_f32_dev(const cnl_outer_state_f32* st, int first, void* stream);
int cnl_outer_ls_step_f32_dev(const cnl_outer_state_f32* st, void* stream);
int cnl_outer_ls_take_f32_dev(const cnl_outer_state_f32* st, void* stream);
int cnl_outer_end_f32_dev(const cnl_outer_state_f32* st, void* stream);
/* the `_ex` entry points and the mask kernel on a Float32 state; the control block is the same structure */
int cnl_outer_begin_ex_f32_dev(const cnl_outer_state_f32* st, const cnl_outer_ctl* ctl, void* stream);
int cnl_outer_trial_done_ex_f32_dev(const cnl_outer_state_f32* st, const cnl_outer_ctl* ctl, void* stream);
int cnl_outer_ls_test_ex_f32_dev(const cnl_outer_state_f32* st, int first, const cnl_outer_ctl* ctl, void* stream);
int cnl_outer_end_ex_f32_dev(const cnl_outer_state_f32* st, const cnl_outer_ctl* ctl, void* stream);
int cnl_outer_hess_mask_f32_dev(const cnl_outer_state_f32* st, const cnl_outer_ctl* ctl, void* stream);
int cnl_outer_compact_f32_dev(const cnl_outer_state_f32* st, int64_t nextra, void* const* d_extra, const int64_t* extra_row_bytes,
                              int64_t min_finished, int32_t* d_orig, int32_t* d_counts, int32_t* d_work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CANNOLES_HIP_H */
