// handle.h — what the translation units of the C ABI driver (capi_*.cpp) share: the plan, handle and multi-handle structures, the
// error helpers and the few functions that cross files.  Host side only: no .hip file includes it.
// The per-problem device arrays of a handle are declared ONCE, where they are allocated (dalloc_batch, below): that puts them into
// the handle's table (batch_arrays.h), and the views of a part of the batch (SubBatch) move whatever the table holds.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cannoles_hip.h"
#include "band.h"
#pragma GCC visibility push(hidden)   // (internal to the library, as everything behind the structures below)
#include "batch_arrays.h"
#pragma GCC visibility pop
#include "call_shape.h"
#include "condense.h"
#include "dense.h"
#include "kernels.h"
#include "options.h"
#include "plan.h"
#include "refine.h"

struct cnl_plan {
  cnl::Cond C;   // static condensation of the residual block (outer -> condensed system)
  cnl::Plan P;   // multifrontal plan of the (condensed) system
  int64_t N = 0, nnz = 0, nvar = 0, nequ = 0, ncon = 0;  // outer dimensions, as the reference sees them
  std::vector<int32_t> perm_outer;
  bool latency = false;  // ordered and cut into tasks for small batches (staged execution, csrc/plan.h)
  bool prefer_dense = false;  // latency plan with fronts of the 64 class on a small condensed system: small batches go the dense route
  cnl::DensePlan D;  // dense residual block (BASELINE config 2): served by the dense backend, csrc/dense.h
  std::vector<int32_t> gpos;  // non-empty: the condensed system may be treated as ONE dense matrix (position of every K2 slot)
  cnl::Tuning opt{};          // the switches the plan was built with (options.h; the handle reads its execution switches from here)
  std::atomic<int> refs{1};   // handles of a cnl_multi share one analysis (read-only after creation)
  bool split_mode = false;    // bidirectional-chain plan for a batch between one and two wavefronts per SIMD (capi_run.cpp, run_split)
  // (round 5) band programs of a throughput plan (csrc/band.h), [f32][wide]: for 8-byte (Float64 handles) and 4-byte elements
  // (Float32 handles), each in the 15-piece form and in the WIDE form (band.h: BAND_NPIECE_WIDE operand pieces per epoch), which is
  // built where the pattern needs more than 15 pieces — a constrained model's H_c as wide as H_F — or where tuning band_pieces = 20
  // asks for it.  B.ok == false: the pattern is no band (of that form).  info / pinfo: the summaries cnl_plan_get returns.
  struct BandSlot {
    cnl::BandPlan B;
    std::vector<int32_t> info, pinfo[2];
  };
  BandSlot band_prog[2][2];
  // the RESIDENT form of band_prog[0][0] (band.h: aligned blocks of `vals` that stay in LDS while the next epoch needs them), built
  // beside it unless tuning band_resident = 0; runs the Float64 handles of 32 problems per workgroup with interleaved `vals`
  BandSlot band_res;
  std::vector<int32_t> band_mov_info;   // "bandm_info": summary of band_res.B's mover table (band.h, BAND_MK_*)
  // the validated COO pattern, 0-based, and — built on first request (kkt_rows(), below) — the rows of the full symmetric matrix
  // (refine.h): what cnl_kkt_residual_dev and the refinement of a float32_refine handle gather along; cnl_plan_get "kkt_row_*"
  std::vector<int32_t> pat_rows, pat_cols;
  mutable std::once_flag kkt_once;
  mutable cnl::KktRows kkt;
};

struct cnl_handle {
  cnl_plan* plan = nullptr;
  int device = 0;
  cnl::Route route = cnl::Route::Plain;   // which backend serves the calls (call_shape.h); set once, by finish_handle
  int64_t batch = 1;        // problems a call works on: the created batch, or fewer behind cnl_set_active_batch (the first `batch` problems)
  int64_t full_batch = 1;   // the batch the handle was created with: what every allocation, array address and cnl_layout_len are sized by
  int64_t factor_batch = 0; // problems the last factorisation covered (cnl_solve_dev must not be asked for more)
  std::vector<void*> dev_allocs;
  // The device arrays a kernel indexes by problem, with their bytes per problem (dalloc_batch / register_batch, below): what a SubBatch
  // view moves.  In it: d_L, d_gs, d_scratch, d_cbuf, d_d2, d_xpos, d_xzer, d_gcnt, d_blk_ok, d_sub_cnt, d_Lband, d_lad_done, d_lad_rho.  NOT in it, and never
  // moved: the staging of the host-pointer calls (d_vals, d_rhs, d_d, d_res, d_npos: addressed by b0 explicitly), d_act, cgls_ws, the
  // r_* arrays of a refined handle and dkkt.partial — the calls that use those are not served through views.
  cnl::BatchArrays batch_arrays;
  cnl::DevPlan dp{};
  cnl::KernelConfig cfg{};
  // v2 (register-front kernel): used for newton_system / factorize when every front has order <= 64
  bool use_v2 = false;
  bool staged = false;    // newton_system: first attempt stage by stage (tasks of the elimination tree on different wavefronts)
  const int32_t* d_tasks = nullptr;
  int* d_gcnt = nullptr;
  void* pin = nullptr;    // pinned host block for the results of small host-pointer calls
  size_t pin_bytes = 0;
  int* d_dep = nullptr;   // dataflow counters of the staged execution (nullptr: one launch per stage)
  int* d_status = nullptr;  // [1] dataflow waits that gave up (sticky; kernels2.hip spin_until)
  // counters of a staged call, ONE allocation behind d_gcnt, zeroed with one memset per call:
  // [gcnt 2B | lgcnt 2B | lad LAD_WORDS * nquads | ldep 2 * tasks * nquads | stat 2 | dep 2 * tasks * nquads (dataflow only)]
  int *d_lgcnt = nullptr, *d_lad = nullptr, *d_ldep = nullptr, *d_stat = nullptr;
  long long zero_ints = 0;
  int resident_waves = 0;   // wavefronts of the register-front kernel the device holds at once
  int lad_mode = 0;         // in-kernel rho ladder of staged newton_system calls (kernels.h): 0 none, 1 behind the staged attempt, 2 fused
  int ntasks = 0;
  int df_waves = 1024;
  std::vector<int32_t> stage_ptr;
  bool v2_solve = false;  // cnl_solve runs on the register-front kernel too (direct records, every front of the fast class)
  int* d_act = nullptr;   // [batch] problems whose rho slots the host ladder rewrites
  bool lean = false;      // every front of the fast class with row-form (or no) products: the kernels' LEAN instantiation serves it
  cnl::DevPlan2 dp2{};
  int wpb2 = 1;
  size_t lds2 = 0;
  void* d_gs = nullptr;   // global scratch of the register-front kernel, in the handle's element type (as d_cbuf, d_d2, d_L, d_scratch)
  // condensation state
  cnl::DevCond dc{};
  void* d_cbuf = nullptr;   // [batch][cstride]
  void* d_d2 = nullptr;     // [batch][N2]
  int *d_xpos = nullptr, *d_xzer = nullptr;
  // tuning general_blocked (a Float32 handle: float32_blocked), where the general kernel's blocked instances serve the handle
  // (cnl_get_config bit 47, in float bit 48; capi_handle.cpp: alloc_blocked_flags): the success flags of
  // the last factorisation of every problem, copied behind each Newton / factorise launch; solve_ldl! leaves the rows of d of a
  // problem without a factor untouched (the blocked instance and the expand pass read them)
  int32_t* d_blk_ok = nullptr;
  // tuning general_subtrees, on a Float32 general handle float32_subtrees, where it acts (capi_handle.cpp: setup_subtrees; cnl_get_config
  // bit 49, in float bit 50; DESIGN sections 3.2 and 9.11; sizes in elements of the handle's type): the three calls
  // run the general kernel's subtree instances stage by stage.  dp.fronts is then the plan's task-region front table and
  // dp.work_doubles its gwork — the work area is d_scratch, global, whatever the configuration said —, d_gtasks the task records,
  // gstage_ptr the plan's stage pointers, d_sub_cnt [tasks][batch][2] the tasks' pivot counts of the call under way (views of the
  // handle use disjoint pieces of it).  Such a handle keeps d_blk_ok whether or not its instances are blocked.
  bool subtrees = false;
  const int32_t* d_gtasks = nullptr;
  int* d_sub_cnt = nullptr;
  std::vector<int32_t> gstage_ptr;
  // tuning subtree_ladder = R > 0 on such a handle (cnl_get_config bits 51 .. 57): newton_system enqueues R rungs of
  // the rho ladder behind the first attempt, stage by stage.  The state of the call under way (kernels.h: LadderState), written by the
  // first decide of every call: d_lad_done [batch], d_lad_rho [batch][2] in the handle's element type.  0: the sequence without the key.
  int ladder_rungs = 0;
  int32_t* d_lad_done = nullptr;
  void* d_lad_rho = nullptr;
  // tuning subtree_wide / subtree_lds_panels on such a handle (cnl_get_config bits 58 / 59): the per-stage table of the
  // factorising forward launches, built once by setup_subtrees and read by subtree_stage_shape() — which the launch loop and
  // cnl_subtree_stage_shape both call.  gstage_fmax[s] = F_s, the largest GTask::fmax of stage s; sub_wide = W where the key acts (the
  // handle has 256 threads per workgroup), else 0; sub_cus the device's CU count; gstage_lpan[s] = the dynamic LDS bytes of stage s's LPAN
  // launch, 0 where the stage runs without LDS panels (every stage of a handle without the key, or one that is not blocked).
  int32_t sub_wide = 0;
  int32_t sub_cus = 0;
  std::vector<int32_t> gstage_fmax, gstage_lpan;
  // tuning subtree_solve_panels = P on such a handle (cnl_get_config bits 60 / 61): solve_panels = P (bit 0: the backward
  // stage launches, bit 1: the forward stage launches of solve_ldl! run subtree_solve_kernel), 0 on every other handle and where no stage fits; gstage_solve_lds[s] =
  // the dynamic LDS bytes of such a launch of stage s, (round4(F_s) + 288) elements, 0 where that exceeds the device's LDS per workgroup
  // (the stage then keeps the unpanelled launch).
  int32_t solve_panels = 0;
  std::vector<int32_t> gstage_solve_lds;
  // Float32 general handles on a condensed plan: the resident condense kernel serves the handle (kernels.h: DevCondEll) — where the
  // tiled kernel's chunks degenerate (dense Jacobians) and [vals | rhs] of a problem fits LDS; tuning float32_condense = 2: never
  bool cond_resident = false;
  cnl::DevCondEll dce{};
  const void* last_vals = nullptr;  // device vals of the last factorisation (needed to condense later right-hand sides)
  void* d_L = nullptr;
  void* d_scratch = nullptr;
  // staging for the host-pointer API, in the handle's element type (capi_calls.cpp: ensure_staging, stage<T>): vals, rhs, d, the
  // per-problem results as one block [rho | rho_old | nfact | success] (nfact / success: int32), and [npos | nzero]
  void *d_vals = nullptr, *d_rhs = nullptr, *d_d = nullptr, *d_res = nullptr;
  int64_t* d_npos = nullptr;
  hipStream_t stream = nullptr;
  int64_t split_staged = 0;   // > 0: problems [0, split_staged) run staged, the rest single-stream, concurrently (run_split)
  bool split_halves = false;  // ... or (round 4): the rest runs staged as well, BEHIND the first part on the same stream (two halves)
  // (round 4) a batch a little above what fills the machine on the bidirectional chain (staged_max_batch < batch <= 5/4 of it):
  // problems [0, split_staged) run on this handle's chain plan, the REMAINDER on a handle of its own with the many-part latency
  // plan cnl_create picks for that small batch, one behind the other on the caller's stream (run_split)
  cnl_handle* tail = nullptr;
  bool tail_fresh = false;    // the factors of the remainder live in the tail handle (false: in this handle's storage — chunked host calls)
  hipStream_t aux_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  static constexpr int kPipeUp = 2;  // host threads that upload chunks of a host-pointer call (each on its own stream)
  hipStream_t pipe_stream[kPipeUp + 1] = {};  // chunked host-pointer calls: the uploaders' compute streams, one more for the results
  std::vector<hipEvent_t> pipe_ev;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timing = false;
  float last_ms = 0.f;
  bool factorized = false;
  // success flags of the last HOST-pointer factorisation (cnl_factorize / cnl_newton_system), for cnl_solve: the reference never
  // solves after a failed factorisation (src/CaNNOLeS.jl:1049) — a one-problem cnl_solve then is a call-sequence error, and a
  // batched one leaves the rows of the failed problems untouched.  Unknown (empty) after a device-pointer factorisation.
  std::vector<char> last_ok;
  cnl::DevJt djt{};  // transposed-Jacobian lists (row f1: residual / optimality vectors on the device)
  cnl::DenseState* dense = nullptr;
  cnl::DenseState* gdense = nullptr;  // dense treatment of an arbitrary condensed system (irregular sparsity, small batch)
  cnl::GeneralOps gops{};
  void* cgls_ws = nullptr;    // [batch][2 * nvar] elements ([batch][2 * nvar + 3 * ncon] where the wide instance runs, tuning cgls_wide): workspace of cnl_cgls_multipliers_dev / _f32_dev, allocated on first use
  // (round 5) band kernels (csrc/band.h): newton_system of a throughput handle whose pattern is a band
  bool band = false;
  cnl::BandDev bd{};
  int band_nl = 16;            // problems per workgroup
  int band_npiece = 15;        // operand pieces per epoch of the program in bd: 15, or 20 = the wide kernel instances
  bool band_mover = false;     // ... with the piece descriptors of its epoch blocks replaced by the mover table: the mover-table instance runs it
  int band_policy = 0;         // ... under this cache policy mask (tuning band_cache_policy; 0 wherever another instance runs the handle)
  bool band_resident = false;  // bd holds the plan's resident program (cnl_plan::band_res): the resident kernel instance runs it
  bool jac_segments = false;   // the J_F and the J_c entries are one run of slots each: [jf_lo, jf_lo + jf_n), [jc_lo, jc_lo + jc_n)
  int64_t jf_lo = 0, jf_n = 0, jc_lo = 0, jc_n = 0;
  int layout = 0;              // band handles: bit 0 = vals (cnl_options.batch_layout), bit 1 = rhs interleaved over groups of 32 problems (band.h)
  void* d_Lband = nullptr;     // [batch + 32][bd.lsize] factor records of the band kernels, in the handle's element type
  // Float32 handle (cnl_create_f32): the band kernels on float data, bd = the 4-byte program, and the row lists of rows f1 / f4 (djt,
  // jac_segments); nothing else of the handle's device state exists, and every Float64 entry point refuses it (CNL_ERR_STATE).
  // last_vals holds its float array of the last factorisation (the band solve factorises those values again).
  bool f32 = false;
  // ... off the band kernels (tuning float32_general = 1 where the band kernels do not serve the handle): the general multifrontal
  // kernel instantiated for float.  The plan is the throughput analysis without condensation (C.active == false), so every call is
  // the one classic launch; the handle owns dp, cfg, the row lists and FLOAT factor panels / global scratch behind d_L / d_scratch
  // (element counts as for double: dp.lsize and dp.work_doubles count elements).  It keeps a real factor: the solve is two sweeps.
  // With tuning float32_condense = 1 the plan is that analysis WITH condensation (C.active): the handle also owns dc, d_xpos / d_xzer
  // and FLOAT arrays behind d_cbuf / d_d2, and a call is condense -> the one classic launch on d_cbuf -> expand, all in float.
  // With tuning float32_register_front = 1 that plan also has register-front records (never direct) and setup_v2 may set use_v2:
  // dp2, wpb2 / lds2 and a FLOAT global scratch behind d_gs (every "doubles" of dp2 counts floats); newton_system / factorize then
  // launch the register-front kernel's float instantiation, the solve stays on the general kernel (v2_solve, lean, staged: false).
  // With tuning float32_direct_records = 1 on top those records are direct (where the analysis can write them and setup_v2 takes
  // them): route Direct, v2_solve by the Float64 rule (lean, staged: still false); d_cbuf / d_d2 and the condensation lists stay,
  // for the solve on plans with class-32 / class-64 fronts.
  // With tuning float32_staged = 1 on top of that, a batch planned for latency has a latency plan on direct records, and where
  // setup_v2 stages it the handle owns d_tasks, stage_ptr and the counters block (gcnt, lgcnt, lad, ldep, status words — no dataflow
  // counters): staged = true, lad_mode = 0, d_dep = nullptr, lean = false.  A call is one launch per stage of the staged float
  // instances and, for newton_system, the classic float launch behind them (skip_done) for the problems that failed the attempt.
  // With tuning float32_latency = 1 on top of that the staged state is a Float64 handle's: d_dep where
  // cnl_options.dataflow, lad_mode by the ladder rule, lean (and then no post-pass) by the Float64 conditions of setup_v2.
  // With tuning float32_dense = 1 a pattern with a dense residual block (plan->D) is the uncondensed handle plus `dense`, a FLOAT
  // state of the dense backend (csrc/dense_f32.hip): route Dense, every call runs there (run_dense dispatches on f32).
  // With tuning float32_general_dense a condensed plan with a front above order 64 (2: any) whose condensed order is 96 .. 4096 is
  // the float32_condense handle plus `gdense`, a FLOAT state of the general form, and gops: route GeneralDense, a call is the float
  // condensation passes around the dense LDL^T of the condensed system (execute dispatches on f32).
  bool f32_general = false;
  // the rows of the full KKT matrix on the device (refine.h), uploaded on first use: cnl_kkt_residual_dev, refined calls
  cnl::DevKktRows dkkt{};
  // Tuning float32_refine = k (cnl_create_ex): a Float64 handle (f32 == false) that owns an INNER Float32 general handle — made by the
  // code behind cnl_create_f32_ex from the caller's options, band_kernel forced to 0 — and shares its plan.  Of the device state above
  // it has the row lists (djt, dkkt) and the staging of the host-pointer calls alone; run() hands every call to run_refined
  // (capi_run.cpp): demote -> the inner handle's call -> widen -> k times [residual in Float64 -> inner solve -> update].
  // last_vals is the caller's FLOAT64 array of the last factorisation: the residual of a later solve_ldl! reads it.
  cnl_handle* inner = nullptr;
  int refine_k = 0;
  float *r_vals = nullptr, *r_rhs = nullptr, *r_e = nullptr;   // [batch][nnz], [batch][N] (right-hand side, then every residual), [batch][N] (d32, then every correction)
  float *r_rho = nullptr, *r_rho_old = nullptr;                // [batch]
  int32_t* r_success = nullptr;                                // [batch] flags of the last factorisation: the mask of every refinement kernel
  double* r_norms = nullptr;                                   // [batch][k] (cnl_get_refine_norms)
  bool r_norms_valid = false;                                  // a NEWTON or SOLVE call has written r_norms
  size_t esz() const { return f32 ? sizeof(float) : sizeof(double); }   // bytes per element of every element array of the handle
};

struct cnl_multi {
  std::vector<cnl_handle*> h;
  std::vector<int64_t> start, count;
  std::vector<int> device;
  int64_t N = 0, nnz = 0, batch = 0;
  // one persistent host thread per shard (created with the handle, bound to the shard's device once): the host-pointer
  // calls hand each of them a job and wait; no thread is created or joined per call
  std::vector<std::thread> workers;
  std::mutex mu;
  std::condition_variable cv_job, cv_done;
  std::function<int(size_t)> job;
  uint64_t generation = 0;
  size_t pending = 0;
  bool stop = false;
  std::vector<int> rc;
  std::vector<std::string> msg;
};

// Everything below is internal to the library: hidden from its dynamic symbol table, which holds the C ABI alone.
#pragma GCC visibility push(hidden)

extern thread_local std::string g_err;   // the text cnl_last_error returns (defined in capi_plan.cpp)

inline int fail(int code, const std::string& m) {
  g_err = m;
  return code;
}

// element type of a handle against that of the entry point: mixing them is a call-sequence error, refused before anything runs
inline int need_f64(const cnl_handle* h, const char* fn) {
  if (h && h->f32) return fail(CNL_ERR_STATE, std::string(fn) + ": this is a Float32 handle (cnl_create_f32); it takes the _f32 entry points only");
  return CNL_OK;
}
inline int need_f32(const cnl_handle* h, const char* fn) {
  if (h && !h->f32) return fail(CNL_ERR_STATE, std::string(fn) + ": this is a Float64 handle; the _f32 entry points need one made by cnl_create_f32");
  return CNL_OK;
}
// host-pointer entry points take the arrays of the created batch: refused while cnl_set_active_batch holds the handle below it
inline int need_full_batch(const cnl_handle* h, const char* fn) {
  if (h && h->batch < h->full_batch)
    return fail(CNL_ERR_STATE, std::string(fn) + ": the handle works on its first " + std::to_string(h->batch) + " of " + std::to_string(h->full_batch) +
                                   " problems (cnl_set_active_batch); host-pointer calls need the whole batch");
  return CNL_OK;
}
#define CNL_NEED_FULL_BATCH(h) do { if (int rc_ = need_full_batch((h), __func__)) return rc_; } while (0)
#define CNL_NEED_F64(h) do { if (int rc_ = need_f64((h), __func__)) return rc_; } while (0)
#define CNL_NEED_F32(h) do { if (int rc_ = need_f32((h), __func__)) return rc_; } while (0)

#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return fail(CNL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// p + n elements of the handle's element type (an absent array stays absent): the one place that does arithmetic on an untyped
// element array
inline const void* elem_offset(const cnl_handle* h, const void* p, int64_t n) { return p ? static_cast<const char*>(p) + n * (int64_t)h->esz() : nullptr; }
inline void* elem_offset(const cnl_handle* h, void* p, int64_t n) { return const_cast<void*>(elem_offset(h, static_cast<const void*>(p), n)); }
// An element array of a Float64 handle, typed, for the routes only Float64 handles have (the dense backends).  To be called behind the
// point where a Float32 handle has been refused (run(): f32_general_serves); one that gets here all the same is a bug, and aborts.
inline double* f64(const cnl_handle* h, void* p) {
  if (h->f32) { fprintf(stderr, "cannoles_hip: a Float64-only route was reached on a Float32 handle\n"); abort(); }
  return static_cast<double*>(p);
}
inline const double* f64(const cnl_handle* h, const void* p) { return f64(h, const_cast<void*>(p)); }

template <class T>
int upload(cnl_handle* h, const std::vector<T>& v, const T** out) {
  void* p = nullptr;
  size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
  HIPCHK(hipMalloc(&p, bytes));
  h->dev_allocs.push_back(p);
  if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = (const T*)p;
  return CNL_OK;
}

template <class T>
int dalloc(cnl_handle* h, T** out, size_t count) {
  void* p = nullptr;
  static const size_t G = getenv("CNL_DBG_GUARD") ? (size_t)atol(getenv("CNL_DBG_GUARD")) : 0;   // debugging aid: NaN-filled guard zones
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  HIPCHK(hipMalloc(&p, bytes + 2 * G));
  if (G) HIPCHK(hipMemset(p, getenv("CNL_DBG_GUARD_PAT") ? atoi(getenv("CNL_DBG_GUARD_PAT")) : 0xFF, bytes + 2 * G));
  h->dev_allocs.push_back(p);
  *out = (T*)(static_cast<char*>(p) + G);
  if (G && getenv("CNL_DBG_GUARD_LOG")) fprintf(stderr, "[dalloc] #%zu %p + %zu bytes\n", h->dev_allocs.size(), (void*)*out, bytes);
  return CNL_OK;
}
// count elements of the handle's element type
inline int dalloc_elems(cnl_handle* h, void** out, size_t count) {
  char* p = nullptr;
  const int rc = dalloc(h, &p, count * h->esz());
  *out = p;
  return rc;
}

// A per-problem device array (batch_arrays.h): put into the handle's table, where the views of a part of the batch find it
template <class T>
int register_batch(cnl_handle* h, T** slot, size_t bytes_per_problem) {
  if (!h->batch_arrays.add(reinterpret_cast<void**>(slot), (int64_t)bytes_per_problem))
    return fail(CNL_ERR_STATE, "per-problem array registered twice, with no bytes per problem, or beyond the table's capacity (batch_arrays.h)");
  return CNL_OK;
}
// ... allocated and registered in one: `per_problem` items for each problem of the CREATED batch and `pad` more behind the last one.
// The one way to give a handle an array that a kernel indexes by problem; what is allocated otherwise is not served through views.
template <class T>
int dalloc_batch(cnl_handle* h, T** out, size_t per_problem, size_t pad = 0) {
  if (int rc = dalloc(h, out, (size_t)h->full_batch * per_problem + pad)) return rc;
  return register_batch(h, out, per_problem * sizeof(T));
}
// ... counted in elements of the handle's element type
inline int dalloc_batch(cnl_handle* h, void** out, size_t per_problem, size_t pad = 0) {
  if (int rc = dalloc_elems(h, out, (size_t)h->full_batch * per_problem + pad)) return rc;
  return register_batch(h, out, per_problem * h->esz());
}

// ---- capi_plan.cpp ----
int resolve_options(const cnl_options* in, cnl::Tuning& out);
int plan_create_tuned(cnl_plan** plan, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar, int64_t nequ,
                      int64_t ncon, int64_t batch, const cnl::Tuning& o);
int plan_create_impl(cnl_plan** plan, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar, int64_t nequ,
                     int64_t ncon, int latency, int par, double slots, const cnl::Tuning& o);
void build_band_programs(cnl_plan* p, const int64_t* rows1, const int64_t* cols1, int esz);
void band_summaries(cnl_plan* p);
const cnl::BandPlan& band_program(const cnl_plan* plan, bool f32);

const cnl::KktRows& kkt_rows(const cnl_plan* plan);   // built on first request
// the plan of a Float32 general handle off the band kernels (what cnl_create_f32_ex analyses behind tuning float32_general): the
// uncondensed throughput analysis, or what float32_condense / _register_front / _direct_records / _dense / _general_dense make of it.
// batch: read with tuning float32_staged alone — the latency analysis on direct records where a Float64 handle of that batch would
// be planned for latency and the plan can run staged, else the plan of f32_unstaged_options(o)
int f32_general_plan(cnl_plan** plan, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar, int64_t nequ, int64_t ncon,
                     const cnl::Tuning& o, cnl::Tuning* used = nullptr, int64_t batch = 0);
// tuning float32_staged taken out of `o`, the keys it implies written out: the options of the handle "without the key"
cnl::Tuning f32_unstaged_options(const cnl::Tuning& o);
// tuning float32_general_dense: do the tiles of `batch` problems of this plan fit the general form of the dense backend in float?
bool f32_general_dense_fits(const cnl_plan* plan, int64_t batch);
// what every creator checks of the float32_* keys (fn: the creator's name, for the message)
int check_f32_options(const cnl::Tuning& o, const char* fn);
// tuning general_blocked or general_subtrees on a creator of Float32 state (cnl_create_f32*, the inner handle of float32_refine): CNL_ERR_ARG
int check_no_general_blocked(const cnl::Tuning& o, const char* fn);
// tuning subtree_ladder at a creator whose own subtree key (f32: float32_subtrees, else general_subtrees) is off: CNL_ERR_ARG
// (and tuning subtree_wide / subtree_lds_panels at such a creator, or subtree_lds_panels without the creator's own blocked key)
int check_subtree_ladder(const cnl::Tuning& o, bool f32, const char* fn);

// ---- capi_handle.cpp ----
int ensure_kkt_rows(cnl_handle* h);   // h->dkkt on the device
int create_from_plan(cnl_handle** hout, cnl_plan* plan, const int64_t* rows1, const int64_t* cols1, int64_t batch, int device);
// a subtree handle: the shape of the factorising forward launch of stage s at a launch of `batch` problems —
// 1024 threads where tuning subtree_wide acts, F_s >= W and tasks_s x batch <= 2 x CUs; the LPAN bytes where the stage has them
cnl::SubtreeStageShape subtree_stage_shape(const cnl_handle* h, int s, int64_t batch);

// ---- capi_run.cpp ----
// what holds for ONE call of run() and is no state of the handle
struct RunOpts {
  bool first_attempt_only = false;  // newton_system on a staged handle: no sequential launch behind the staged attempt (the host ladder follows)
  bool part_of_split = false;       // the call is one part of a split batch (run_split): it is not split again
};
int run(cnl_handle* h, cnl::LaunchArgs& a, void* d_vals, const void* d_rhs, void* d_d, hipStream_t stream, RunOpts o = {});
int kkt_residual(cnl_handle* h, const double* d_vals, const double* d_rhs, const double* d_d, double* d_g, double* d_norms, hipStream_t stream);

// no timing (cnl_set_timing) of the launches enqueued while this lives: they are part of a call that is timed as a whole, or not at all
struct TimingOff {
  cnl_handle* h; const bool was;
  explicit TimingOff(cnl_handle* h_) : h(h_), was(h_->timing) { h->timing = false; }
  ~TimingOff() { h->timing = was; }
};

// run() on problems [b0, b0 + nb) of the handle: every array of the handle's table (batch_arrays) is moved to problem b0 and the
// batch set to nb for the lifetime of the view (b0 a multiple of 4: a wavefront serves four problems); last_vals — the caller's array,
// nnz elements per problem — moves with them.  Views nest: one opened inside another counts b0 from the outer one's first problem.
// Dataflow counters are per handle, not per view: views run one launch per stage (d_dep, d_lad, d_stat: null); !allow_staged: classic.
struct SubBatch {
  cnl_handle* h;
  cnl::BatchView arrays;
  int64_t batch;
  const void* last_vals;
  bool staged;
  int *dep, *lad, *stat;
  SubBatch(cnl_handle* h_, int64_t b0, int64_t nb, bool allow_staged = true);
  ~SubBatch();
};

#pragma GCC visibility pop
