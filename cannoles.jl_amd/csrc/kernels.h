// kernels.h — launch interface between the C ABI driver (capi_*.cpp) and the HIP kernels.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "plan.h"

namespace cnl {

// device-resident copy of the plan (index data shared by every problem)
struct DevPlan {
  const FrontHdr* fronts;
  const int32_t* seg_ptr;
  const int32_t* asm_pos;
  const int32_t* asm_src;
  const int32_t* child_idx;
  const int32_t* rel_idx;
  const int32_t* perm;
  int32_t nsuper, N, nnz, rho_begin, nvar, nequ, ncon;
  int32_t fmax;
  int32_t pb_off;        // offset (elements: doubles, or floats on a Float32 handle) of the panel buffer inside a problem's work area
  int32_t wv_off;        // offset of the two pivot-row staging vectors (2*fmax elements; tuning general_blocked / float32_blocked: the panel buffer W, 16*fmax)
  int32_t work_doubles;  // work area per problem (elements)
  int64_t lsize;         // factor storage per problem (elements)
  int64_t vstride, rstride, dstride;  // per-problem strides (elements) of vals / rhs / d
};

struct KernelConfig {
  int tpp = 64;          // threads per problem (16, 32, 64, 256, 1024)
  int ppb = 1;           // problems per workgroup
  int lds_work = 1;      // work area in LDS (else global scratch)
  size_t lds_bytes = 0;  // dynamic LDS per workgroup
  int blocked = 0;       // MODE_NEWTON / MODE_FACTOR run the blocked instance (tuning general_blocked, float32_blocked on a Float32 handle; newton_blocked_has)
};

// device-resident v2 plan (record streams, see plan.h / kernels2.hip); elements: doubles, or floats on a Float32 handle
struct DevPlan2 {
  const int32_t* rec;
  const int32_t* brec;
  int32_t nsuper, N, nnz, rho_begin, nvar;
  int32_t N0;            // length of the right-hand side the records address (outer N with direct records)
  int32_t count_d;       // 1: the fronts count the condensed residual pivots they own (no separate inertia pass)
  int32_t reccap;        // words of the forward record buffer (one per wave)
  int32_t breccap;       // words per backward record buffer (two per wave, same LDS area)
  int32_t recwords;      // words of that area = max(reccap, 2 * breccap)
  int32_t u2_peak;       // elements: per-problem LDS update stack; the staging triangle follows it
  int32_t prob_doubles;  // elements of LDS per problem
  int32_t jraw_off;      // elements: offset of the raw-value area of the on-the-fly condensation inside the per-problem LDS
  int32_t bpanel_off;    // elements: offset of the backward sweep's two panel buffers inside the per-problem LDS (behind the x stack)
  int64_t gs_doubles;    // elements of global scratch per problem
  int64_t lsize;
  int64_t vstride, rstride, dstride;  // per-problem strides (elements) of vals / rhs / d
};

// device-resident condensation lists (condense.h)
struct DevCond {
  const int32_t *c_ptr, *c_a, *c_b, *c_d, *c_order;
  const int32_t *ch_slot, *ch_rng, *ch_tile, *rng_start, *rng_len, *c_la, *c_lb, *c_ld, *ch_tptr, *tile_src;  // LDS-tiled condense (condense.h)
  const uint64_t* c_pack;
  int32_t tile_max, chunk_ncon_max, chunk_nslot_max, tiled_ok;
  const int32_t *r_dsrc, *r_ptr, *r_jsrc, *r_jx;
  const int32_t *red_of, *cidx_of, *orig_of, *r_orig;
  int32_t N, nnz, nvar, N2, ncs, ncond;
  int64_t cstride;
};

// The contribution lists once more, for the resident condense kernel of the Float32 general handles (kernels_aux.hip,
// condense_resident_kernel): slots in blocks of COND_RES_THREADS, block j holding the k-th contribution of its
// slots side by side at pack[blk_ptr[j] + k * COND_RES_THREADS + t] (one coalesced load per step of a wavefront), as
// a | (b + 1) << 16 | (d + 1) << 32 with a, b, d indices into [vals | rhs] (all below 65 535); a slot's entries past its own count
// (c_ptr) are zero words, read and not used.  A separate structure: DevCond is a kernel argument of the Float64 passes too.
constexpr int COND_RES_THREADS = 1024;
struct DevCondEll {
  const uint64_t* pack;
  const int32_t* blk_ptr;   // [blocks + 1], in entries
  const int32_t* c_ptr;     // DevCond::c_ptr
  int32_t nslot, nnz, N;
  int64_t cstride;
};

// Transposed-Jacobian lists of the KKT pattern: for every variable column j the entries of
// J_F and J_c in COO order, as (slot in vals, index into r resp. lambda).
struct DevJt {
  const int32_t *ptrF, *slotF, *idxF;  // [nvar + 1], [nnz(J_F)] x 2
  const int32_t *ptrC, *slotC, *idxC;  // [nvar + 1], [nnz(J_c)] x 2
  const int32_t *rptrC, *rslotC, *rcolC;  // J_c by rows: [ncon + 1], [nnz(J_c)] x 2 (slot in vals, variable) — CGLS (row f4)
  int32_t nvar, nequ, ncon, N, nnz;
  // (round 5) column tiles of row f1: when the entries of RVT_COLS consecutive columns lie in short slot / index ranges (band
  // and block patterns in COO order do), a workgroup streams those ranges of `vals`, r and lambda coalesced into LDS and forms the
  // column sums from there (residual_vectors_tiled_kernel).  rv_ntiles == 0: the gather kernel serves the pattern.
  const int32_t* rv_tiles;    // [rv_ntiles][RVT_TW]
  const uint32_t* rv_table;   // [rv_ntiles][RVT_KF + RVT_KC + 1][RVT_COLS]: window offsets of a column's first entries, counts
  int32_t rv_ntiles, rv_lds_doubles, rv_primal_tiles;
};
// where rows f1 / f4 read the Jacobian values: value of slot k (a position in `vals`) of problem b = vF[b * sF + k] for the J_F
// entries, vC[b * sC + k] for the J_c entries.  From `vals` itself: {vals, nnz, vals, nnz}; from the model's arrays Jx / Jcx (what
// prepare_newton_system! copies into those segments, src/CaNNOLeS.jl:968-974): {Jx - first J_F slot, nnz(J_F), Jcx - first J_c slot, nnz(J_c)}
// (JacSrcF: the same for the float arrays of a Float32 handle)
template <class T>
struct JacSrcT {
  const T* vF; long long sF;
  const T* vC; long long sC;
  int safeF, safeC;   // a slot of each kind that exists in every problem (the gather kernel's loads of absent entries; vC is never null)
};
typedef JacSrcT<double> JacSrc;
typedef JacSrcT<float> JacSrcF;
constexpr int RVT_COLS = 256;   // columns per tile: one per thread of a 256-thread workgroup (two per thread: 190 registers)
constexpr int RVT_KF = 6, RVT_KC = 2;   // entries of a column held in the table (the rest of a longer column: index lists)
constexpr int RVT_MAXF = 2046, RVT_MAXR = 510, RVT_MAXC = 510, RVT_MAXL = 510;   // window limits (doubles): 4 + 1 + 1 + 1 chunks of 16 bytes per thread
constexpr int RVT_PROWS = 2048;  // rows per primal tile when the dual tiles cannot own the primal rows
enum { RVT_FSLO = 0, RVT_WF, RVT_RLO, RVT_WR, RVT_CSLO, RVT_WC, RVT_LLO, RVT_WL, RVT_OWNLO, RVT_OWNHI, RVT_TW = 12 };

enum { MODE_NEWTON = 0, MODE_FACTOR = 1, MODE_SOLVE = 2 };

// The element arrays (vals, rhs, d, L, scratch, rho_old, rho) are in the launch's element type: the _f32 launchers read them as float.
struct LaunchArgs {
  int mode;
  int batch;
  void* vals;            // [batch][nnz]   (NEWTON: rho tail written back; FACTOR: read only)
  const void* rhs;       // [batch][N]     (NEWTON, SOLVE)
  int layout;            // band kernels, 32 problems per workgroup: bit 0 = vals, bit 1 = rhs interleaved over the workgroup's problems (band.h: band_il_index)
  void* d;               // [batch][N]     (NEWTON, SOLVE)
  void* L;               // [batch][lsize] factor storage
  void* scratch;         // [batch][work_doubles] when !lds_work
  void* rho_old;         // [batch] in/out (NEWTON)
  void* rho;             // [batch] out    (NEWTON)
  int32_t* nfact;        // [batch] out    (NEWTON)
  int32_t* success;      // [batch] out    (NEWTON: solve_success, FACTOR: success); in (SOLVE on a blocked handle: 0 = no factor, skip)
  int64_t* npos;         // [batch] optional (FACTOR)
  int64_t* nzero;        // [batch] optional (FACTOR)
  double params[9];      // ParamCaNNOLeS; params[0] = eig_tol also for FACTOR (a Float32 launch: the Float32 parameters, widened)
  const int* extra_pos;  // [batch] optional: inertia counts of pivots eliminated outside the kernel (condensed r nodes)
  const int* extra_zer;
  // staged execution (latency plans, kernels2.hip STAGED): one launch per phase when `dep` is given (a task waits for its
  // children resp. its parent on device counters), else one launch per stage and phase
  const int32_t* tasks;  // device: 6 words per task {record offset, fronts, backward record offset, 1 if a root of the forest,
                         //                            parent task or -1, number of child tasks}
  int task0, ntasks;     // tasks of this launch
  int phase;             // 0: forward (assembly + elimination) of the tasks, 1: backward sweep of the tasks
  int nquads;            // groups of four problems
  int* gcnt;             // [batch][2] pivot counts summed over the tasks
  int skip_done;         // classic launch behind a staged attempt: problems with success[b] == 1 are left alone (register-front kernel;
                         //    of the general kernel the subtree instances alone read it: the climbers' launch, launch_newton_subtrees)
  int ntasks_all;        // tasks of the plan (the counters of the backward phase follow those of the forward phase)
  int df_live;           // 1: this launch spans several stages (tasks wait on the counters; signals are released); 0: one stage,
                         //    its dependencies are complete by launch order (no wait, plain counter bump)
  int df_waves;          // the top stages of the tree whose wavefronts together number at most this run as ONE launch per phase
  int* dep;              // [2][tasks][nquads] dataflow counters (zeroed per call): children done (forward), task done (backward)
  // A dataflow wait that gives up after spin_limit polls bumps both counters: status_total is sticky (cnl_dataflow_timeouts),
  // status_call is zeroed with `dep` at the start of every staged call and makes the classic launch behind the staged attempt
  // redo the whole batch sequentially (only_if_status: that launch exits at once when the attempt had no timeout)
  int lean;              // 1: the plan qualifies for the kernels' LEAN instantiation (fast-class fronts, row-form products only)
  int back_rows;         // 1: (lean) the backward records carry the rows sections (plan.h, B_ROWS_FLAG): no post-pass behind the launch
  int* status_total;
  int* status_call;
  int spin_limit;
  int only_if_status;
  // In-kernel rho ladder of staged plans (phase == 2, kernels2.hip): ONE launch in which every task of the elimination tree of a
  // group of four problems has a wavefront of its own; per rung the tasks factorise in dataflow fashion, the last one to finish
  // applies the ladder rule of src/CaNNOLeS.jl:1029-1047 to the group's four problems and publishes the decision, the others
  // wait for it; the backward sweeps of the tasks follow in the same launch.  All wavefronts of a launch must be resident at
  // once (the host sizes lad_slots for that).
  int* lad;              // [nquads][LAD_WORDS] control block per group of four problems (zeroed per call), see kernels2.hip
  int* lgcnt;            // [batch][2] pivot counts of the current rung (zeroed per call, reset by the deciding wavefront)
  int* ldep;             // [2][tasks][nquads] counters of the fused launch: children done (monotone over the rungs), task done (backward)
  int lad_first;         // 1: the launch makes the first attempt too (rho as given); 0: only groups with a problem that failed the
                         //    staged first attempt are processed (the others exit at once)
  int lad_slots;         // groups of problems this launch covers, starting at quad0; wavefront index = task * lad_slots + slot
  int quad0;
  // host side of it (launch_newton2_staged): lad_mode 0 = no in-kernel ladder (the caller's sequential launch takes the failed
  // problems), 1 = the fused launch(es) behind the staged first attempt, 2 = the fused launch makes the first attempt too;
  // lad_capacity = wavefronts of this kernel the device holds at once; lad_zero_ints = ints to zero from gcnt on (gcnt, lgcnt,
  // lad and ldep are one allocation, zeroed with one memset per call)
  int lad_mode, lad_capacity;
  long long lad_zero_ints;
};
constexpr int LAD_WORDS = 32;  // ints per group: [0] tasks that finished the rung, [1] epoch (2 * rung + final), [4..7] state of the
                               // four problems (0 active, 1 factorised, 2 gave up), doubles at [8..15] rho last written to the
                               // slots ("wrote"; 0: never laddered), at [16..23] the rho_old to commit

// device-resident band program (band.h; kernels: band.hip)
struct BandDev {
  const int32_t* fops[2];
  const int32_t* bops[2];
  const int32_t* epochs[2];
  const int32_t* borders[2];
  int32_t nsteps[2], nepochs[2];
  long long loff[2];
  int32_t nparts, m0, n, N, nnz, nvar;
  long long lsize;
};
// newton_system! / try_to_factorize of a.batch problems on the band kernels, nl problems per workgroup (8, 16 or 32); a.L = the
// band factor storage [batch][P.lsize]
// npiece: operand pieces per epoch of the program P was uploaded from (BandPlan::npiece): 15, or 20 = the wide kernel instances
// resident: P is the resident form of the 15-piece program (band.h) — nl = 32, `vals` interleaved (a.layout & 1)
// mover: ... whose epoch blocks carry the mover table in place of the piece descriptors (band.h, BAND_MK_*)
// policy: the cache policy mask of the mover-table instance (tuning band_cache_policy; band.hip, BAND_POL_*): 0, or a mask
// band_policy_built() names, and then with mover only
hipError_t launch_band(const BandDev& P, int nl, const LaunchArgs& a, hipStream_t stream, int npiece = 15, bool resident = false, bool mover = false, int policy = 0);
bool band_policy_built(int policy);   // is there a mover-table instance for this cache policy mask? (0: always)
// the same on Float32 data: P is the 4-byte program (build_band_plan with esz = 4), P.lsize counts floats
hipError_t launch_band_f32(const BandDev& P, int nl, const LaunchArgs& a, hipStream_t stream, int npiece = 15);
bool band_wide_has(int esz, int nl);   // is there a wide (20-piece) instance for this element size and problems per workgroup?
size_t band_lds_bytes(int nparts, int nl, int esz = 8, int npiece = 15);   // esz: bytes per element (8 double, 4 float); npiece: of the program

// returns hipSuccess or the launch error
hipError_t launch_newton(const DevPlan& P, const KernelConfig& cfg, const LaunchArgs& a, hipStream_t stream);
// the same kernel on Float32 data (a Float32 handle off the band kernels, tuning float32_general): every offset, stride and size of
// P counts elements, cfg.lds_bytes = 4 * (16 + ppb * work area).  Only the configurations newton_f32_has() names are compiled for
// float; any other is hipErrorInvalidConfiguration.
hipError_t launch_newton_f32(const DevPlan& P, const KernelConfig& cfg, const LaunchArgs& a, hipStream_t stream);
bool newton_f32_has(int tpp, int ppb, bool lds_work);
bool newton_blocked_has(int tpp, int ppb, bool f32 = false);   // is there a blocked instance (cfg.blocked) of the element type for this configuration?
// Subtree execution of the general kernel (tuning general_subtrees, float32_subtrees on a Float32 handle; DESIGN sections 3.2 and 9.11;
// kernels.hip: newton_subtrees).  f32: the element type of the handle (arrays of a, work area, rho).  One launch of
// a SUB instance: P.fronts = the plan's task-region front table (Plan::gfronts), P.work_doubles = Plan::gwork, a.tasks = the device copy
// of Plan::gtasks (8 words per task), a.scratch the global work area, a.gcnt [tasks][batch][2] the tasks' pivot-count slots;
// a.phase 0: forward (a.mode MODE_NEWTON / MODE_FACTOR: assembly + elimination at rho as given; MODE_SOLVE: the vector sweep) of the
// tasks [a.task0, a.task0 + a.ntasks), one workgroup per (task, problem); a.phase 1: their backward sweep, problems with
// a.success[b] == 0 skipped; a.phase 2: the climbers — one workgroup per problem runs the whole sequential newton_system over the
// a.ntasks_all tasks, and with a.skip_done = 1 (read by these instances alone among the general kernel's) a problem whose
// a.success[b] is already 1 leaves at once.  MODE_SOLVE skips problems whose a.success[b] is 0 in both phases.
// The shape of one factorising forward launch of a stage (a.phase 0, MODE_NEWTON / MODE_FACTOR, and the rungs of the ladder; DESIGN
// section 3.4): threads per workgroup — the handle's, or 1024 on a 256-thread handle (tuning subtree_wide) — and dynamic LDS bytes — the
// 16 elements of psum, or (16 + 32 F_s) elements where the stage eliminates its dependent pivot panels in LDS (tuning subtree_lds_panels,
// the LPAN instances of a blocked handle).  nullptr everywhere below: the handle's shape.
struct SubtreeStageShape {
  int32_t tpp;
  int32_t lds_bytes;
};
hipError_t launch_newton_subtrees(const DevPlan& P, const KernelConfig& cfg, const LaunchArgs& a, hipStream_t stream, bool f32,
                                  const SubtreeStageShape* shape = nullptr);
// The solve sweeps of a subtree handle in panels of PANEL_W = 16 pivots (tuning subtree_solve_panels; kernels.hip:
// subtree_solve_kernel — entries of their own, double at 256 or 1024 threads, float at 256).  One launch of a stage, grid and arguments as
// launch_newton_subtrees': a.phase 1 — the backward sweep; a.phase 0 with MODE_SOLVE — the forward substitution.  Dynamic LDS of a launch
// of a stage whose largest task fmax is F_s, in elements: [the front's vector, round4(F_s) | the panel's triangle, 16 rows of stride 17 |
// the panel's 16 values] — every carve offset a multiple of 4 elements, 16 bytes in float.
constexpr int SOLVE_PANEL_TRI = 16 * 17;
inline int64_t subtree_solve_vec_elems(int64_t fmax_s) { return (fmax_s + 3) & ~(int64_t)3; }
inline int64_t subtree_solve_lds_elems(int64_t fmax_s) { return subtree_solve_vec_elems(fmax_s) + SOLVE_PANEL_TRI + 16; }
// fmax_s: F_s of the stage; lds_bytes = subtree_solve_lds_elems(fmax_s) x the element size
hipError_t launch_subtree_solve(const DevPlan& P, const KernelConfig& cfg, const LaunchArgs& a, hipStream_t stream, bool f32, int fmax_s,
                                size_t lds_bytes);
bool newton_subtrees_has(int tpp, int ppb, bool f32);   // is there a subtree instance of the element type for this configuration?
// behind the last forward stage of a factorising subtree call: success (and a.npos / a.nzero where given) from the slots of gcnt plus
// a.extra_pos / a.extra_zer; MODE_NEWTON: rho = 0, nfact = 1 of the problems that succeeded
hipError_t launch_subtree_decide(const LaunchArgs& a, const int* gcnt, int ntasks, int nvar, hipStream_t stream, bool f32);
// The rho ladder of a subtree handle stage by stage (tuning subtree_ladder = R > 0; kernels.hip: subtree_ladder_kernel).
// The per-problem state of the call under way: done [batch] — 0 climbing, 1 succeeded on the first attempt, 2 finished inside the rungs —,
// rho [batch][2] in the handle's element type — {the rho of the problem's next rung, the last rho tried}; rungs = R.
struct LadderState {
  int32_t* done;
  void* rho;
  int rungs;
};
// a.phase 0: forward of the tasks [a.task0, a.task0 + a.ntasks) of one stage at every climbing problem's rho (rho_override), one workgroup
// per (task, problem), pivot counts into the slots of a.gcnt; a.phase 2: the climbers of the problems still climbing after st.rungs rungs,
// resumed behind them.  MODE_NEWTON only.  Problems that are done are left alone by both.
hipError_t launch_subtree_ladder(const DevPlan& P, const KernelConfig& cfg, const LaunchArgs& a, const LadderState& st, hipStream_t stream, bool f32,
                                 const SubtreeStageShape* shape = nullptr);
// the first decide of such a call (in the place of launch_subtree_decide): its outputs, st.done and rho_1 of every problem
hipError_t launch_subtree_ladder_first(const LaunchArgs& a, const LadderState& st, const int* gcnt, int ntasks, int nvar, hipStream_t stream, bool f32);
// behind the stages of rung k = 1 .. R: inertia rule, nfact = k + 1, success / exhaustion / the next rho of every problem that is not done
hipError_t launch_subtree_rung_decide(const LaunchArgs& a, const LadderState& st, int k, const int* gcnt, int ntasks, int nvar, hipStream_t stream, bool f32);
// behind the backward stages: the last rho tried into the rho slots of a.vals of the problems that finished inside the rungs
hipError_t launch_subtree_ladder_commit(const DevPlan& P, const LaunchArgs& a, const LadderState& st, hipStream_t stream, bool f32);
hipError_t launch_newton2(const DevPlan2& P, int wpb, size_t lds_bytes, const LaunchArgs& a, hipStream_t stream);
// the register-front kernel on Float32 data (a Float32 general handle with tuning float32_register_front): every size of P named
// "doubles" counts floats, lds_bytes is computed with 4-byte elements (the record area stays in 32-bit words).  Direct records with
// tuning float32_direct_records; MODE_SOLVE (direct records, every front of the fast class) runs an instance of its own.  skip_done
// (the launch behind a staged attempt, tuning float32_staged) is served by the plain instances; lean and only_if_status (a handle
// of tuning float32_latency: lean plans, the commit / redo behind dataflow and fused-ladder launches) pick from the same table as
// launch_newton2.
hipError_t launch_newton2_f32(const DevPlan2& P, int wpb, size_t lds_bytes, const LaunchArgs& a, hipStream_t stream);
// one attempt at the rho given in vals, stage by stage (stage_ptr: host array of nstages + 1 task offsets)
// f32: on Float32 data (tuning float32_staged; sizes as for launch_newton2_f32) — the float instances by the same lean / lean-solve /
// late / ladder rules; a handle without tuning float32_latency hands over a.dep = nullptr, a.lad_mode = 0, a.lean = 0: one launch
// per stage
hipError_t launch_newton2_staged(const DevPlan2& P, int wpb, size_t lds_bytes, LaunchArgs a, const int32_t* stage_ptr, int nstages, hipStream_t stream,
                                 bool f32 = false);
hipError_t launch_condense(const DevCond& C, const double* vals, const double* rhs, double* cbuf, int slot_begin, int slot_end,
                           int batch, hipStream_t stream);
// LDS-tiled variant over all chunks; mask: 1 matrix slots, 2 rho slots, 4 right-hand-side slots
hipError_t launch_condense_tiled(const DevCond& C, const double* vals, const double* rhs, double* cbuf, int mask, int nchunks,
                                 int batch, hipStream_t stream);
hipError_t launch_cond_inertia(const DevCond& C, const double* vals, int* extra_pos, int* extra_zer, double eig_tol, int batch,
                               hipStream_t stream);
hipError_t launch_prepare(int nnzhF, int nnzhc, int nnzjF, int nnzjc, int nvar, int nequ, int ncon, const double* hF, const double* hc,
                          const double* Jx, const double* Jcx, const double* delta, double* vals, int batch, int interleaved, hipStream_t stream);
// problem-major <-> interleaved over groups of 32 problems (band.h: band_il_index); rows of `len` doubles
hipError_t launch_interleave(const double* src, double* dst, int batch, int full_batch, long long len, int to_interleaved, hipStream_t stream);
hipError_t launch_interleave_f32(const float* src, float* dst, int batch, int full_batch, long long len, int to_interleaved, hipStream_t stream);
// wide: the instance whose ncon-vectors live in `ws` ([batch][2 nvar + 3 ncon] then; [batch][2 nvar] and ncon <= 1024 otherwise)
hipError_t launch_cgls(const DevJt& J, const JacSrc& S, const double* r, double* lambda, double* Jxtr, double* ws, int32_t* iters,
                       double atol, double rtol, int itmax, int ones_if_zero, bool wide, int batch, hipStream_t stream);
hipError_t launch_residual_vectors(const DevJt& J, const JacSrc& S, const double* r, const double* lambda, const double* Fx,
                                   const double* cx, double* rhs, double* norms, int batch, hipStream_t stream);
hipError_t launch_trial_point(const DevJt& J, const double* x, const double* r, const double* lambda, const double* d,
                              double max_dlambda, double* xt, double* rt, double* lambdat, double* dlambda, int batch,
                              hipStream_t stream);
// float twins of the four launchers above (Float32 handles): the same kernels instantiated for float, the same grid rules
hipError_t launch_prepare(int nnzhF, int nnzhc, int nnzjF, int nnzjc, int nvar, int nequ, int ncon, const float* hF, const float* hc,
                          const float* Jx, const float* Jcx, const float* delta, float* vals, int batch, int interleaved, hipStream_t stream);
hipError_t launch_cgls(const DevJt& J, const JacSrcF& S, const float* r, float* lambda, float* Jxtr, float* ws, int32_t* iters,
                       float atol, float rtol, int itmax, int ones_if_zero, bool wide, int batch, hipStream_t stream);
hipError_t launch_residual_vectors(const DevJt& J, const JacSrcF& S, const float* r, const float* lambda, const float* Fx,
                                   const float* cx, float* rhs, float* norms, int batch, hipStream_t stream);
hipError_t launch_trial_point(const DevJt& J, const float* x, const float* r, const float* lambda, const float* d,
                              float max_dlambda, float* xt, float* rt, float* lambdat, float* dlambda, int batch,
                              hipStream_t stream);
// float twins of the condensation passes (Float32 general handles with tuning float32_condense): the same kernels instantiated for
// float, every operation a float operation, eig_tol narrowed to float
hipError_t launch_condense(const DevCond& C, const float* vals, const float* rhs, float* cbuf, int slot_begin, int slot_end,
                           int batch, hipStream_t stream);
hipError_t launch_condense_tiled(const DevCond& C, const float* vals, const float* rhs, float* cbuf, int mask, int nchunks,
                                 int batch, hipStream_t stream);
// ... and the resident form: one workgroup per problem holds [vals | rhs] in LDS and forms the slots [slot_begin, slot_end)
hipError_t launch_condense_resident(const DevCondEll& E, const float* vals, const float* rhs, float* cbuf, int slot_begin, int slot_end,
                                    int batch, hipStream_t stream);
size_t condense_resident_lds_bytes(int64_t nnz, int64_t N);
hipError_t launch_cond_inertia(const DevCond& C, const float* vals, int* extra_pos, int* extra_zer, float eig_tol, int batch,
                               hipStream_t stream);
hipError_t launch_expand(const DevCond& C, float* vals, const float* rhs, const float* d2, const float* cbuf, float* dout,
                         const int* success, int copy_rho_tail, int batch, hipStream_t stream);
hipError_t launch_fill_rho(double* vals, long long nnz, int nvar, const double* rho, const int* active, int batch, hipStream_t stream);
hipError_t launch_lds_fill(int pattern, hipStream_t stream);   // debugging aid, see kernels_aux.hip
hipError_t launch_expand(const DevCond& C, double* vals, const double* rhs, const double* d2, const double* cbuf, double* dout,
                         const int* success, int copy_rho_tail, int batch, hipStream_t stream);
// largest dynamic LDS a workgroup may use on the current device
size_t max_lds_bytes();
int lds_attr_cap(int need);   // value for hipFuncAttributeMaxDynamicSharedMemorySize: the device's limit (kernels2.hip)

}  // namespace cnl
