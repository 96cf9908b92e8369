// capi_run.cpp — the launch logic: run() hands one call on device-resident data to the handle's backend (band kernels, dense routes,
// register-front / general multifrontal kernels with their condensation passes, staged execution) or, for a split batch, to views
// of the handle and its remainder handle (SubBatch, run_split).  Everything is enqueued on the caller's stream.
#include "handle.h"

static_assert(cnl::CALL_NEWTON == cnl::MODE_NEWTON && cnl::CALL_FACTOR == cnl::MODE_FACTOR && cnl::CALL_SOLVE == cnl::MODE_SOLVE, "call_shape.h: modes");

namespace {

// debugging aid (include/cannoles_hip.h): CNL_DBG_LDSFILL=<byte pattern> — kernels that leave the pattern in LDS, scratch and registers
// run in front of every launch.  The variable is read ONCE per process (round 6: it was a getenv per launch in the product build).
const int* dbg_ldsfill() {
  static const int pat = [] { const char* e = getenv("CNL_DBG_LDSFILL"); return e ? (int)strtol(e, nullptr, 0) : -1; }();
  static const bool on = getenv("CNL_DBG_LDSFILL") != nullptr;
  return on ? &pat : nullptr;
}

// launches per kernel family since the library was loaded (cnl_launch_counts): [band kernels, register-front kernel, general kernel]
std::atomic<long long> g_launches[3];

// the time between the handle's two events (cnl_set_timing), once the second one has been recorded
int read_timing(cnl_handle* h) {
  HIPCHK(hipEventSynchronize(h->ev1));
  HIPCHK(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
  return CNL_OK;
}
// closes the timed region behind the last launch of a call (cnl_set_timing) and reads it
int end_timed(cnl_handle* h, hipStream_t stream) {
  if (!h->timing) return CNL_OK;
  HIPCHK(hipEventRecord(h->ev1, stream));
  return read_timing(h);
}

// what every launch of a call begins with: the debug fill, and the fields of the arguments that come from the handle alone
void begin_launch(const cnl_handle* h, cnl::LaunchArgs& a, hipStream_t stream) {
  if (const int* pat = dbg_ldsfill()) (void)cnl::launch_lds_fill(*pat, stream);
  a.batch = (int)h->batch;
  a.lean = h->lean ? 1 : 0;
  a.back_rows = (h->lean && h->plan->P.back_rows) ? 1 : 0;
}

// the per-problem result arrays of a call, from problem b0 on
cnl::LaunchArgs shifted(const cnl_handle* h, cnl::LaunchArgs a, int64_t b0) {
  a.rho_old = elem_offset(h, a.rho_old, b0);
  a.rho = elem_offset(h, a.rho, b0);
  if (a.nfact) a.nfact += b0;
  if (a.success) a.success += b0;
  if (a.npos) a.npos += b0;
  if (a.nzero) a.nzero += b0;
  return a;
}

// A call of the plugin surface on a band handle, either element type: exactly one launch of the band kernels.  try_to_factorize is
// the forward sweep alone;
// solve_ldl! factorises the values of the last factorisation again (rho slots as the ladder left them) and sweeps the new
// right-hand side in the same launch — the band kernels' six-element records hold z = c / d of the one right-hand side they were
// computed with, so there is no stored factor a second right-hand side could use.
int run_band(cnl_handle* h, cnl::LaunchArgs& a, void* d_vals, const void* d_rhs, void* d_d, hipStream_t stream) {
  // (a band handle owns the band factor records alone: the buffers of the other kernels do not exist for it)
  if (a.skip_done || a.only_if_status || (a.mode == cnl::MODE_NEWTON && !d_rhs))
    return fail(CNL_ERR_STATE, "this call is not served by the band kernels, and a band handle has no other"
                               " (no factor panels, no condensed buffer; interleaved `vals` are the band kernels' layout)");
  begin_launch(h, a, stream);
  a.vals = a.mode == cnl::MODE_SOLVE ? const_cast<void*>(h->last_vals) : d_vals;
  a.rhs = d_rhs; a.d = d_d;
  a.L = h->d_Lband;
  a.layout = h->layout;
  if (h->timing) HIPCHK(hipEventRecord(h->ev0, stream));
  const hipError_t e = h->f32 ? cnl::launch_band_f32(h->bd, h->band_nl, a, stream, h->band_npiece)
                              : cnl::launch_band(h->bd, h->band_nl, a, stream, h->band_npiece, h->band_resident, h->band_mover, h->band_policy);
  g_launches[0]++;
  if (e != hipSuccess)
    return fail(CNL_ERR_HIP, std::string("band kernel launch (") + (h->f32 ? "Float32, " : "") + std::to_string(h->band_nl) +
                                 " problems per workgroup): " + hipGetErrorString(e));
  return end_timed(h, stream);
}

// a Float32 handle off the band kernels: the float instantiation of the general kernel serves the three calls of the plugin
// surface as one classic launch each (on a condensed plan between the float condensation passes), and nothing else; with tuning
// float32_register_front the launch of newton_system / try_to_factorize is the register-front kernel's float instantiation
// (launch(), below).  rhs: the right-hand side the call was given
int f32_general_serves(const cnl_handle* h, const cnl::LaunchArgs& a, const void* rhs) {
  if (h->f32 && (a.skip_done || a.only_if_status || (a.mode == cnl::MODE_NEWTON && !rhs) || !h->f32_general))
    return fail(CNL_ERR_STATE, "this call is not served by the Float32 instantiation of the general kernel, and the handle has no other");
  return CNL_OK;
}

// one classic launch of the register-front or the general kernel (run() sends no band or dense handle here)
int launch(cnl_handle* h, cnl::LaunchArgs& a, hipStream_t stream) {
  begin_launch(h, a, stream);
  a.L = h->d_L;
  a.scratch = h->d_scratch;
  hipError_t e;
  if (h->timing) HIPCHK(hipEventRecord(h->ev0, stream));  // events bracket the multifrontal kernel only
  if (h->use_v2 && (a.mode != cnl::MODE_SOLVE || h->v2_solve)) {
    a.scratch = h->d_gs;
    e = h->f32 ? cnl::launch_newton2_f32(h->dp2, h->wpb2, h->lds2, a, stream) : cnl::launch_newton2(h->dp2, h->wpb2, h->lds2, a, stream);
    g_launches[1]++;
  } else {
    if (h->d_blk_ok && a.mode == cnl::MODE_SOLVE) a.success = h->d_blk_ok;   // (a blocked handle: problems without a factor are skipped)
    e = h->f32 ? cnl::launch_newton_f32(h->dp, h->cfg, a, stream) : cnl::launch_newton(h->dp, h->cfg, a, stream);
    g_launches[2]++;
    if (h->d_blk_ok && a.mode != cnl::MODE_SOLVE && a.success && e == hipSuccess)   // ... which these flags say, from here on
      e = hipMemcpyAsync(h->d_blk_ok, a.success, (size_t)h->batch * sizeof(int32_t), hipMemcpyDeviceToDevice, stream);
  }
  if (e != hipSuccess)
    return fail(CNL_ERR_HIP, std::string("kernel launch (tpp=") + std::to_string(h->cfg.tpp) + " ppb=" + std::to_string(h->cfg.ppb) +
                                 " lds=" + std::to_string(h->cfg.lds_work) + "): " + hipGetErrorString(e));
  if (h->timing) HIPCHK(hipEventRecord(h->ev1, stream));
  return CNL_OK;
}

// one staged pass over the tasks of a latency plan (first attempt of newton_system, try_to_factorize, or solve_ldl!)
// ladder_ran: the pass enqueued fused ladder launches (their commit / redo launch must follow: staged_follow_up)
int launch_staged(cnl_handle* h, cnl::LaunchArgs& a, bool first_attempt_only, bool& ladder_ran, hipStream_t stream) {
  begin_launch(h, a, stream);
  a.L = h->d_L; a.scratch = h->d_gs;
  a.tasks = h->d_tasks; a.gcnt = h->d_gcnt; a.skip_done = 0; a.dep = h->d_dep; a.df_waves = h->df_waves;
  a.status_total = h->d_status;
  a.status_call = h->d_stat;   // (nullptr in views of the handle: one launch per stage, nothing waits)
  a.lad = h->d_lad; a.lgcnt = h->d_lgcnt; a.ldep = h->d_ldep; a.lad_zero_ints = h->d_stat ? h->zero_ints : 0;
  a.lad_capacity = h->resident_waves;
  a.lad_mode = (a.mode == cnl::MODE_NEWTON && h->d_lad && !first_attempt_only) ? h->lad_mode : 0;
  ladder_ran = a.lad_mode != 0;
  a.spin_limit = h->plan->opt.dataflow_spin_limit > 0 ? h->plan->opt.dataflow_spin_limit : (1 << 22);
  if (h->timing) HIPCHK(hipEventRecord(h->ev0, stream));
  // (a Float32 handle — tuning float32_staged — runs the staged float instances: lad_mode = 0, a.dep = nullptr and lean = 0 by
  //  setup_v2, unless tuning float32_latency set them up by the Float64 rules)
  hipError_t e = cnl::launch_newton2_staged(h->dp2, h->wpb2, h->lds2, a, h->stage_ptr.data(), (int)h->stage_ptr.size() - 1, stream, h->f32);
  if (e != hipSuccess) return fail(CNL_ERR_HIP, std::string("staged launch: ") + hipGetErrorString(e));
  return CNL_OK;
}

// One call of a subtree handle of either element type (tuning general_subtrees, float32_subtrees; DESIGN sections 3.2 and 9.11),
// S = stages of the cut: a launch per stage walks the tasks of that stage forward (one workgroup per problem and task); where the call factorises, the decide kernel behind the last stage
// makes the flags of the first attempt; where it solves, a launch per stage in reverse runs the backward sweeps of the problems that
// hold a factor; newton_system ends with the climbers' launch, which takes the failed problems through the whole ladder.
// Launches: newton_system 2 S + 2, try_to_factorize S + 1, solve_ldl! 2 S.  The order on the stream is the only dependency.
// The handle keeps the flags of its last factorisation (d_blk_ok), which solve_ldl! and the expand pass read.
// Tuning subtree_ladder = R > 0 changes newton_system alone: the first decide also writes the ladder state; R rungs
// follow, each the S stages at every climbing problem's rho and a rung-decide launch; then the backward stages, the commit of the rho
// slots and the climbers, who resume the problems still climbing.  (R + 2) S + R + 3 launches, whatever the problems need: the host
// reads nothing back, and a rung no problem needs is S + 1 launches of workgroups that leave at once.
int launch_subtrees(cnl_handle* h, cnl::LaunchArgs& a, hipStream_t stream) {
  begin_launch(h, a, stream);
  const bool newton = a.mode == cnl::MODE_NEWTON, solve = a.mode == cnl::MODE_SOLVE;
  const int nst = (int)h->gstage_ptr.size() - 1, ntasks = h->gstage_ptr[nst];
  a.L = h->d_L; a.scratch = h->d_scratch;
  a.tasks = h->d_gtasks; a.gcnt = h->d_sub_cnt; a.ntasks_all = ntasks; a.skip_done = 0;
  int32_t* const callers_flags = a.success;
  if (solve) a.success = h->d_blk_ok;
  if (h->timing) HIPCHK(hipEventRecord(h->ev0, stream));
  hipError_t e = hipSuccess;
  // (tuning subtree_wide / subtree_lds_panels, DESIGN section 3.4: a factorising forward launch takes its stage's shape at this launch's
  //  batch; the vector sweeps of solve_ldl! and the backward stages keep the handle's)
  auto stage = [&](int s, int phase) {
    a.phase = phase; a.task0 = h->gstage_ptr[s]; a.ntasks = h->gstage_ptr[s + 1] - h->gstage_ptr[s];
    g_launches[2]++;
    // (tuning subtree_solve_panels, DESIGN section 3.5: a backward stage — bit 0 — and a forward stage of solve_ldl! — bit 1 — run the
    //  panelled entries where the stage's vector and panel areas fit a workgroup's LDS)
    const int panel_bit = phase == 1 ? 1 : (solve ? 2 : 0);
    if ((h->solve_panels & panel_bit) && h->gstage_solve_lds[s])
      return cnl::launch_subtree_solve(h->dp, h->cfg, a, stream, h->f32, h->gstage_fmax[s], (size_t)h->gstage_solve_lds[s]);
    if (phase != 0 || solve) return cnl::launch_newton_subtrees(h->dp, h->cfg, a, stream, h->f32);
    const cnl::SubtreeStageShape sh = subtree_stage_shape(h, s, a.batch);
    return cnl::launch_newton_subtrees(h->dp, h->cfg, a, stream, h->f32, &sh);
  };
  const int rungs = newton ? h->ladder_rungs : 0;
  const cnl::LadderState lad{h->d_lad_done, h->d_lad_rho, rungs};
  for (int s = 0; s < nst && e == hipSuccess; s++) e = stage(s, 0);
  if (!solve && e == hipSuccess) {
    g_launches[2]++;   // (cnl_launch_counts: the decide kernel is a launch of the pass, counted with the stages)
    e = rungs ? cnl::launch_subtree_ladder_first(a, lad, h->d_sub_cnt, ntasks, (int)h->dp.nvar, stream, h->f32)
              : cnl::launch_subtree_decide(a, h->d_sub_cnt, ntasks, (int)h->dp.nvar, stream, h->f32);
  }
  for (int k = 1; k <= rungs && e == hipSuccess; k++) {
    for (int s = 0; s < nst && e == hipSuccess; s++) {
      a.phase = 0; a.task0 = h->gstage_ptr[s]; a.ntasks = h->gstage_ptr[s + 1] - h->gstage_ptr[s];
      g_launches[2]++;
      const cnl::SubtreeStageShape sh = subtree_stage_shape(h, s, a.batch);
      e = cnl::launch_subtree_ladder(h->dp, h->cfg, a, lad, stream, h->f32, &sh);
    }
    if (e != hipSuccess) break;
    g_launches[2]++;
    e = cnl::launch_subtree_rung_decide(a, lad, k, h->d_sub_cnt, ntasks, (int)h->dp.nvar, stream, h->f32);
  }
  if (a.mode != cnl::MODE_FACTOR)
    for (int s = nst - 1; s >= 0 && e == hipSuccess; s--) e = stage(s, 1);
  if (rungs && e == hipSuccess) {
    g_launches[2]++;
    e = cnl::launch_subtree_ladder_commit(h->dp, a, lad, stream, h->f32);
  }
  if (newton && e == hipSuccess) {
    a.phase = 2; a.task0 = 0; a.ntasks = ntasks; a.skip_done = 1;
    g_launches[2]++;
    e = rungs ? cnl::launch_subtree_ladder(h->dp, h->cfg, a, lad, stream, h->f32) : cnl::launch_newton_subtrees(h->dp, h->cfg, a, stream, h->f32);
    a.skip_done = 0;
  }
  if (!solve && e == hipSuccess)
    e = hipMemcpyAsync(h->d_blk_ok, a.success, (size_t)h->batch * sizeof(int32_t), hipMemcpyDeviceToDevice, stream);
  a.success = callers_flags;
  if (e != hipSuccess)
    return fail(CNL_ERR_HIP, std::string("subtree launch (tpp=") + std::to_string(h->cfg.tpp) + ", " + std::to_string(ntasks) + " tasks in " +
                                 std::to_string(nst) + " stages): " + hipGetErrorString(e));
  if (h->timing) HIPCHK(hipEventRecord(h->ev1, stream));
  return CNL_OK;
}

}  // namespace

// SubBatch (handle.h): the table's view moves the handle's per-problem arrays; the rest of the view is set here, and undone when it
// goes out of scope
SubBatch::SubBatch(cnl_handle* h_, int64_t b0, int64_t nb, bool allow_staged)
    : h(h_), arrays(h_->batch_arrays, b0), batch(h_->batch), last_vals(h_->last_vals), staged(h_->staged), dep(h_->d_dep), lad(h_->d_lad), stat(h_->d_stat) {
  h->batch = nb;
  h->last_vals = elem_offset(h, h->last_vals, b0 * h->plan->nnz);
  if (!allow_staged) h->staged = false;
  h->d_dep = nullptr; h->d_lad = nullptr; h->d_stat = nullptr;   // views run one launch per stage and keep the sequential ladder
}

SubBatch::~SubBatch() {
  h->batch = batch; h->last_vals = last_vals; h->staged = staged;
  h->d_dep = dep; h->d_lad = lad; h->d_stat = stat;
}

namespace {

// run() on problems [b0, b0 + nb) of the handle and of the caller's arrays, as one part of a split batch: the view, the result arrays
// and vals / rhs / d from problem b0 on (the caller's `a` is left as it is)
int run_part(cnl_handle* h, const cnl::LaunchArgs& a, void* d_vals, const void* d_rhs, void* d_d, int64_t b0, int64_t nb, bool allow_staged,
             hipStream_t stream, RunOpts o) {
  const int64_t nnz = h->plan->nnz, N = h->plan->N;
  SubBatch view(h, b0, nb, allow_staged);
  cnl::LaunchArgs b = shifted(h, a, b0);
  return run(h, b, elem_offset(h, d_vals, b0 * nnz), elem_offset(h, d_rhs, b0 * N), elem_offset(h, d_d, b0 * N), stream, o);
}

// Batches between one and two wavefronts per SIMD (4096 .. 8192 problems of cfg3's size): the single stream gives a group of
// four problems ONE wavefront for 1000 fronts, the bidirectional chain TWO for 500 each, and the machine holds 2048 wavefronts.
// With x groups on the chain and y on the stream, 2 x + y = 2048 fills every slot whatever the batch: the chain part runs staged
// on the caller's stream, the rest single-stream on a second stream of the handle, forked and joined with events (no host
// synchronisation).  Both parts use the SAME plan — the chain order has the throughput order's fronts, and the classic launch
// runs any plan's records from end to end (it already does behind every staged attempt).
// (the parts are calls of run() with part_of_split set; the events of a timed call bracket all of them)
int run_split_parts(cnl_handle* h, cnl::LaunchArgs& a, void* d_vals, const void* d_rhs, void* d_d, hipStream_t stream, RunOpts o) {
  const int64_t nA = h->split_staged, nB = h->batch - nA;
  TimingOff untimed(h);
  o.part_of_split = true;
  if (h->tail || h->split_halves) {
    // One part behind the other on the caller's stream.  Tail: 4096 problems fill every wavefront slot on the bidirectional chain
    // (4.1 ms at cfg3's size); a remainder of r <= 1024 problems takes 0.5 .. 1.7 ms on its own many-part plan, where two halves of the
    // whole batch need 2 x 3 ms (4608 problems: 5.95 -> 5.0 ms).  Two halves, each on the chain (two wavefronts per group of problems):
    // a half of 2304 .. 3840 problems runs at 0.81 .. 0.96 M systems/s, where the single-stream part of the concurrent split needs
    // its >= 6 ms however few problems it holds (4608 problems: 6.5 ms = 707 k systems/s; two halves: ~5.7 ms).
    cnl_handle* t = h->tail;
    const bool on_tail = t && (a.mode != cnl::MODE_SOLVE || h->tail_fresh);   // (else the remainder's factors are in this handle's storage)
    if (int rc = run_part(h, a, d_vals, d_rhs, d_d, 0, nA, true, stream, o)) return rc;
    if (!on_tail) return run_part(h, a, d_vals, d_rhs, d_d, nA, nB, true, stream, o);
    // a whole call of the tail handle, on the caller's arrays from problem nA on
    cnl::LaunchArgs b = shifted(h, a, nA);
    void* tv = elem_offset(h, d_vals, nA * h->plan->nnz);
    const int rc = run(t, b, tv, elem_offset(h, d_rhs, nA * h->plan->N), elem_offset(h, d_d, nA * h->plan->N), stream, RunOpts{o.first_attempt_only, false});
    if (rc == CNL_OK && a.mode != cnl::MODE_SOLVE) { t->last_vals = tv; t->factorized = true; h->tail_fresh = true; }
    return rc;
  }
  HIPCHK(hipEventRecord(h->ev_fork, stream));
  HIPCHK(hipStreamWaitEvent(h->aux_stream, h->ev_fork, 0));
  int rc = run_part(h, a, d_vals, d_rhs, d_d, nA, nB, false, h->aux_stream, o);
  if (rc == CNL_OK) rc = run_part(h, a, d_vals, d_rhs, d_d, 0, nA, true, stream, o);
  // join also when an enqueue failed: work already on the second stream must not overlap a later call's use of the handle's arrays
  const hipError_t je = hipEventRecord(h->ev_join, h->aux_stream);
  const hipError_t we = je == hipSuccess ? hipStreamWaitEvent(stream, h->ev_join, 0) : je;
  if (rc) { if (we != hipSuccess) (void)hipStreamSynchronize(h->aux_stream); return rc; }
  HIPCHK(we);
  return CNL_OK;
}
int run_split(cnl_handle* h, cnl::LaunchArgs& a, void* d_vals, const void* d_rhs, void* d_d, hipStream_t stream, RunOpts o) {
  if (!h->aux_stream && !h->tail && !h->split_halves) {
    HIPCHK(hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
  }
  if (h->timing) HIPCHK(hipEventRecord(h->ev0, stream));
  if (int rc = run_split_parts(h, a, d_vals, d_rhs, d_d, stream, o)) return rc;
  return end_timed(h, stream);
}

// The classic launch behind launch_staged (the caller's events bracket it too).  newton_system, whose first attempt (rho as given) ran
// stage by stage: the problems that failed it (rare) go through the whole rho ladder here, the others are skipped (skip_done).
// Everything else is the REDO: the sequential execution of the same call, which exits at once unless a dataflow wait of the attempt
// gave up (kernels2.hip, spin_until) — try_to_factorize, solve_ldl!, a newton_system whose failed problems have climbed the ladder
// inside the fused launches (ladder_ran: the redo also commits rho_old and the rho slots), or one the host ladder follows
// (first_attempt_only: the redo goes through the device ladder, and the host finds the per-call status word set).
int staged_follow_up(cnl_handle* h, cnl::LaunchArgs& a, bool ladder_ran, bool first_attempt_only, hipStream_t stream) {
  TimingOff untimed(h);
  if (a.mode == cnl::MODE_NEWTON && !ladder_ran && !first_attempt_only) {
    a.skip_done = 1;
    return launch(h, a, stream);
  }
  if (!a.status_call || (!h->d_dep && !ladder_ran)) return CNL_OK;  // one launch per stage: nothing waits, nothing can time out
  a.only_if_status = 1;
  const int rc = launch(h, a, stream);
  a.only_if_status = 0;
  return rc;
}

// The stand-alone condensation passes around a launch on the condensed system (csrc/condense.h).
// condense: which slots of the handle's condensed buffer are formed from `vals` [and `rhs`] (call_shape.h: CondensePart; the plain
// kernel takes the tiled kernel's mask as a slot range)
// (T: the handle's element type, picked from h->f32 by the three functions without a T; each types its arguments once on entry)
template <class T>
hipError_t condense_t(cnl_handle* h, cnl::CondensePart part, const void* vals, const void* rhs, hipStream_t stream) {
  const cnl::Cond& C = h->plan->C;
  const int B = (int)h->batch, s_mat = (int)(C.ncs + C.nvar), s_all = (int)C.cstride;
  const T* v = static_cast<const T*>(vals);
  const T* r = static_cast<const T*>(rhs);
  T* cbuf = static_cast<T*>(h->d_cbuf);
  using cnl::MATRIX_ONLY; using cnl::RHS_ONLY;
  if constexpr (sizeof(T) == 4)
    if (h->cond_resident)
      return cnl::launch_condense_resident(h->dce, v, r, cbuf, part == RHS_ONLY ? s_mat : 0, part == MATRIX_ONLY ? s_mat : s_all, B, stream);
  return C.tiled_ok ? cnl::launch_condense_tiled(h->dc, v, r, cbuf, part, C.ch_region[3], B, stream)
                    : cnl::launch_condense(h->dc, v, r, cbuf, part == RHS_ONLY ? s_mat : 0, part == MATRIX_ONLY ? s_mat : s_all, B, stream);
}
// (a handle without the condensed buffer — a band handle — has none of these passes)
int no_cbuf() { return fail(CNL_ERR_STATE, "this handle has no condensed buffer: the condensation passes do not serve it"); }
int condense(cnl_handle* h, cnl::CondensePart part, const void* vals, const void* rhs, hipStream_t stream) {
  if (!h->d_cbuf) return no_cbuf();
  const hipError_t e = h->f32 ? condense_t<float>(h, part, vals, rhs, stream) : condense_t<double>(h, part, vals, rhs, stream);
  if (e != hipSuccess) return fail(CNL_ERR_HIP, std::string("condense: ") + hipGetErrorString(e));
  return CNL_OK;
}
// inertia of the condensed pivots, for the kernels that do not count them themselves (Float32: against eig_tol narrowed to float)
int cond_inertia(cnl_handle* h, const void* vals, double eig_tol, hipStream_t stream) {
  const hipError_t e = h->f32 ? cnl::launch_cond_inertia(h->dc, static_cast<const float*>(vals), h->d_xpos, h->d_xzer, (float)eig_tol, (int)h->batch, stream)
                              : cnl::launch_cond_inertia(h->dc, static_cast<const double*>(vals), h->d_xpos, h->d_xzer, eig_tol, (int)h->batch, stream);
  if (e != hipSuccess) return fail(CNL_ERR_HIP, std::string("condense: ") + hipGetErrorString(e));
  return CNL_OK;
}
// post-pass: the condensed components of d (and, d2 != nullptr, the kept ones out of the reduced solution)
template <class T>
hipError_t expand_t(cnl_handle* h, const void* vals, const void* rhs, const void* d2, void* d, const int* success, int copy_rho_tail, hipStream_t stream) {
  return cnl::launch_expand(h->dc, static_cast<T*>(const_cast<void*>(vals)), static_cast<const T*>(rhs), static_cast<const T*>(d2),
                            static_cast<const T*>(h->d_cbuf), static_cast<T*>(d), success, copy_rho_tail, (int)h->batch, stream);
}
int expand(cnl_handle* h, const void* vals, const void* rhs, const void* d2, void* d, const int* success, int copy_rho_tail, hipStream_t stream) {
  if (!h->d_cbuf) return no_cbuf();
  const hipError_t e = h->f32 ? expand_t<float>(h, vals, rhs, d2, d, success, copy_rho_tail, stream)
                              : expand_t<double>(h, vals, rhs, d2, d, success, copy_rho_tail, stream);
  if (e != hipSuccess) return fail(CNL_ERR_HIP, std::string("expand: ") + hipGetErrorString(e));
  return CNL_OK;
}

}  // namespace

namespace {

// dense residual block: J'WJ + tiled dense LDL^T on the fp64 matrix cores (csrc/dense.hip); asynchronous, the rho ladder is decided
// on the device
int run_dense(cnl_handle* h, cnl::LaunchArgs& a, void* d_vals, const void* d_rhs, void* d_d, hipStream_t stream) {
  std::string err;
  if (const int* pat = dbg_ldsfill()) (void)cnl::launch_lds_fill(*pat, stream);
  if (h->timing) HIPCHK(hipEventRecord(h->ev0, stream));
  // (a Float32 handle — tuning float32_dense — runs the float kernels of csrc/dense_f32.hip: same sequence, float element arrays)
  const int rc = h->f32 ? cnl::dense_run_f32(h->dense, a.mode, d_vals, d_rhs, d_d, a.rho_old, a.rho, a.nfact, a.success, a.npos, a.nzero, a.params, stream, err)
                        : cnl::dense_run(h->dense, h->plan->D, a.mode, f64(h, d_vals), f64(h, d_rhs), f64(h, d_d), f64(h, a.rho_old), f64(h, a.rho), a.nfact,
                                         a.success, a.npos, a.nzero, a.params, stream, err);
  if (rc) return fail(rc == 5 ? CNL_ERR_STATE : CNL_ERR_HIP, "dense backend: " + err);
  return end_timed(h, stream);
}

// The executor of the Plain, Direct, Condensed and GeneralDense routes: [condense -> inertia ->] launch [-> expand], as S says
// (call_shape.h).  The launch is the multifrontal kernel — one classic launch, or stage by stage with its follow-up — or, on the
// GeneralDense route, the dense LDL^T / solves of the condensed system as one matrix (csrc/dense.hip).  The events of a timed call
// bracket the classic launch alone (launch()), the staged pass with its follow-up (the register-front kernel's, or the general
// kernel's subtree pass: launch_subtrees), or the whole dense route.
int execute(cnl_handle* h, const cnl::CallShape& S, cnl::LaunchArgs& a, void* d_vals, const void* d_rhs, void* d_d, hipStream_t stream, RunOpts o) {
  const cnl::Cond& C = h->plan->C;
  const bool gdense = S.launch == cnl::Launch::GeneralDense, factors = a.mode != cnl::MODE_SOLVE, solves = a.mode != cnl::MODE_FACTOR;
  const void* src = S.needs_last_vals ? h->last_vals : d_vals;   // the values the call is about
  int rc;
  if (gdense) {
    if (const int* pat = dbg_ldsfill()) (void)cnl::launch_lds_fill(*pat, stream);
    if (h->timing) HIPCHK(hipEventRecord(h->ev0, stream));
  }
  if (S.condense && (rc = condense(h, S.condense, src, solves ? d_rhs : nullptr, stream))) return rc;
  if (S.inertia && (rc = cond_inertia(h, d_vals, a.params[0], stream))) return rc;
  if (gdense) {
    std::string err;
    // (a Float32 handle — tuning float32_general_dense — runs the float kernels of csrc/dense_f32.hip: same sequence, float element arrays)
    rc = h->f32 ? cnl::dense_run_general_f32(h->gdense, h->gops, a.mode, h->d_cbuf, h->d_xpos, h->d_xzer, h->d_d2, elem_offset(h, d_vals, C.nnz - C.nvar),
                                             C.nnz, a.rho_old, a.rho, a.nfact, a.success, a.npos, a.nzero, a.params, stream, err)
                : cnl::dense_run_general(h->gdense, h->gops, a.mode, f64(h, h->d_cbuf), h->d_xpos, h->d_xzer, f64(h, h->d_d2),
                                         d_vals ? f64(h, d_vals) + (C.nnz - C.nvar) : nullptr, C.nnz, f64(h, a.rho_old), f64(h, a.rho), a.nfact,
                                         a.success, a.npos, a.nzero, a.params, stream, err);
    if (rc) return fail(CNL_ERR_HIP, "dense backend: " + err);
  } else {
    // (from the condensed buffer: the matrix slots where the call factorises, the right-hand-side slots where it solves)
    a.vals = !S.from_cbuf ? const_cast<void*>(src) : factors ? h->d_cbuf : nullptr;
    a.rhs = !S.from_cbuf ? d_rhs : solves ? elem_offset(h, h->d_cbuf, C.ncs + C.nvar) : nullptr;
    a.d = S.d_to_d2 ? h->d_d2 : d_d;
    a.extra_pos = S.extra_counts ? h->d_xpos : nullptr; a.extra_zer = S.extra_counts ? h->d_xzer : nullptr;
    if (S.launch == cnl::Launch::Staged) {
      bool ladder_ran = false;
      if ((rc = launch_staged(h, a, o.first_attempt_only, ladder_ran, stream))) return rc;
      if ((rc = staged_follow_up(h, a, ladder_ran, o.first_attempt_only, stream))) return rc;
      if (h->timing) HIPCHK(hipEventRecord(h->ev1, stream));
    } else if (S.launch == cnl::Launch::Subtrees) {
      if ((rc = launch_subtrees(h, a, stream))) return rc;
    } else if ((rc = launch(h, a, stream))) return rc;
  }
  if (S.expand && (rc = expand(h, src, d_rhs, S.expand_d2 ? h->d_d2 : nullptr, d_d, S.expand_success ? a.success : !solves || factors ? nullptr : h->d_blk_ok, S.copy_rho_tail, stream))) return rc;
  return gdense ? end_timed(h, stream) : h->timing ? read_timing(h) : CNL_OK;
}

cnl::RouteFacts route_facts(const cnl_handle* h) {
  const cnl::Plan& P = h->plan->P;
  return {h->route, h->dp2.count_d != 0, P.d_outer != 0, h->v2_solve, h->lean && P.back_rows, h->staged, h->subtrees};
}

}  // namespace

namespace {

hipError_t residual_step(cnl_handle* h, const double* vals, const double* rhs, const double* d, int j, hipStream_t stream) {
  return cnl::launch_kkt_residual(h->dkkt, vals, rhs, d, h->r_rhs, h->r_norms + j, h->refine_k, h->r_success, (int)h->batch, stream);
}

// One call of a refined handle (tuning float32_refine; handle.h: cnl_handle::inner), everything on the caller's stream and nothing
// read back: the inputs demoted into the handle's float arrays, the call of the inner Float32 handle — the rho ladder, nfact and
// success are its own —, the results widened, then k times  g = rhs + K d  (Float64 data, written as float into the inner
// right-hand side)  ->  e = inner solve(g)  ->  d += e  where the problem holds a factor.
// eig_tol of the inner factorisation is max((float)eig_tol, eps(Float32)): a pivot below Float32 rounding is noise in a Float32
// factor — the one deliberate deviation in decisions from a Float64 handle.
int run_refined(cnl_handle* h, cnl::LaunchArgs& a, void* d_vals, const void* d_rhs, void* d_d, hipStream_t stream) {
  cnl_handle* in = h->inner;
  const int64_t B = h->batch, N = h->plan->N, nnz = h->plan->nnz;
  if (a.skip_done || a.only_if_status || (a.mode == cnl::MODE_NEWTON && !d_rhs))
    return fail(CNL_ERR_STATE, "this call is not served by a refined handle (tuning float32_refine)");
  if (a.mode == cnl::MODE_SOLVE && !h->last_vals) return fail(CNL_ERR_STATE, "cnl_solve before cnl_factorize");
  if (in->batch != B) return fail(CNL_ERR_STATE, "refined handle: the inner handle works on another batch");
  const double* vals = static_cast<const double*>(a.mode == cnl::MODE_SOLVE ? h->last_vals : d_vals);
  const double* rhs = static_cast<const double*>(d_rhs);
  double* d = static_cast<double*>(d_d);
  auto hip = [](hipError_t e, const char* what) { return e == hipSuccess ? CNL_OK : fail(CNL_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); };
  int rc;
  if (h->timing) HIPCHK(hipEventRecord(h->ev0, stream));
  if (a.mode != cnl::MODE_SOLVE && (rc = hip(cnl::launch_refine_demote(vals, h->r_vals, B * nnz, stream), "refine_demote"))) return rc;
  if (a.mode != cnl::MODE_FACTOR && (rc = hip(cnl::launch_refine_demote(rhs, h->r_rhs, B * N, stream), "refine_demote"))) return rc;
  float p32[9] = {};
  const int np = a.mode == cnl::MODE_NEWTON ? 9 : a.mode == cnl::MODE_FACTOR ? 1 : 0;
  for (int k = 0; k < np; k++) p32[k] = (float)a.params[k];
  if (np) p32[0] = std::max(p32[0], FLT_EPSILON);
  if (a.mode == cnl::MODE_NEWTON) {
    if ((rc = hip(cnl::launch_refine_demote(static_cast<const double*>(a.rho_old), h->r_rho_old, B, stream), "refine_demote"))) return rc;
    if ((rc = cnl_newton_system_f32_dev(in, h->r_vals, h->r_rhs, h->r_e, h->r_rho_old, h->r_rho, a.nfact, a.success, p32, stream))) return rc;
    if ((rc = hip(cnl::launch_refine_widen_rho(h->r_rho, h->r_rho_old, static_cast<double*>(a.rho), static_cast<double*>(a.rho_old), h->r_vals,
                                               static_cast<double*>(d_vals), nnz, (int)h->plan->nvar, a.nfact, (int)B, stream), "refine_widen_rho"))) return rc;
  } else if (a.mode == cnl::MODE_FACTOR) {
    // (the inertia counts of a host-pointer try_to_factorize: straight through run(), as factorize_impl<float> asks for them)
    cnl::LaunchArgs f{};
    f.mode = cnl::MODE_FACTOR; f.success = a.success; f.npos = a.npos; f.nzero = a.nzero; f.params[0] = p32[0];
    HIPCHK(hipSetDevice(in->device));
    if ((rc = run(in, f, h->r_vals, nullptr, nullptr, stream))) return rc;
    in->factorized = true; in->factor_batch = in->batch; in->last_vals = h->r_vals; in->last_ok.clear();
  } else {
    if ((rc = cnl_solve_f32_dev(in, h->r_rhs, h->r_e, stream))) return rc;
  }
  if (a.mode != cnl::MODE_SOLVE) {
    HIPCHK(hipMemcpyAsync(h->r_success, a.success, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    h->last_vals = d_vals;
  }
  if (a.mode != cnl::MODE_FACTOR) {
    if ((rc = hip(cnl::launch_refine_update(d, h->r_e, h->r_success, (int)N, (int)B, 1, stream), "refine_update"))) return rc;
    for (int j = 0; j < h->refine_k; j++) {
      if ((rc = hip(residual_step(h, vals, rhs, d, j, stream), "kkt_residual"))) return rc;
      if ((rc = cnl_solve_f32_dev(in, h->r_rhs, h->r_e, stream))) return rc;
      if ((rc = hip(cnl::launch_refine_update(d, h->r_e, h->r_success, (int)N, (int)B, 0, stream), "refine_update"))) return rc;
    }
    h->r_norms_valid = true;
  }
  return end_timed(h, stream);
}

}  // namespace

// cnl_kkt_residual_dev: the residual kernel on its own, on any Float64 handle with problem-major vals
int kkt_residual(cnl_handle* h, const double* d_vals, const double* d_rhs, const double* d_d, double* d_g, double* d_norms, hipStream_t stream) {
  if (int rc = ensure_kkt_rows(h)) return rc;
  HIPCHK(hipSetDevice(h->device));
  const hipError_t e = cnl::launch_kkt_residual(h->dkkt, d_vals, d_rhs, d_d, d_g, d_norms, 1, nullptr, (int)h->batch, stream);
  if (e != hipSuccess) return fail(CNL_ERR_HIP, std::string("kkt_residual: ") + hipGetErrorString(e));
  return CNL_OK;
}

// One call of the path on device-resident data.  A split batch comes back here part by part; the rule of last_vals — the solve
// uses the values of the last factorisation — is checked and kept here for every route (call_shape.h: needs / sets).
int run(cnl_handle* h, cnl::LaunchArgs& a, void* d_vals, const void* d_rhs, void* d_d, hipStream_t stream, RunOpts o) {
  if (h->inner) return run_refined(h, a, d_vals, d_rhs, d_d, stream);   // (no route of call_shape.h: a sequence of calls of the inner handle)
  const cnl::CallShape S = cnl::call_shape(route_facts(h), a.mode);
  int rc;
  if (h->split_staged > 0 && !o.part_of_split && (h->staged || h->tail) && h->split_staged < h->batch) rc = run_split(h, a, d_vals, d_rhs, d_d, stream, o);
  // (a Float32 general handle refuses what its kernel does not serve here, before a condensation pass is enqueued)
  else if (h->route != cnl::Route::Band && (rc = f32_general_serves(h, a, d_rhs))) return rc;
  else if (S.needs_last_vals && !h->last_vals) return fail(CNL_ERR_STATE, "cnl_solve before cnl_factorize");
  else switch (h->route) {
    case cnl::Route::Band: rc = run_band(h, a, d_vals, d_rhs, d_d, stream); break;
    case cnl::Route::Dense: rc = run_dense(h, a, d_vals, d_rhs, d_d, stream); break;
    default: rc = execute(h, S, a, d_vals, d_rhs, d_d, stream, o);
  }
  if (rc == CNL_OK && S.sets_last_vals) h->last_vals = d_vals;
  return rc;
}

extern "C" int cnl_launch_counts(int64_t counts[3]) {
  if (!counts) return fail(CNL_ERR_ARG, "null argument");
  for (int k = 0; k < 3; k++) counts[k] = g_launches[k].load();
  return CNL_OK;
}
