// capi_handle.cpp — the device state of a handle, for both element types: creation from a plan (uploads, the choice of the kernel
// backend and its configuration, band kernels, batch layout, row lists of rows f1 / f4), destruction, and what a caller may read
// back or switch on a handle (configuration, timing, layout lengths and conversions).
#include "handle.h"

namespace {

// Float64 handles have the register-front kernel beside the band kernels.  On the pattern that needs the wide program it measured
// FASTER than the wide kernel (model_band_structure(10000, 50), same machine, alternated: 8 192 problems 8.31 against 8.67 ms, 16 384
// problems 15.78 against 17.42 ms; `vals` interleaved 8.68 / 17.2 ms — DESIGN section 4, tools/time_band_wide.py), so a Float64 handle
// runs the wide program only where tuning band_pieces = 20 asks for it; the 15-piece program is chosen as it always was.
// (Float32 handles have no other kernel: they always take the wide program where the pattern needs it.)
bool band_wide_serves_f64(const cnl_plan* plan) {
  return band_program(plan, false).npiece == cnl::BAND_NPIECE || plan->opt.band_pieces == cnl::BAND_NPIECE_WIDE;
}

// The general kernel's work area and launch configuration, for the handle's element type.  A Float32 handle is asked with its
// 4-byte elements — twice the problems per workgroup fit, and fronts up to order ~190 keep their work area in LDS — and chooses
// among the configurations compiled for float (kernels.h: newton_f32_has).
int choose_config(cnl_handle* h) {
  const cnl::Plan& P = h->plan->P;
  const size_t esz = h->esz();
  cnl::DevPlan& dp = h->dp;
  int64_t pb_off = std::max<int64_t>(P.fwd_peak, P.bwd_peak);
  pb_off = (pb_off + 1) & ~(int64_t)1;
  int64_t wv_off = pb_off + ((P.panel_max + 1) & ~1);
  // (tuning general_blocked, on a Float32 handle float32_blocked: the panel buffer W[16][fmax] takes the place of the two staging
  //  vectors, and the work area is sized — and placed in LDS or global scratch — with it whether or not the configuration chosen below
  //  has a blocked instance; elements of the handle's type)
  const bool want_blocked = h->f32 ? h->plan->opt.float32_blocked != 0 : h->plan->opt.general_blocked != 0;
  int64_t work = wv_off + (want_blocked ? 16 : 2) * (int64_t)((P.fmax + 1) & ~1);
  if (work >= ((int64_t)1 << 30))
    return fail(CNL_ERR_DIM, h->f32 ? "cnl_create_f32: work area too large (largest front of order " + std::to_string(P.fmax) + ")" : std::string("work area too large"));
  dp.pb_off = (int32_t)pb_off;
  dp.wv_off = (int32_t)wv_off;
  dp.work_doubles = (int32_t)work;
  size_t maxlds = cnl::max_lds_bytes();
  if (maxlds == 0) return fail(CNL_ERR_HIP, "cannot query LDS size (no HIP device?)");
  maxlds = std::min<size_t>(maxlds, 160 * 1024);
  cnl::KernelConfig& c = h->cfg;
  const size_t hdr = 16 * esz;
  const size_t per = (size_t)work * esz;
  int tpp, ppb, ldsw;
  if (hdr + per <= maxlds) {
    ldsw = 1;
    if (P.fmax <= 96) {
      tpp = 64;
      // problems per workgroup: leave room for two workgroups per CU when the work area
      // allows it, and spread small batches over the 256 CUs
      size_t fit = (maxlds - hdr) / per;
      size_t fit2 = maxlds / 2 > hdr ? (maxlds / 2 - hdr) / per : 0;
      size_t cap = fit2 >= 1 ? fit2 : fit;
      size_t want = (size_t)std::min<int64_t>(16, std::max<int64_t>(1, h->batch / 256));
      ppb = 1;
      for (int cand : {16, 8, 4, 2, 1})
        if ((size_t)cand <= cap && (size_t)cand <= want && (!h->f32 || cnl::newton_f32_has(tpp, cand, true))) { ppb = cand; break; }
    } else {
      tpp = P.fmax <= 400 || h->f32 ? 256 : 1024;
      ppb = 1;
    }
  } else {
    ldsw = 0;
    tpp = P.fmax <= 96 ? 64 : (P.fmax <= 400 || h->f32 ? 256 : 1024);
    ppb = tpp == 64 ? 4 : 1;
  }
  const cnl::Tuning& o = h->plan->opt;
  if (o.v1_tpp > 0) tpp = o.v1_tpp;
  if (o.v1_ppb > 0) ppb = o.v1_ppb;
  if (o.v1_lds >= 0) ldsw = o.v1_lds;
  c.tpp = tpp; c.ppb = ppb; c.lds_work = ldsw;
  c.blocked = want_blocked && cnl::newton_blocked_has(tpp, ppb, h->f32);
  c.lds_bytes = hdr + (ldsw ? (size_t)ppb * per : 0);
  if (h->f32) {
    const std::string what = "tpp=" + std::to_string(tpp) + " ppb=" + std::to_string(ppb) + " lds=" + std::to_string(ldsw);
    if (c.lds_bytes > maxlds)
      return fail(CNL_ERR_DIM, "cnl_create_f32: the work area of the general kernel (largest front of order " + std::to_string(P.fmax) + ", " +
                                   std::to_string(per) + " bytes per problem) does not fit the LDS of a workgroup with " + what);
    if (!cnl::newton_f32_has(tpp, ppb, ldsw != 0))
      return fail(CNL_ERR_ARG, "cnl_create_f32: the general kernel has no Float32 instance for " + what + " (tuning v1_tpp / v1_ppb / v1_lds; largest front of order " +
                                   std::to_string(P.fmax) + ")");
    return CNL_OK;
  }
  if (c.lds_bytes > maxlds) return fail(CNL_ERR_DIM, "kernel configuration exceeds LDS");
  return CNL_OK;
}

// The success flags a blocked handle keeps (handle.h: d_blk_ok), for the handles cnl_get_config reports as blocked (bit 47, in float
// bit 48): the Newton / factorise launches are the general kernel's, in a configuration with a blocked instance.  No flag set: no
// problem holds a factor yet.
int alloc_blocked_flags(cnl_handle* h) {
  if ((!h->cfg.blocked && !h->subtrees) || h->use_v2 || h->band || h->dense || h->gdense) return CNL_OK;   // (a subtree handle keeps them too)
  if (int rc = dalloc_batch(h, &h->d_blk_ok, 1)) return rc;
  if (hipMemset(h->d_blk_ok, 0, (size_t)h->full_batch * sizeof(int32_t)) != hipSuccess) return fail(CNL_ERR_HIP, "hipMemset failed");
  return CNL_OK;
}

// Tuning general_subtrees, on a Float32 general handle float32_subtrees: does the key of the
// handle's element type act on this handle?  A pure function of plan, batch and options (the configuration is choose_config's, which
// reads the same three and the device's LDS size):
//   - the Newton / factorise launch is the general kernel: no register-front, band or dense route took the handle;
//   - one problem per workgroup of 256 or 1024 threads, in float of 256 (the configurations with subtree instances);
//   - the cut has at least two tasks in its first stage (a chain of single-front stages gains nothing: every stage is one task);
//   - the task regions of the whole batch, in elements of the handle's type, fit 8e9 bytes (the bound of the dense batch rule).
// Where it acts the work area becomes the global array of task regions (gwork elements per problem; LDS cannot be shared between
// workgroups) and the device plan walks the second front table.  Everywhere else nothing of the handle changes.
// To be called once the routes are decided and before the factor storage (and with it d_scratch) is allocated.
int setup_subtrees(cnl_handle* h) {
  const cnl::Plan& P = h->plan->P;
  const cnl::Tuning& o = h->plan->opt;
  if (!(h->f32 ? o.float32_subtrees : o.general_subtrees) || h->use_v2 || h->band || h->dense || h->gdense) return CNL_OK;
  if (!cnl::newton_subtrees_has(h->cfg.tpp, h->cfg.ppb, h->f32)) return CNL_OK;
  if (P.gtasks.empty() || P.gstage_ptr.size() < 2 || P.gstage_ptr[1] < 2) return CNL_OK;
  if ((double)h->full_batch * (double)P.gwork * (double)h->esz() > 8e9) return CNL_OK;
  int rc;
  const cnl::FrontHdr* d_gfronts = nullptr;
  if ((rc = upload(h, P.gfronts, &d_gfronts))) return rc;
  std::vector<int32_t> tk(reinterpret_cast<const int32_t*>(P.gtasks.data()), reinterpret_cast<const int32_t*>(P.gtasks.data()) + 8 * P.gtasks.size());
  if ((rc = upload(h, tk, &h->d_gtasks))) return rc;
  if ((rc = dalloc_batch(h, &h->d_sub_cnt, 2 * P.gtasks.size()))) return rc;   // (a view's slots: [tasks][nb][2] from its base)
  h->gstage_ptr = P.gstage_ptr;
  h->dp.fronts = d_gfronts;
  h->dp.work_doubles = (int32_t)P.gwork;
  h->cfg.lds_work = 0;
  h->cfg.lds_bytes = 16 * h->esz();
  h->subtrees = true;
  if (o.subtree_ladder > 0) {   // (tuning subtree_ladder: the ladder state of a call, moved and shortened with every array of the table)
    if ((rc = dalloc_batch(h, &h->d_lad_done, 1))) return rc;
    if ((rc = dalloc_batch(h, &h->d_lad_rho, 2))) return rc;
    h->ladder_rungs = o.subtree_ladder;
  }
  // tuning subtree_wide / subtree_lds_panels: the per-stage table of the factorising forward launches
  const int nst = (int)P.gstage_ptr.size() - 1;
  h->gstage_fmax.assign(nst, 0);
  h->gstage_lpan.assign(nst, 0);
  std::vector<char> has_panel(nst, 0);   // a front with at least PANEL_W (16) pivots: the only fronts eliminate_blocked takes
  for (const cnl::GTask& t : P.gtasks) {
    h->gstage_fmax[t.stage] = std::max(h->gstage_fmax[t.stage], t.fmax);
    for (int32_t f = t.f0; f < t.f1; f++) if (P.gfronts[f].npiv >= 16) has_panel[t.stage] = 1;
  }
  if (o.subtree_wide > 0 && h->cfg.tpp == 256) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) return fail(CNL_ERR_HIP, "hipGetDeviceProperties failed");
    h->sub_wide = o.subtree_wide;
    h->sub_cus = prop.multiProcessorCount;
  }
  if (o.subtree_lds_panels > 0 && h->cfg.blocked) {
    const size_t cap = std::min<size_t>(cnl::max_lds_bytes(), (size_t)160 * 1024);
    for (int s = 0; s < nst; s++) {
      const size_t need = (size_t)(16 + 32 * (int64_t)h->gstage_fmax[s]) * h->esz();
      if (h->gstage_fmax[s] <= o.subtree_lds_panels && has_panel[s] && need <= cap) h->gstage_lpan[s] = (int32_t)need;
    }
  }
  // tuning subtree_solve_panels: the dynamic LDS of a panelled solve sweep of a stage — the front's vector, the panel's
  // triangle and its 16 values (kernels.h: subtree_solve_lds_elems)
  h->gstage_solve_lds.assign(nst, 0);
  if (o.subtree_solve_panels > 0) {
    const size_t cap = std::min<size_t>(cnl::max_lds_bytes(), (size_t)160 * 1024);
    bool any = false;
    for (int s = 0; s < nst; s++) {
      const size_t need = (size_t)cnl::subtree_solve_lds_elems(h->gstage_fmax[s]) * h->esz();
      if (need <= cap) { h->gstage_solve_lds[s] = (int32_t)need; any = true; }
    }
    if (any) h->solve_panels = o.subtree_solve_panels;   // (no stage fits: every launch is the unpanelled one, and the handle reports 0)
  }
  return CNL_OK;
}

// The register-front kernel for a handle of either element type.  A Float32 general handle (tuning float32_register_front) is
// asked with its 4-byte elements: every size "in doubles" of DevPlan2 then counts floats, the wavefront's LDS block and the global
// scratch are sized in floats, and the 32-bit byte offsets of the kernel reach twice as many elements.  Its plan has no dense route
// and lean stays off; direct records only with tuning float32_direct_records, and then v2_solve by the Float64 rule (DESIGN section
// 9.4); tasks, and with them the staged state, only with tuning float32_staged; dataflow counters, the
// in-kernel ladder and lean by the Float64 rules only with tuning float32_latency on top.
int setup_v2(cnl_handle* h) {
  const cnl::Plan& P = h->plan->P;
  h->use_v2 = false;
  const cnl::Tuning& o = h->plan->opt;
  const size_t esz = h->esz();
  if (!P.v2_ok || !o.register_front) return CNL_OK;
  // (a float plan with tasks is the latency plan of tuning float32_staged, f32_general_plan: staged below by the Float64 conditions, one
  //  launch per stage; with tuning float32_latency on top also dataflow, the fused ladder and lean)
  if (h->f32 && !P.tasks.empty() && !o.float32_staged) return CNL_OK;
  if (!h->f32 && !h->plan->gpos.empty() && (o.general_dense == 2 || (h->plan->prefer_dense && h->batch <= 16))) return CNL_OK;  // the dense route (capi_plan.cpp, plan_create_impl); 2: wherever it is possible
  cnl::DevPlan2& d = h->dp2;
  // streams are over-read by the prefetcher: pad with zeros
  std::vector<int32_t> rec(P.rec), brec(P.brec);
  rec.resize(rec.size() + 2048, 0);
  brec.resize(brec.size() + 2048, 0);
  int rc;
  if ((rc = upload(h, rec, &d.rec))) return rc;
  if ((rc = upload(h, brec, &d.brec))) return rc;
  d.nsuper = P.nsuper; d.N = (int32_t)P.N; d.nnz = (int32_t)P.nnz; d.rho_begin = P.rho_begin; d.nvar = (int32_t)P.nvar;
  d.N0 = (int32_t)P.N;
  d.reccap = (P.rec_maxlen + 64 + 3) & ~3;  // + slack: the product loop reads up to 48 words past a list
  d.breccap = (P.brec_maxlen + 3) & ~3;
  d.recwords = std::max(d.reccap, 2 * d.breccap);
  d.u2_peak = h->f32 ? (P.u2_peak + 1) & ~1 : P.u2_peak;   // (float: the image behind the stack is zeroed in 8-byte pairs)
  // (round 5, found by the randomised run with lds_pad = 0: the out-of-line elimination of a class-64 front publishes its pivot row at
  //  lb[0 .. 65] of the staging area — lanes beyond the pivot park their value at index TE + 1 —, two doubles more than the 64 reserved
  //  here; without padding between the problems they landed in the next problem's update stack)
  d.jraw_off = (int32_t)((d.u2_peak + std::max<int64_t>(P.fs2_max, 72) + 1) & ~(int64_t)1);
  d.bpanel_off = (int32_t)((P.bwd_peak + 2 + 1) & ~(int64_t)1);  // end of the backward sweep's x stack
  // the raw-value area (128 doubles per problem) is needed only by fast fronts whose products come as lists (plan.h: RF_ROWS)
  int64_t prob = std::max<int64_t>((int64_t)d.jraw_off + (P.rec_direct && P.listprod_fronts > 0 ? 128 : 0), (int64_t)d.bpanel_off);
  // per-problem areas 32 banks apart modulo 64 (prob_doubles = 16 mod 32): the 16 lanes of two neighbouring problems
  // then touch disjoint LDS banks when they read the same row of their images (env CNL_LDS_PAD=0 disables)
  prob = (prob + 1) & ~(int64_t)1;
  const int64_t padm = h->f32 ? 64 : 32;   // (elements: 32 banks of 4 bytes are 16 doubles or 32 floats)
  if (o.lds_pad) while (prob % padm != padm / 2) prob += 2;
  d.prob_doubles = (int32_t)prob;
  d.gs_doubles = P.gs_doubles + 64;
  d.lsize = h->dp.lsize;  // padded stride, see cnl_create
  d.vstride = h->dp.vstride; d.rstride = h->dp.rstride; d.dstride = h->dp.dstride;
  if (P.rec_direct) {  // the assembly lists address the caller's arrays
    d.nnz = P.nnz_outer; d.rho_begin = P.nnz_outer - (int32_t)P.nvar;
    d.vstride = P.nnz_outer; d.rstride = P.n_outer;
    d.N0 = P.n_outer;
    if (P.d_outer) d.dstride = P.n_outer;
    d.count_d = P.d_owned == (int64_t)h->plan->C.r_dsrc.size() ? 1 : 0;  // every condensed pivot is staged by some front
  }
  // the kernel addresses vals / rhs / L of the 4 problems of a wave with 32-bit byte offsets from the first one
  if (4 * esz * (uint64_t)std::max<int64_t>({d.lsize, d.vstride, d.rstride, d.dstride, (int64_t)d.nnz + d.N0}) >= (1ull << 32)) return CNL_OK;
  const size_t wave_bytes = (size_t)d.recwords * 4 + (4 * (size_t)d.prob_doubles) * esz + 128;   // + 128: counters, flags, slow_front's scalars (kernels2.hip)
  size_t maxlds = std::min<size_t>(cnl::max_lds_bytes(), 160 * 1024);
  if (wave_bytes + 512 > maxlds) return CNL_OK;  // does not fit: stay on v1
  // waves per workgroup: small workgroups give the dispatcher freedom; 2 keeps the launch grid moderate
  int wpb = 1;
  if (o.waves_per_block > 0) wpb = std::max(1, std::min(4, o.waves_per_block));
  while (wpb > 1 && wpb * wave_bytes + 512 > maxlds) wpb--;
  h->wpb2 = wpb;
  h->lds2 = wpb * wave_bytes + 512;
  if ((rc = dalloc_batch(h, &h->d_gs, (size_t)d.gs_doubles))) return rc;
  h->use_v2 = true;
  h->staged = false;
  if ((rc = dalloc(h, &h->d_status, 1))) return rc;
  if (hipMemset(h->d_status, 0, sizeof(int)) != hipSuccess) return fail(CNL_ERR_HIP, "hipMemset failed");
  {
    // wavefronts of this kernel the device holds at once: two per SIMD by the register budget of every instantiation
    // (profiles/r04_kernel_resources.txt), and what the LDS of a CU holds
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) {
      const size_t per_wg = (size_t)wpb * wave_bytes + 512;
      const long long by_lds = (long long)(std::min<size_t>(prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : maxlds, 160 * 1024) / per_wg) * wpb;
      const long long resident = (long long)prop.multiProcessorCount * std::max<long long>(1, std::min<long long>(8, by_lds));
      h->resident_waves = (int)std::min<long long>(resident, 1 << 20);
    }
  }
  // Rounds 4 - 5, for the record (profiles/HISTORY.md 4b item 8, 4c): staged handles on plans with out-of-line front classes (order 17 .. 64) gave
  // history-dependent wrong decisions and memory faults.  Three causes, all found with garbage left in LDS / scratch / registers in
  // front of every launch (CNL_DBG_SCRATCHFILL, CNL_DBG_LDSFILL) and tools/fuzz_parity.py: the update-matrix slots of the global scratch
  // were padded for 16-lane rows whatever the class of the front (analysis.cpp); the class-64 elimination publishes its pivot row two
  // doubles past the LDS staging area (setup above); and — the one that survived both — the compiler placed the register spills of the
  // call to the out-of-line front path IN FRONT of the EXEC restore of the join block behind the lane-divergent `if (dep_wait)`, so a
  // task with nothing to wait for stored no spills and reloaded garbage (kernels2.hip: DEP_WAITING; tools/check_spill_exec.py checks the
  // ISA of every build for the pattern).  No restriction is left: every stageable plan runs staged, with the in-kernel ladder.
  if (!P.tasks.empty() && P.rec_direct && P.d_outer && d.count_d && o.staged) {
    std::vector<int32_t> tk;
    for (const cnl::Task& t : P.tasks) { tk.push_back(t.rec_off); tk.push_back(t.f1 - t.f0); tk.push_back(t.brec_off); tk.push_back(t.is_root); tk.push_back(t.parent); tk.push_back(t.nchild); }
    if ((rc = upload(h, tk, &h->d_tasks))) return rc;
    // dataflow execution: per (task, group of four problems) a count of finished children (forward) and a done flag (backward)
    h->ntasks = (int)P.tasks.size();
    // (measured, tools/sweep_dataflow.py: one system 0.132 against 0.165 ms, eight 0.177 against 0.193 ms; cfg4's pattern with
    //  29 tasks: 32 problems 0.110 against 0.131 ms.  With more wavefronts than about half the machine's slots the waiting ones
    //  crowd out the working ones — cfg3, 501 tasks: sixteen problems 0.233 against 0.196 ms, 256: 82 k against 367 k systems/s —
    //  so only the top stages whose tasks x groups of problems number at most 1024 run that way; env CNL_DATAFLOW_WAVES)
    // a wavefront that waits occupies its slot: never more waiting wavefronts than the device holds at once (the scheme
    // relies on the lowest unfinished workgroup being resident; kernels2.hip)
    h->df_waves = o.dataflow_waves > 0 ? o.dataflow_waves : 1024;
    if (h->resident_waves > 0) h->df_waves = std::min(h->df_waves, h->resident_waves);
    {
      const size_t B = (size_t)h->full_batch, nq = (B + 3) / 4, tq = 2 * (size_t)h->ntasks * nq;
      // (float: one launch per stage only — no dataflow part, d_dep stays null — unless tuning float32_latency brings the Float64 rules)
      const bool dataflow = o.dataflow && (!h->f32 || o.float32_latency);
      const size_t total = 4 * B + (size_t)cnl::LAD_WORDS * nq + tq + 2 + (dataflow ? tq : 0);
      if ((rc = dalloc(h, &h->d_gcnt, total))) return rc;
      // (the head of the block, two ints per problem, is what views address: the other counters are per handle — handle.h, SubBatch)
      if ((rc = register_batch(h, &h->d_gcnt, 2 * sizeof(int)))) return rc;
      if (hipMemset(h->d_gcnt, 0, total * sizeof(int)) != hipSuccess) return fail(CNL_ERR_HIP, "hipMemset failed");
      h->d_lgcnt = h->d_gcnt + 2 * B;
      h->d_lad = h->d_lgcnt + 2 * B;
      h->d_ldep = h->d_lad + (size_t)cnl::LAD_WORDS * nq;
      h->d_stat = h->d_ldep + tq;   // per-call status words (kernels2.hip, spin_until)
      if (dataflow) h->d_dep = h->d_stat + 2;
      h->zero_ints = (long long)total;
    }
    h->stage_ptr = P.stage_ptr;
    h->staged = true;
    // The in-kernel rho ladder needs all tasks of a group of four problems resident at once.  With more groups than the device
    // holds the fused launch is repeated over ranges of groups; beyond four such launches the sequential launch keeps the job
    // (plans of very many tasks on batches that large do not occur: the planner gives large batches few, large tasks).
    h->lad_mode = 0;
    // Plans of a few LARGE tasks (the bidirectional chain of mid-size batches) keep the sequential launch when one fused launch
    // cannot hold the batch: a rung there is the same chain of fronts either way, and two fused launches of two wavefronts per SIMD
    // lose to one sequential launch of one (cfg5 at 4096 problems: 3.9 against 2.9 ms).
    // (float: the problems that fail the attempt climb the ladder in the classic launch behind it; with tuning float32_latency the
    //  rule below, on the fused float instances)
    if ((!h->f32 || o.float32_latency) && o.device_ladder && h->resident_waves >= h->ntasks) {
      const long long slots = h->resident_waves / h->ntasks, nq = (h->batch + 3) / 4;
      const long long launches = (nq + slots - 1) / slots;
      if (launches == 1 || (launches <= 4 && h->ntasks >= 16)) h->lad_mode = o.device_ladder_fused ? 2 : 1;
    }
  }
  h->v2_solve = P.rec_direct && P.d_outer && P.ncls[1] == 0 && P.ncls[2] == 0 && !o.v1_solve;
  // (float: lean instances only behind tuning float32_latency, whose plan_create_impl shaped the plan for them — the key stays in the
  //  options of that latency plan alone, every fallback plan has it cleared: f32_unstaged_options)
  h->lean = (!h->f32 || o.float32_latency) && o.lean_kernel && P.rec_direct && P.d_outer && d.count_d && P.ncls[1] == 0 && P.ncls[2] == 0 && P.listprod_fronts == 0;
  return CNL_OK;
}

// ---- handle creation: what the creators of both element types share ----
// what every creator checks before it analyses anything
int check_batch(int64_t batch) {
  if (batch < 1 || batch > (1 << 24)) return fail(CNL_ERR_ARG, "batch out of range");
  return CNL_OK;
}
int check_device(int device) {
  int ndev = 0;
  const hipError_t ce = hipGetDeviceCount(&ndev);
  if (ce != hipSuccess || ndev == 0)
    return fail(CNL_ERR_HIP, std::string("no HIP device available (this backend has no CPU fallback): hipGetDeviceCount -> ") +
                                 hipGetErrorString(ce) + ", " + std::to_string(ndev) + " device(s)");
  if (device < 0 || device >= ndev) return fail(CNL_ERR_ARG, "device index out of range");
  return CNL_OK;
}

// The band kernels for a handle of either element type (h->f32): uploads the program, chooses the problems per workgroup and
// allocates the factor records; h->band says whether they serve the handle.  They do not where the program does not fit them —
// *unfit then names the reason and the caller decides what that means (a Float64 handle has the register-front kernel, a Float32
// handle nothing).  An option that asks for an instance that does not exist is an error.
int setup_band(cnl_handle* h, const cnl::BandPlan& Bp0, const char** unfit) {
  const cnl_plan* plan = h->plan;
  const int esz = (int)h->esz();
  const int64_t batch = h->batch;
  int rc;
  h->band_npiece = Bp0.npiece;
  const bool wide = Bp0.npiece != cnl::BAND_NPIECE;
  cnl::BandDev& bd = h->bd;
  // 16 problems per workgroup (two workgroups = four wavefronts per CU: one per SIMD) up to the 8192 problems that fills; above,
  // 32 per workgroup (the LDS of a CU holds two such workgroups: 16384 problems resident) — tools/time_band.py
  // (wide program, Float64: 16 at every batch — three workgroups per CU hold 48 problems where one of 32 would hold 32, and the
  // 32-problem instance would spill; band.hip, band_wide_has)
  h->band_nl = plan->opt.band_problems_per_group > 0 ? plan->opt.band_problems_per_group
                                                     : (batch > 8192 && (!wide || cnl::band_wide_has(esz, 32)) ? 32 : 16);
  if (h->band_nl != 8 && h->band_nl != 16 && h->band_nl != 32) return fail(CNL_ERR_ARG, "band_problems_per_group must be 8, 16 or 32");
  if (wide && !cnl::band_wide_has(esz, h->band_nl))   // (there is a wide Float32 instance for each of the three)
    return fail(CNL_ERR_ARG, "band_problems_per_group = 32: the wide band program (20 operand pieces) has Float64 kernels for 8 and 16 problems per workgroup only");
  // The resident form of the 15-piece program where the plan has it and the handle is the one it was built for: Float64, `vals`
  // interleaved (an aligned block is then one 64-byte run per problem), 32 problems per workgroup (the instance that stores factor
  // records directly, so that the out ring's LDS is free in the forward sweep).  Same steps and arithmetic: bit-equal outputs.
  h->band_resident = !h->f32 && !wide && h->band_nl == 32 && plan->opt.batch_layout == CNL_LAYOUT_INTERLEAVED && plan->band_res.B.ok;
  const cnl::BandPlan& Bp = h->band_resident ? plan->band_res.B : Bp0;
  // ... and its mover table where it has one (band.h, BAND_MK_*; tuning band_mover_table = 0: none): the table's words take the place
  // of the piece descriptors in the uploaded epoch blocks, which is the whole difference for the device
  h->band_mover = h->band_resident && plan->opt.band_mover_table && Bp.mover_ok;
  // ... under the cache policy of tuning band_cache_policy (band.hip, BAND_POL_*): that instance has them, every other ignores the key
  h->band_policy = h->band_mover ? plan->opt.band_cache_policy : 0;
  for (int q = 0; q < Bp.nparts; q++) {
    if ((rc = upload(h, Bp.part[q].fops, &bd.fops[q]))) return rc;
    if ((rc = upload(h, Bp.part[q].bops, &bd.bops[q]))) return rc;
    if (h->band_mover) {
      std::vector<int32_t> ep = Bp.part[q].epochs;
      static_assert(cnl::BE_BP == cnl::BE_FP + cnl::BAND_NPIECE && cnl::BAND_MOV_EW == 2 * cnl::BAND_NPIECE, "the two piece lists of an epoch block are adjacent");
      for (int32_t e = 0; e < Bp.part[q].nepochs; e++)
        std::copy_n(Bp.part[q].mover.begin() + (size_t)e * cnl::BAND_MOV_EW, cnl::BAND_MOV_EW, ep.begin() + (size_t)e * cnl::BAND_EW + cnl::BE_FP);
      if ((rc = upload(h, ep, &bd.epochs[q]))) return rc;
    } else if ((rc = upload(h, Bp.part[q].epochs, &bd.epochs[q]))) return rc;
    if ((rc = upload(h, Bp.part[q].borders, &bd.borders[q]))) return rc;
    bd.nsteps[q] = Bp.part[q].nsteps; bd.nepochs[q] = Bp.part[q].nepochs; bd.loff[q] = Bp.part[q].loff;
  }
  bd.nparts = Bp.nparts; bd.m0 = Bp.m0; bd.n = Bp.n; bd.N = Bp.N; bd.nnz = Bp.nnz; bd.nvar = (int32_t)plan->nvar; bd.lsize = Bp.lsize;
  // 32-bit byte offsets inside a workgroup's problems
  const uint64_t span = (uint64_t)esz * (uint64_t)h->band_nl * (uint64_t)std::max<int64_t>({plan->nnz, plan->N, bd.lsize});
  if (span >= (1ull << 32)) { *unfit = "the arrays of a workgroup's problems span 4 GB or more (32-bit offsets of the band kernels)"; return CNL_OK; }
  if (cnl::band_lds_bytes(bd.nparts, h->band_nl, esz, h->band_npiece) > std::min<size_t>(cnl::max_lds_bytes(), 160 * 1024)) {
    *unfit = "the band kernels' LDS does not fit a workgroup";
    return CNL_OK;
  }
  // (+ 32 problems: the band kernels interleave the records of a workgroup's problems, the last workgroup's region is a whole one)
  const size_t lpad = 32 * (size_t)bd.lsize + 64;
  if ((rc = dalloc_batch(h, &h->d_Lband, (size_t)bd.lsize, lpad))) return rc;
  if (hipMemset(h->d_Lband, 0, ((size_t)h->full_batch * (size_t)bd.lsize + lpad) * (size_t)esz) != hipSuccess) return fail(CNL_ERR_HIP, "hipMemset failed");
  h->band = true;
  return CNL_OK;
}

// cnl_options.batch_layout: the interleaved layout is the band kernels' (groups of 32 problems = one workgroup of the 32-problem
// instantiation)
int setup_layout(cnl_handle* h) {
  const cnl::Tuning& o = h->plan->opt;
  if (o.batch_layout == CNL_LAYOUT_PROBLEM_MAJOR) return CNL_OK;
  if (o.batch_layout != CNL_LAYOUT_INTERLEAVED) return fail(CNL_ERR_ARG, "cnl_options.batch_layout: unknown layout");
  if (!h->band)
    return fail(CNL_ERR_ARG, "batch_layout = CNL_LAYOUT_INTERLEAVED needs a handle the band kernels serve "
                             "(band-structured pattern, throughput plan, cnl_options.band_kernel != 0; csrc/band.h)");
  h->layout = 1 | (o.band_rhs_interleaved ? 2 : 0);
  return CNL_OK;
}

// ---- cnl_options.batch_layout = CNL_LAYOUT_INTERLEAVED: lengths and conversions (csrc/band.h: band_il_index) ----
int layout_rowlen(const cnl_handle* h, int which, int64_t* len) {
  if (which == 0) *len = h->djt.nnz;
  else if (which == 1) *len = (int64_t)h->djt.nvar + h->djt.nequ + h->djt.ncon;
  else return fail(CNL_ERR_ARG, "which: 0 = vals, 1 = an N-vector per problem (rhs)");
  return CNL_OK;
}
template <class T>
int convert_layout(cnl_handle* h, int which, const T* src, T* dst, int to_interleaved, void* stream) {
  if (!h || !src || !dst) return fail(CNL_ERR_ARG, "null argument");
  if (src == dst) return fail(CNL_ERR_ARG, "the conversion is not in place");
  int64_t len = 0;
  if (int rc = layout_rowlen(h, which, &len)) return rc;
  HIPCHK(hipSetDevice(h->device));
  hipError_t e;
  if constexpr (sizeof(T) == 4) e = cnl::launch_interleave_f32(src, dst, (int)h->batch, (int)h->full_batch, len, to_interleaved, (hipStream_t)stream);
  else e = cnl::launch_interleave(src, dst, (int)h->batch, (int)h->full_batch, len, to_interleaved, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CNL_ERR_HIP, std::string("interleave: ") + hipGetErrorString(e));
  return CNL_OK;
}

// Rows f1 / f4 (both element types): the transposed-Jacobian lists of the pattern (DevJt), the column tiles of row f1 and the J_F / J_c
// segments of `vals`.  Pattern-sized, shared by all problems of the handle.
int build_row_lists(cnl_handle* h, const cnl_plan* plan, const int64_t* rows1, const int64_t* cols1) {
  const int64_t N = plan->N, nnz = plan->nnz, nvar = plan->nvar, nequ = plan->nequ, ncon = plan->ncon;
  int rc = CNL_OK;
  // transposed-Jacobian lists from the pattern: entries with column <= nvar < row, in COO order per column
  std::vector<int32_t> ptrF(nvar + 1, 0), ptrC(nvar + 1, 0), slotF, idxF, slotC, idxC;
  for (int64_t e = 0; e < nnz; e++) {
    const int64_t r0 = rows1[e] - 1, c0 = cols1[e] - 1;
    if (c0 < nvar && r0 >= nvar) (r0 < nvar + nequ ? ptrF : ptrC)[c0 + 1]++;
  }
  for (int64_t j2 = 0; j2 < nvar; j2++) { ptrF[j2 + 1] += ptrF[j2]; ptrC[j2 + 1] += ptrC[j2]; }
  slotF.resize(ptrF[nvar]); idxF.resize(ptrF[nvar]); slotC.resize(ptrC[nvar]); idxC.resize(ptrC[nvar]);
  std::vector<int32_t> fillF(ptrF.begin(), ptrF.end() - 1), fillC(ptrC.begin(), ptrC.end() - 1);
  for (int64_t e = 0; e < nnz; e++) {
    const int64_t r0 = rows1[e] - 1, c0 = cols1[e] - 1;
    if (!(c0 < nvar && r0 >= nvar)) continue;
    if (r0 < nvar + nequ) { const int32_t q = fillF[c0]++; slotF[q] = (int32_t)e; idxF[q] = (int32_t)(r0 - nvar); }
    else { const int32_t q = fillC[c0]++; slotC[q] = (int32_t)e; idxC[q] = (int32_t)(r0 - nvar - nequ); }
  }
  cnl::DevJt& J = h->djt;
  if ((rc = upload(h, ptrF, &J.ptrF))) return rc;
  // the J_F / J_c entries as segments of `vals` (the reference's 7-segment layout, src/CaNNOLeS.jl:256-315): rows f1 / f4 can
  // read them from the model's arrays instead (cnl_residual_vectors_jac_dev) when each kind occupies one run of slots
  {
    auto run = [](const std::vector<int32_t>& sl, int64_t& lo) {
      if (sl.empty()) { lo = 0; return true; }
      const auto mm = std::minmax_element(sl.begin(), sl.end());
      lo = *mm.first;
      return (int64_t)*mm.second - *mm.first + 1 == (int64_t)sl.size();
    };
    h->jac_segments = run(slotF, h->jf_lo) && run(slotC, h->jc_lo);
    h->jf_n = (int64_t)slotF.size(); h->jc_n = (int64_t)slotC.size();
  }
  if ((rc = upload(h, slotF, &J.slotF))) return rc;
  if ((rc = upload(h, idxF, &J.idxF))) return rc;
  if ((rc = upload(h, ptrC, &J.ptrC))) return rc;
  if ((rc = upload(h, slotC, &J.slotC))) return rc;
  if ((rc = upload(h, idxC, &J.idxC))) return rc;
  {
    // J_c by rows (CGLS, row f4)
    std::vector<int32_t> rptr(ncon + 1, 0), rslot(slotC.size()), rcol(slotC.size());
    for (int64_t j2 = 0; j2 < nvar; j2++) for (int32_t q = ptrC[j2]; q < ptrC[j2 + 1]; q++) rptr[idxC[q] + 1]++;
    for (int64_t k2 = 0; k2 < ncon; k2++) rptr[k2 + 1] += rptr[k2];
    std::vector<int32_t> fillr(rptr.begin(), rptr.end() - 1);
    for (int64_t j2 = 0; j2 < nvar; j2++)
      for (int32_t q = ptrC[j2]; q < ptrC[j2 + 1]; q++) { const int32_t w = fillr[idxC[q]]++; rslot[w] = slotC[q]; rcol[w] = (int32_t)j2; }
    if ((rc = upload(h, rptr, &J.rptrC))) return rc;
    if ((rc = upload(h, rslot, &J.rslotC))) return rc;
    if ((rc = upload(h, rcol, &J.rcolC))) return rc;
  }
  J.nvar = (int32_t)nvar; J.nequ = (int32_t)nequ; J.ncon = (int32_t)ncon; J.N = (int32_t)N; J.nnz = (int32_t)nnz;
  // (round 5) column tiles of row f1 (kernels.h: DevJt::rv_*): the slot / index ranges of every tile of RVT_COLS columns
  if (plan->opt.f1_tiles && nvar > 0) {
    const int32_t nt = (int32_t)((nvar + cnl::RVT_COLS - 1) / cnl::RVT_COLS);
    std::vector<int32_t> tiles((size_t)nt * cnl::RVT_TW, 0);
    std::vector<uint32_t> table((size_t)nt * (cnl::RVT_KF + cnl::RVT_KC + 1) * cnl::RVT_COLS, 0u);
    bool ok = true;
    int32_t lds_max = 0;
    for (int32_t t = 0; t < nt && ok; t++) {
      const int64_t c0 = (int64_t)t * cnl::RVT_COLS, c1 = std::min<int64_t>(nvar, c0 + cnl::RVT_COLS);
      int32_t fslo = INT32_MAX, fshi = -1, rlo = INT32_MAX, rhi = -1, cslo = INT32_MAX, cshi = -1, llo = INT32_MAX, lhi = -1;
      for (int32_t q = ptrF[c0]; q < ptrF[c1]; q++) { fslo = std::min(fslo, slotF[q]); fshi = std::max(fshi, slotF[q]); rlo = std::min(rlo, idxF[q]); rhi = std::max(rhi, idxF[q]); }
      for (int32_t q = ptrC[c0]; q < ptrC[c1]; q++) { cslo = std::min(cslo, slotC[q]); cshi = std::max(cshi, slotC[q]); llo = std::min(llo, idxC[q]); lhi = std::max(lhi, idxC[q]); }
      int32_t* T = &tiles[(size_t)t * cnl::RVT_TW];
      T[cnl::RVT_FSLO] = fshi < 0 ? 0 : fslo; T[cnl::RVT_WF] = fshi < 0 ? 0 : fshi - fslo + 1;
      T[cnl::RVT_RLO] = rhi < 0 ? 0 : rlo;   T[cnl::RVT_WR] = rhi < 0 ? 0 : rhi - rlo + 1;
      T[cnl::RVT_CSLO] = cshi < 0 ? 0 : cslo; T[cnl::RVT_WC] = cshi < 0 ? 0 : cshi - cslo + 1;
      T[cnl::RVT_LLO] = lhi < 0 ? 0 : llo;   T[cnl::RVT_WL] = lhi < 0 ? 0 : lhi - llo + 1;
      if (T[cnl::RVT_WF] > cnl::RVT_MAXF || T[cnl::RVT_WR] > cnl::RVT_MAXR || T[cnl::RVT_WC] > cnl::RVT_MAXC || T[cnl::RVT_WL] > cnl::RVT_MAXL) { ok = false; break; }
      auto even = [](int32_t w) { return (w + 3) & ~1; };   // a window and the double its 16-byte alignment may put in front
      lds_max = std::max(lds_max, even(T[cnl::RVT_WF]) + even(T[cnl::RVT_WR]) + even(T[cnl::RVT_WC]) + even(T[cnl::RVT_WL]));
      uint32_t* tab = &table[(size_t)t * (cnl::RVT_KF + cnl::RVT_KC + 1) * cnl::RVT_COLS];
      for (int64_t c = c0; c < c1; c++) {
        const int32_t nF = ptrF[c + 1] - ptrF[c], nC = ptrC[c + 1] - ptrC[c];
        if (nF > 255 || nC > 255) { ok = false; break; }
        for (int32_t u = 0; u < std::min(nF, cnl::RVT_KF); u++)
          tab[(size_t)u * cnl::RVT_COLS + (c - c0)] = (uint32_t)(slotF[ptrF[c] + u] - T[cnl::RVT_FSLO]) | (uint32_t)(idxF[ptrF[c] + u] - T[cnl::RVT_RLO]) << 16;
        for (int32_t u = 0; u < std::min(nC, cnl::RVT_KC); u++)
          tab[(size_t)(cnl::RVT_KF + u) * cnl::RVT_COLS + (c - c0)] = (uint32_t)(slotC[ptrC[c] + u] - T[cnl::RVT_CSLO]) | (uint32_t)(idxC[ptrC[c] + u] - T[cnl::RVT_LLO]) << 16;
        tab[(size_t)(cnl::RVT_KF + cnl::RVT_KC) * cnl::RVT_COLS + (c - c0)] = (uint32_t)nF | (uint32_t)nC << 8;
      }
    }
    if (ok) {
      // the residual rows a tile has in LDS anyway are the rows whose primal entry F - r it writes: possible when the tiles' row
      // ranges are ordered and cover 0 .. nequ without gaps (a band); otherwise tiles of rows of their own follow the column tiles
      bool own = nequ > 0;
      int32_t prev = 0;
      for (int32_t t = 0; t < nt && own; t++) {
        int32_t* T = &tiles[(size_t)t * cnl::RVT_TW];
        const int32_t lo = T[cnl::RVT_RLO], hi = lo + T[cnl::RVT_WR];
        const int32_t next_lo = t + 1 < nt ? tiles[(size_t)(t + 1) * cnl::RVT_TW + cnl::RVT_RLO] : (int32_t)nequ;
        const int32_t own_hi = t + 1 < nt ? std::min(hi, std::max(next_lo, prev)) : (int32_t)nequ;
        if (prev < lo || own_hi > hi || own_hi < prev) { own = false; break; }
        T[cnl::RVT_OWNLO] = prev; T[cnl::RVT_OWNHI] = own_hi;
        prev = own_hi;
      }
      if (own && prev != nequ) own = false;
      if (!own) for (int32_t t = 0; t < nt; t++) tiles[(size_t)t * cnl::RVT_TW + cnl::RVT_OWNLO] = tiles[(size_t)t * cnl::RVT_TW + cnl::RVT_OWNHI] = 0;
      if ((rc = upload(h, tiles, &J.rv_tiles))) return rc;
      if ((rc = upload(h, table, &J.rv_table))) return rc;
      J.rv_ntiles = nt; J.rv_lds_doubles = lds_max;
      J.rv_primal_tiles = own ? 0 : (int32_t)((nequ + cnl::RVT_PROWS - 1) / cnl::RVT_PROWS);
    }
    if (std::getenv("CNL_VERBOSE")) fprintf(stderr, "[cnl] row f1: %s\n", ok ? "column tiles" : "gather kernel (a tile's windows exceed the limits)");
  }
  return CNL_OK;
}

int create_tuned(cnl_handle** hout, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar,
                 int64_t nequ, int64_t ncon, int64_t batch, int device, const cnl::Tuning& o) {
  *hout = nullptr;
  if (int rc = check_batch(batch)) return rc;
  if (int rc = check_device(device)) return rc;
  cnl_plan* plan = nullptr;
  // small batches cannot fill the chip with one wavefront per four problems: plan for latency (bushy order, tasks)
  int rc = plan_create_tuned(&plan, N, nnz, rows1, cols1, nvar, nequ, ncon, batch, o);
  if (rc) return rc;
  return create_from_plan(hout, plan, rows1, cols1, batch, device);
}

// the device copy of the general kernel's plan (kernels.h: DevPlan), either element type: index data, sizes and strides in elements
int upload_dev_plan(cnl_handle* h) {
  const cnl_plan* plan = h->plan;
  const cnl::Plan& P = plan->P;
  cnl::DevPlan& dp = h->dp;
  int rc;
  if ((rc = upload(h, P.fronts, &dp.fronts))) return rc;
  if ((rc = upload(h, P.seg_ptr, &dp.seg_ptr))) return rc;
  if ((rc = upload(h, P.asm_pos, &dp.asm_pos))) return rc;
  if ((rc = upload(h, P.asm_src, &dp.asm_src))) return rc;
  if ((rc = upload(h, P.child_idx, &dp.child_idx))) return rc;
  if ((rc = upload(h, P.rel_idx, &dp.rel_idx))) return rc;
  if ((rc = upload(h, P.perm, &dp.perm))) return rc;
  dp.nsuper = P.nsuper; dp.N = (int32_t)P.N; dp.nnz = (int32_t)P.nnz; dp.rho_begin = P.rho_begin;
  dp.nvar = (int32_t)P.nvar; dp.nequ = (int32_t)P.nequ; dp.ncon = (int32_t)P.ncon;
  dp.fmax = (P.fmax + 1) & ~1;
  // factor storage stride per problem: + 16 zero doubles that are never written.  The solve sweeps read a panel row as 16
  // lanes, so the last rows of a problem's factor are over-read by up to 15 entries, which are multiplied by zeros; without
  // the pad they would be the first entries of the NEXT problem's factor, and a NaN / Inf there (a neighbour whose
  // factorisation broke down) would turn 0 * x into NaN in this problem's solution
  dp.lsize = P.lsize + 16;
  const cnl::Cond& C = plan->C;
  dp.vstride = C.active ? C.cstride : plan->nnz;
  dp.rstride = C.active ? C.cstride : plan->N;
  dp.dstride = C.active ? C.N2 : plan->N;
  return CNL_OK;
}

// the device copy of the condensation lists (kernels.h: DevCond) and the per-problem inertia counts of the condensed pivots, either
// element type: index data only.  (d_cbuf / d_d2 — the condensed buffer and the reduced solution of the stand-alone condensation
// passes — are allocated by the creators, in their element type.)
int upload_dev_cond(cnl_handle* h) {
  const cnl_plan* plan = h->plan;
  const cnl::Cond& C = plan->C;
  const int64_t N = plan->N, nnz = plan->nnz, nvar = plan->nvar;
  int rc;
  cnl::DevCond& dc = h->dc;
  std::vector<int32_t> cidx(N, -1);
  for (size_t q = 0; q < C.r_orig.size(); q++) cidx[C.r_orig[q]] = (int32_t)q;
  if ((rc = upload(h, C.c_ptr, &dc.c_ptr))) return rc;
  if ((rc = upload(h, C.c_a, &dc.c_a))) return rc;
  if ((rc = upload(h, C.c_b, &dc.c_b))) return rc;
  if ((rc = upload(h, C.c_d, &dc.c_d))) return rc;
  if ((rc = upload(h, C.c_order, &dc.c_order))) return rc;
  if ((rc = upload(h, C.ch_slot, &dc.ch_slot))) return rc;
  if ((rc = upload(h, C.ch_rng, &dc.ch_rng))) return rc;
  if ((rc = upload(h, C.ch_tile, &dc.ch_tile))) return rc;
  if ((rc = upload(h, C.rng_start, &dc.rng_start))) return rc;
  if ((rc = upload(h, C.rng_len, &dc.rng_len))) return rc;
  if ((rc = upload(h, C.c_la, &dc.c_la))) return rc;
  if ((rc = upload(h, C.c_lb, &dc.c_lb))) return rc;
  if ((rc = upload(h, C.c_ld, &dc.c_ld))) return rc;
  if ((rc = upload(h, C.ch_tptr, &dc.ch_tptr))) return rc;
  if ((rc = upload(h, C.tile_src, &dc.tile_src))) return rc;
  if ((rc = upload(h, C.c_pack, &dc.c_pack))) return rc;
  dc.tile_max = C.tile_max; dc.chunk_ncon_max = C.chunk_ncon_max; dc.chunk_nslot_max = C.chunk_nslot_max; dc.tiled_ok = C.tiled_ok ? 1 : 0;
  if ((rc = upload(h, C.r_dsrc, &dc.r_dsrc))) return rc;
  if ((rc = upload(h, C.r_ptr, &dc.r_ptr))) return rc;
  if ((rc = upload(h, C.r_jsrc, &dc.r_jsrc))) return rc;
  if ((rc = upload(h, C.r_jx, &dc.r_jx))) return rc;
  if ((rc = upload(h, C.red_of, &dc.red_of))) return rc;
  if ((rc = upload(h, cidx, &dc.cidx_of))) return rc;
  if ((rc = upload(h, C.orig_of, &dc.orig_of))) return rc;
  if ((rc = upload(h, C.r_orig, &dc.r_orig))) return rc;
  dc.N = (int32_t)N; dc.nnz = (int32_t)nnz; dc.nvar = (int32_t)nvar; dc.N2 = (int32_t)C.N2; dc.ncs = (int32_t)C.ncs;
  dc.ncond = (int32_t)C.r_orig.size(); dc.cstride = C.cstride;
  if ((rc = dalloc_batch(h, &h->d_xpos, 1))) return rc;
  return dalloc_batch(h, &h->d_xzer, 1);
}

// The resident condense kernel for a Float32 general handle (kernels.h: DevCondEll), where it pays and fits: the tiled kernel stages
// sum(ch_tile) elements per problem, the resident one nnz + N; a dense Jacobian makes the former many times the latter (every chunk's
// tile holds the whole Jacobian), and where the tile fits no LDS at all the plain kernel gathers from L2 per slot.
int setup_cond_resident(cnl_handle* h) {
  const cnl_plan* plan = h->plan;
  const cnl::Cond& C = plan->C;
  const int64_t nsrc = plan->nnz + plan->N, nslot = (int64_t)C.c_ptr.size() - 1;
  if (plan->opt.float32_condense != 1 || nsrc >= 65535) return CNL_OK;
  if (cnl::condense_resident_lds_bytes(plan->nnz, plan->N) > std::min<size_t>(cnl::max_lds_bytes(), 160 * 1024)) return CNL_OK;
  int64_t staged = 0;
  for (int32_t t : C.ch_tile) staged += t;
  if (C.tiled_ok && staged <= 4 * nsrc) return CNL_OK;   // the tiled kernel's chunks are what they were made for
  constexpr int NT = cnl::COND_RES_THREADS;
  const int64_t nblk = (nslot + NT - 1) / NT;
  std::vector<int32_t> blk_ptr(nblk + 1, 0);
  for (int64_t j = 0; j < nblk; j++) {
    int32_t len = 0;
    for (int64_t s = j * NT; s < std::min<int64_t>(nslot, (j + 1) * NT); s++) len = std::max(len, C.c_ptr[s + 1] - C.c_ptr[s]);
    const int64_t next = (int64_t)blk_ptr[j] + (int64_t)len * NT;
    if (next >= ((int64_t)1 << 30)) return CNL_OK;
    blk_ptr[j + 1] = (int32_t)next;
  }
  std::vector<uint64_t> pack((size_t)blk_ptr[nblk], 0);
  for (int64_t s = 0; s < nslot; s++) {
    const int64_t j = s / NT, t = s % NT;
    for (int32_t c = C.c_ptr[s]; c < C.c_ptr[s + 1]; c++)
      pack[(size_t)blk_ptr[j] + (size_t)(c - C.c_ptr[s]) * NT + t] =
          (uint64_t)C.c_a[c] | ((uint64_t)(C.c_b[c] + 1) << 16) | ((uint64_t)(C.c_b[c] < 0 ? 0 : C.c_d[c] + 1) << 32);
  }
  int rc;
  if ((rc = upload(h, pack, &h->dce.pack))) return rc;
  if ((rc = upload(h, blk_ptr, &h->dce.blk_ptr))) return rc;
  h->dce.c_ptr = h->dc.c_ptr;
  h->dce.nslot = (int32_t)nslot; h->dce.nnz = (int32_t)plan->nnz; h->dce.N = (int32_t)plan->N; h->dce.cstride = C.cstride;
  h->cond_resident = true;
  return CNL_OK;
}

// ---- the skeleton the creators share: a fresh handle on `plan` (which it owns from here on: cnl_destroy frees both), `device` current
int new_handle(cnl_handle** hout, cnl_plan* plan, int64_t batch, int device, bool f32, bool f32_general) {
  cnl_handle* h = new cnl_handle();
  h->plan = plan; h->device = device; h->batch = h->full_batch = batch; h->f32 = f32; h->f32_general = f32_general;
  if (hipSetDevice(device) != hipSuccess) { cnl_destroy(h); return fail(CNL_ERR_HIP, "hipSetDevice failed"); }
  *hout = h;
  return CNL_OK;
}
// Storage of the general and register-front kernels, in the handle's element type: the factor panels, zero-filled (the pad of every
// problem stays zero) and padded — the row prefetch of the backward pass reads (never uses) a little past a panel —, and the global
// work area where it is not in LDS.  (A band handle keeps the pad alone: create_from_plan.)
int alloc_factor_storage(cnl_handle* h) {
  int rc;
  const size_t lelems = (h->band ? 0 : (size_t)h->full_batch * (size_t)h->dp.lsize) + 4096;
  // (the pad of a band handle is no array of problems — no kernel of such a handle reads d_L —, so there is nothing for a view to move)
  if ((rc = h->band ? dalloc_elems(h, &h->d_L, lelems) : dalloc_batch(h, &h->d_L, (size_t)h->dp.lsize, 4096))) return rc;
  if (hipMemset(h->d_L, 0, lelems * h->esz()) != hipSuccess) return fail(CNL_ERR_HIP, "hipMemset failed");
  if (!h->cfg.lds_work && (rc = dalloc_batch(h, &h->d_scratch, (size_t)h->dp.work_doubles))) return rc;
  return CNL_OK;
}
// the handle's route (call_shape.h: decided here, once, for run() and everything that asks what kind of handle this is), its stream,
// its two timing events and the row lists (rows f1 / f2 / f4, the trial point, the dimensions cnl_layout_len reads)
int finish_handle(cnl_handle* h, const int64_t* rows1, const int64_t* cols1) {
  using cnl::Route;
  h->route = h->band ? Route::Band : h->dense ? Route::Dense : h->gdense ? Route::GeneralDense : !h->plan->C.active ? Route::Plain
             : (h->use_v2 && h->plan->P.rec_direct) ? Route::Direct : Route::Condensed;
  if (hipStreamCreate(&h->stream) != hipSuccess) return fail(CNL_ERR_HIP, "hipStreamCreate failed");
  if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) return fail(CNL_ERR_HIP, "hipEventCreate failed");
  return build_row_lists(h, h->plan, rows1, cols1);
}

}  // namespace

// device state for `batch` problems of an analysed pattern; takes ownership of `plan` (freed with the handle, or here on failure)
int create_from_plan(cnl_handle** hout, cnl_plan* plan, const int64_t* rows1, const int64_t* cols1, int64_t batch, int device) {
  const int64_t N = plan->N, nnz = plan->nnz, nvar = plan->nvar, nequ = plan->nequ, ncon = plan->ncon;
  int rc = CNL_OK;
  cnl_handle* h = nullptr;
  if ((rc = new_handle(&h, plan, batch, device, false, false))) return rc;
  auto bail = [&](int code) { cnl_destroy(h); return code; };
  if ((rc = upload_dev_plan(h))) return bail(rc);
  const cnl::Cond& C = plan->C;
  if (C.active && (rc = upload_dev_cond(h))) return bail(rc);
  if ((rc = choose_config(h))) return bail(rc);
  if ((rc = setup_v2(h))) return bail(rc);
  if (band_program(plan, false).ok && band_wide_serves_f64(plan) && plan->opt.band_kernel && h->use_v2 && !h->staged && h->v2_solve && h->lean && plan->P.back_rows && !plan->latency && !plan->split_mode) {
    // band kernels for newton_system, try_to_factorize and solve_ldl! (csrc/band.h); the wide program where the plan has one.
    // (A program that does not fit them — setup_band — leaves the handle on the register-front kernel.)
    const char* unfit = nullptr;
    if ((rc = setup_band(h, band_program(plan, false), &unfit))) return bail(rc);
  }
  if ((rc = setup_layout(h))) return bail(rc);
  // (d_cbuf / d_d2 only once it is known whether the band kernels serve the handle: they never touch them)
  // Storage only the register-front / general kernels and the stand-alone condensation passes use.  A band handle runs all three
  // calls of the plugin surface on the band kernels (round 6), so it owns the band factor records alone: 0.48 MB per problem of
  // cfg3's size instead of 0.48 + 1.16 (factor panels) + 0.64 (condensed buffer, reduced solution) — 16 384 problems: 29 GB less,
  // and twice the batch fits the 288 GB of a device beside the caller's arrays.
  if (plan->C.active && !h->band) {
    if ((rc = dalloc_batch(h, &h->d_cbuf, (size_t)plan->C.cstride))) return bail(rc);
    if ((rc = dalloc_batch(h, &h->d_d2, (size_t)plan->C.N2))) return bail(rc);
  }
  if (plan->split_mode && h->staged) {
    // x groups of four problems on the chain (two wavefronts each), the rest on the single stream: 2 x + y = 2048 slots
    const int64_t nquads = (batch + 3) / 4, x = std::max<int64_t>(0, 2048 - nquads);
    h->split_staged = std::min<int64_t>(batch, 4 * x);
    if (h->plan->opt.split_batch == 1 && batch <= 6400) {
      // two halves on the chain (multiples of four problems), sequentially — measured against chain + single stream concurrently
      // (cfg3's size, same box, k systems/s): 4608: 768 / 707, 5120: 836 / 790, 6144: 931 / 898, 6656: 912 / ~935, 7168: 956 / 959,
      // 7424: 904 / ~965 — halves up to 6400 problems (see run_split)
      h->split_halves = true;
      h->split_staged = (((batch + 1) / 2) + 3) & ~(int64_t)3;
    }
    if (h->split_staged == 0) h->staged = false;  // the whole batch on the single stream
    // a remainder of at most a quarter of the machine-filling batch: its own handle with its own (many-part) plan — run_split
    const int64_t smb = ((plan->opt.staged_max_batch > 0 ? plan->opt.staged_max_batch : 4096)) & ~(int64_t)3;
    if (h->staged && plan->opt.split_batch == 1 && plan->opt.split_tail != 0 && batch > smb && batch - smb <= smb / 4) {
      cnl_handle* t = nullptr;
      if (create_tuned(&t, N, nnz, rows1, cols1, nvar, nequ, ncon, batch - smb, device, plan->opt) == CNL_OK) {
        if (t->staged && t->use_v2 && !t->dense && !t->gdense && !t->tail && t->split_staged == 0) {
          h->tail = t; h->split_halves = false; h->split_staged = smb;
        } else {
          cnl_destroy(t);
        }
      }
      if (hipSetDevice(device) != hipSuccess) return bail(fail(CNL_ERR_HIP, "hipSetDevice failed"));
    }
  }
  if (!plan->latency && !plan->split_mode && h->use_v2 && !h->staged && h->resident_waves > 0 && plan->opt.plan_kind == CNL_PLAN_AUTO &&
      plan->opt.split_tail != 0 && plan->opt.force_order[0] == 0 && !plan->D.active && plan->gpos.empty()) {
    // The single stream gives a group of four problems ONE wavefront for all fronts, and the device holds `resident_waves` of
    // them: a batch of k full machine loads + r problems runs k + 1 rounds, the last one for the r problems alone (cfg3's size:
    // 8448 problems 13.0 ms against 7.9 ms for 8192).  The remainder as a batch of its own has a better plan (many parts, the
    // bidirectional chain, ...): it gets a handle of its own, enqueued behind the full loads (run_split).
    // (band kernels: 512 workgroups of 32 problems are resident at once)
    const int64_t cap = h->band ? 16384 : 4 * (int64_t)h->resident_waves, r = batch % cap;
    if (batch > cap && r > 0 && r <= cap - cap / 16 && !h->layout) {   // (an interleaved batch is one array of whole groups)
      cnl_handle* t = nullptr;
      if (create_tuned(&t, N, nnz, rows1, cols1, nvar, nequ, ncon, r, device, plan->opt) == CNL_OK) {
        if (t->staged && t->use_v2 && !t->dense && !t->gdense) { h->tail = t; h->split_staged = batch - r; }
        else cnl_destroy(t);
      }
      if (hipSetDevice(device) != hipSuccess) return bail(fail(CNL_ERR_HIP, "hipSetDevice failed"));
    }
  }
  if (h->plan->D.active) {
    std::string derr;
    int drc = cnl::dense_create(&h->dense, h->plan->D, batch, derr, h->plan->opt.dense_graph != 0, h->plan->opt.dense_syrk_wgs, h->plan->opt.dense_panel_blocks);
    if (drc) return bail(fail(CNL_ERR_HIP, "dense backend: " + derr));
  } else if (!h->plan->gpos.empty() && !h->use_v2 &&
             // S0, S and G in 64 x 64 tiles per problem: small batches always, larger ones while the tiles stay below 8 GB
             // (round 2 stopped at 16 problems; batches of small irregular systems then fell to the general kernel)
             (batch <= 16 || (double)batch * 3.0 * 32768.0 * std::pow(std::ceil((double)h->plan->C.N2 / 64.0), 2) <= 8e9)) {
    std::string derr;
    const cnl::Cond& C2 = h->plan->C;
    h->gops.ns = (int32_t)C2.N2; h->gops.nv = (int32_t)nvar; h->gops.nslots = (int32_t)C2.ncs; h->gops.cstride = C2.cstride;
    if ((rc = upload(h, h->plan->gpos, &h->gops.d_pos))) return bail(rc);
    int drc = cnl::dense_create_general(&h->gdense, (int32_t)C2.N2, (int32_t)nvar, (int32_t)C2.ncs, h->gops.d_pos, batch, derr, h->plan->opt.dense_graph != 0, h->plan->opt.dense_panel_blocks);
    if (drc) return bail(fail(CNL_ERR_HIP, "dense backend: " + derr));
  }
  if ((rc = setup_subtrees(h))) return bail(rc);   // (tuning general_subtrees: where it acts, d_scratch below is the task regions)
  if ((rc = alloc_factor_storage(h))) return bail(rc);   // (band handles: the pad alone, see above)
  if ((rc = alloc_blocked_flags(h))) return bail(rc);
  if ((rc = finish_handle(h, rows1, cols1))) return bail(rc);
  *hout = h;
  return CNL_OK;
}

namespace {

int create_f32_from_plan(cnl_handle** hout, cnl_plan* plan, const int64_t* rows1, const int64_t* cols1, int64_t batch, int device) {
  int rc = CNL_OK;
  cnl_handle* h = nullptr;
  if ((rc = new_handle(&h, plan, batch, device, true, false))) return rc;
  auto bail = [&](int code) { cnl_destroy(h); return code; };
  const char* unfit = nullptr;
  if ((rc = setup_band(h, band_program(plan, true), &unfit))) return bail(rc);   // the wide program where the plan has one
  if (!h->band) {   // the program does not fit the band kernels: refused, or (tuning float32_general) the caller goes on to the general kernel
    *hout = nullptr;
    if (plan->opt.float32_general) { cnl_destroy(h); return CNL_OK; }   // (the plan goes with the handle)
    return bail(fail(CNL_ERR_ARG, std::string("cnl_create_f32: ") + unfit));
  }
  if ((rc = setup_layout(h))) return bail(rc);
  if ((rc = finish_handle(h, rows1, cols1))) return bail(rc);
  *hout = h;
  return CNL_OK;
}

// A Float32 handle on the general multifrontal kernel (tuning float32_general): `plan` is the throughput analysis without condensation,
// or (tuning float32_condense) with it.  The handle owns the device plan, float factor panels (with the zero pad per problem of
// upload_dev_plan), float global scratch where the work area does not fit LDS, and the row lists; on a condensed plan also the
// condensation lists, the inertia counts of the condensed pivots, and the condensed buffer and reduced solution as FLOAT arrays.
// Nothing of the dense or staged state exists for it; the register-front state (setup_v2, in floats) only with tuning
// float32_register_front on a plan whose fronts that kernel takes; the general form of the dense backend (`gdense`, a FLOAT state)
// only with tuning float32_general_dense on a plan it takes.
int create_f32_general_from_plan(cnl_handle** hout, cnl_plan* plan, const int64_t* rows1, const int64_t* cols1, int64_t batch, int device) {
  int rc = CNL_OK;
  cnl_handle* h = nullptr;
  if ((rc = new_handle(&h, plan, batch, device, true, true))) return rc;
  auto bail = [&](int code) { cnl_destroy(h); return code; };
  if (plan->C.active && !plan->opt.float32_condense)
    return bail(fail(CNL_ERR_STATE, "cnl_create_f32: the plan of a Float32 general handle is condensed only with tuning float32_condense = 1"));
  if ((rc = upload_dev_plan(h))) return bail(rc);   // (condensed plan: the strides of vals / rhs / d are those of d_cbuf / d_d2)
  if ((rc = choose_config(h))) return bail(rc);     // (... and the front sizes those of the condensed system)
  if ((rc = setup_layout(h))) return bail(rc);   // (batch_layout = CNL_LAYOUT_INTERLEAVED is the band kernels': CNL_ERR_ARG)
  if (plan->C.active) {
    if ((rc = upload_dev_cond(h))) return bail(rc);
    if ((rc = dalloc_batch(h, &h->d_cbuf, (size_t)plan->C.cstride))) return bail(rc);
    if ((rc = dalloc_batch(h, &h->d_d2, (size_t)plan->C.N2))) return bail(rc);
    if ((rc = setup_cond_resident(h))) return bail(rc);
  }
  // tuning float32_general_dense: the condensed system as ONE dense matrix on the float kernels of csrc/dense_f32.hip (Route::GeneralDense,
  // as a Float64 default handle's), where the analysis kept the slot positions (condensed order 96 .. 4096), a front exceeds order 64
  // (2: whatever the fronts) and the Float64 handle's batch rule holds for S0, S and G in 64 x 64 tiles of 4-byte elements
  const cnl::Cond& C = plan->C;
  const int gd = plan->opt.float32_general_dense;
  // ("a front exceeds order 64" is P.fmax > 64 here and not !P.v2_ok: analysis.cpp defines v2_ok as fmax <= 64 && register_front &&
  // with_rhs_row, and the forced analysis of a Float32 general handle sets register_front = 0, so v2_ok is false for EVERY such plan;
  // fmax > 64 is the clause of v2_ok that speaks about the fronts.  Keep the 64 in step with analysis.cpp.)
  const bool gd_fits = gd && C.active && !plan->gpos.empty() && (gd == 2 || plan->P.fmax > 64) && f32_general_dense_fits(plan, batch);
  // tuning float32_register_front: the register-front kernel in float runs newton_system / try_to_factorize between the passes
  // where the plan's fronts allow it and its LDS block fits; where not, the handle is the float32_condense handle and nothing else
  // (a plan that kernel takes stays on it with float32_general_dense = 1; 2 asks for the dense route wherever it is possible)
  if (plan->opt.float32_register_front && plan->C.active && !(gd == 2 && gd_fits) && (rc = setup_v2(h))) return bail(rc);
  if (gd_fits && !h->use_v2) {
    std::string derr;
    h->gops.ns = (int32_t)C.N2; h->gops.nv = (int32_t)plan->nvar; h->gops.nslots = (int32_t)C.ncs; h->gops.cstride = C.cstride;
    if ((rc = upload(h, plan->gpos, &h->gops.d_pos))) return bail(rc);
    // (tuning dense_graph as on every dense handle: the call sequence is captured and replayed, key mode 16 + mode as in double)
    if (cnl::dense_create_general_f32(&h->gdense, (int32_t)C.N2, (int32_t)plan->nvar, (int32_t)C.ncs, h->gops.d_pos, batch, derr,
                                      plan->opt.dense_graph != 0, plan->opt.dense_panel_blocks))
      return bail(fail(CNL_ERR_HIP, "dense backend (Float32): " + derr));
  }
  if ((rc = setup_subtrees(h))) return bail(rc);   // (tuning float32_subtrees: where it acts, d_scratch below is the task regions, in floats)
  if ((rc = alloc_factor_storage(h))) return bail(rc);
  if ((rc = alloc_blocked_flags(h))) return bail(rc);   // (tuning float32_blocked, float32_subtrees)
  if ((rc = finish_handle(h, rows1, cols1))) return bail(rc);
  *hout = h;
  return CNL_OK;
}

// A Float32 handle on the dense backend (tuning float32_dense): `plan` is the uncondensed throughput analysis of a pattern that
// detect_dense accepted (plan->D).  The three calls of the plugin surface run on the float kernels of csrc/dense_f32.hip (Route::Dense
// at any batch size, as in Float64); the handle is otherwise the Float32 general handle of that plan — device plan, configuration,
// factor storage and row lists in float —, so that everything that asks what kind of handle this is finds what it finds there.
int create_f32_dense_from_plan(cnl_handle** hout, cnl_plan* plan, const int64_t* rows1, const int64_t* cols1, int64_t batch, int device) {
  int rc = CNL_OK;
  cnl_handle* h = nullptr;
  if ((rc = new_handle(&h, plan, batch, device, true, true))) return rc;
  auto bail = [&](int code) { cnl_destroy(h); return code; };
  if ((rc = upload_dev_plan(h))) return bail(rc);
  if ((rc = choose_config(h))) return bail(rc);
  if ((rc = setup_layout(h))) return bail(rc);   // (batch_layout = CNL_LAYOUT_INTERLEAVED is the band kernels': CNL_ERR_ARG)
  std::string derr;
  if (cnl::dense_create_f32(&h->dense, plan->D, batch, derr, plan->opt.dense_graph != 0, plan->opt.dense_syrk_wgs, plan->opt.dense_panel_blocks))
    return bail(fail(CNL_ERR_HIP, "dense backend (Float32): " + derr));
  if ((rc = alloc_factor_storage(h))) return bail(rc);
  if ((rc = finish_handle(h, rows1, cols1))) return bail(rc);
  *hout = h;
  return CNL_OK;
}

// A Float32 general handle off the band kernels, from the caller's options: the dense backend in float where tuning float32_dense finds
// a dense residual block, else the general / register-front / general-dense handle of the plan (what cnl_create_f32_ex does behind
// the band kernels, and all the inner handle of a float32_refine handle is)
int create_f32_general(cnl_handle** hout, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar, int64_t nequ, int64_t ncon,
                       int64_t batch, int device, const cnl::Tuning& o) {
  cnl_plan* plan = nullptr;
  cnl::Tuning g;
  if (int rc = f32_general_plan(&plan, N, nnz, rows1, cols1, nvar, nequ, ncon, o, &g, batch)) return rc;
  if (plan->D.active) return create_f32_dense_from_plan(hout, plan, rows1, cols1, batch, device);
  const bool direct_plan = plan->P.rec_direct, staged_plan = g.float32_staged && plan->latency;
  if (int rc = create_f32_general_from_plan(hout, plan, rows1, cols1, batch, device)) return rc;
  if (staged_plan && !(*hout)->staged) {
    // tuning float32_staged, and setup_v2 declined the latency plan (its LDS block, its 32-bit offsets): on the single stream the
    // latency order is only a worse order, so the handle is the one without the key, from its own throughput analysis
    cnl_destroy(*hout);
    *hout = nullptr;
    return create_f32_general(hout, N, nnz, rows1, cols1, nvar, nequ, ncon, batch, device, f32_unstaged_options(o));
  }
  if (direct_plan && (*hout)->route != cnl::Route::Direct) {
    // setup_v2 declined the direct records (their LDS block is the larger one): the handle is the one without the key
    cnl_destroy(*hout);
    *hout = nullptr;
    g.direct_records = 0;
    if (int rc = plan_create_impl(&plan, N, nnz, rows1, cols1, nvar, nequ, ncon, 0, 0, 0, g)) return rc;
    return create_f32_general_from_plan(hout, plan, rows1, cols1, batch, device);
  }
  return CNL_OK;
}

// Tuning float32_refine (handle.h: cnl_handle::inner): the inner Float32 general handle from the caller's own options with band_kernel
// forced to 0, and around it a Float64 handle on the same plan that owns the Float64 row lists, the rows of the full matrix and the
// float arrays the refined calls convert into.
int create_refined(cnl_handle** hout, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar, int64_t nequ, int64_t ncon,
                   int64_t batch, int device, const cnl::Tuning& o) {
  if (int rc = check_batch(batch)) return rc;
  if (int rc = check_f32_options(o, "cnl_create_ex")) return rc;
  if (int rc = check_no_general_blocked(o, "cnl_create_ex (the inner Float32 handle of tuning float32_refine)")) return rc;
  if (int rc = check_device(device)) return rc;
  cnl::Tuning oi = o;
  oi.band_kernel = 0; oi.float32_refine = 0;
  cnl_handle* inner = nullptr;
  if (int rc = create_f32_general(&inner, N, nnz, rows1, cols1, nvar, nequ, ncon, batch, device, oi)) return rc;
  cnl_handle* h = nullptr;
  inner->plan->refs.fetch_add(1);
  if (int rc = new_handle(&h, inner->plan, batch, device, false, false)) { cnl_destroy(inner); return rc; }
  h->inner = inner;
  h->refine_k = o.float32_refine;
  auto bail = [&](int code) { cnl_destroy(h); return code; };
  int rc;
  const size_t B = (size_t)batch;
  if ((rc = dalloc(h, &h->r_vals, B * (size_t)nnz))) return bail(rc);
  if ((rc = dalloc(h, &h->r_rhs, B * (size_t)N))) return bail(rc);
  if ((rc = dalloc(h, &h->r_e, B * (size_t)N))) return bail(rc);
  if ((rc = dalloc(h, &h->r_rho, B))) return bail(rc);
  if ((rc = dalloc(h, &h->r_rho_old, B))) return bail(rc);
  if ((rc = dalloc(h, &h->r_success, B))) return bail(rc);
  if ((rc = dalloc(h, &h->r_norms, B * (size_t)h->refine_k))) return bail(rc);
  {
    const std::vector<double> none(B * (size_t)h->refine_k, -1.0);   // (no problem holds a factor yet)
    if (hipMemcpy(h->r_norms, none.data(), none.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return bail(fail(CNL_ERR_HIP, "hipMemcpy failed"));
  }
  if ((rc = finish_handle(h, rows1, cols1))) return bail(rc);   // (the route it sets is never read: run() dispatches on h->inner first)
  if ((rc = ensure_kkt_rows(h))) return bail(rc);
  *hout = h;
  return CNL_OK;
}

}  // namespace

// the rows of the full KKT matrix on the device, on first use (as cgls_ws): pattern-sized, shared by all problems of the handle
int ensure_kkt_rows(cnl_handle* h) {
  if (h->dkkt.ptr) return CNL_OK;
  const cnl::KktRows& R = kkt_rows(h->plan);
  cnl::DevKktRows D{};
  int rc;
  HIPCHK(hipSetDevice(h->device));
  if ((rc = upload(h, R.slot, &D.slot))) return rc;
  if ((rc = upload(h, R.col, &D.col))) return rc;
  D.N = (int32_t)h->plan->N; D.nnz = h->plan->nnz;
  // the instance (tuning refine_rows: 1 lane, 2 wavefront; 0: by the mean row length, refine.h)
  const int force = h->plan->opt.refine_rows;
  D.wave_rows = force ? force == 2 : (int64_t)R.slot.size() >= (int64_t)cnl::KKT_WAVE_ROW_THRESHOLD * h->plan->N;
  // small batches: several workgroups per problem, each a chunk of whole rows — at least a row per thread (lane rows) or four rows
  // per wavefront (wavefront rows)
  const int64_t min_rows = D.wave_rows ? 16 : 256, max_chunks = (h->plan->N + min_rows - 1) / min_rows;
  D.nchunk = (int32_t)std::max<int64_t>(1, std::min<int64_t>(max_chunks, (cnl::KKT_TARGET_WORKGROUPS + h->full_batch - 1) / h->full_batch));
  D.rows_per_chunk = (int32_t)((h->plan->N + D.nchunk - 1) / D.nchunk);
  D.nchunk = (int32_t)((h->plan->N + D.rows_per_chunk - 1) / D.rows_per_chunk);   // (no empty chunk)
  if (D.nchunk > 1 && (rc = dalloc(h, &D.partial, (size_t)h->full_batch * (size_t)D.nchunk))) return rc;
  if ((rc = upload(h, R.ptr, &D.ptr))) return rc;   // (last: the lists exist)
  h->dkkt = D;
  return CNL_OK;
}

cnl::SubtreeStageShape subtree_stage_shape(const cnl_handle* h, int s, int64_t batch) {
  const int64_t tasks = h->gstage_ptr[s + 1] - h->gstage_ptr[s];
  const bool wide = h->sub_wide > 0 && h->gstage_fmax[s] >= h->sub_wide && tasks * batch <= 2 * (int64_t)h->sub_cus;
  return {wide ? 1024 : h->cfg.tpp, h->gstage_lpan[s] ? h->gstage_lpan[s] : (int32_t)(16 * h->esz())};
}

extern "C" {

int cnl_create(cnl_handle** hout, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar,
               int64_t nequ, int64_t ncon, int64_t batch, int device) {
  return cnl_create_ex(hout, N, nnz, rows1, cols1, nvar, nequ, ncon, batch, device, nullptr);
}

int cnl_create_ex(cnl_handle** hout, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar,
                  int64_t nequ, int64_t ncon, int64_t batch, int device, const cnl_options* opt) {
  if (!hout) return fail(CNL_ERR_ARG, "null handle pointer");
  *hout = nullptr;
  cnl::Tuning o;
  const int rc0 = resolve_options(opt, o);
  if (rc0) return rc0;
  if (o.float32_refine) return create_refined(hout, N, nnz, rows1, cols1, nvar, nequ, ncon, batch, device, o);
  if (int rc = check_subtree_ladder(o, false, "cnl_create_ex")) return rc;
  if (o.float32_staged || o.float32_latency)   // (the key's own rules, as every creator answers them; a Float64 handle reads nothing else of it)
    if (int rc = check_f32_options(o, "cnl_create_ex")) return rc;
  return create_tuned(hout, N, nnz, rows1, cols1, nvar, nequ, ncon, batch, device, o);
}

int cnl_create_f32(cnl_handle** hout, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar, int64_t nequ,
                   int64_t ncon, int64_t batch, int device) {
  return cnl_create_f32_ex(hout, N, nnz, rows1, cols1, nvar, nequ, ncon, batch, device, nullptr);
}

int cnl_create_f32_ex(cnl_handle** hout, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar, int64_t nequ,
                      int64_t ncon, int64_t batch, int device, const cnl_options* opt) {
  if (!hout) return fail(CNL_ERR_ARG, "null handle pointer");
  *hout = nullptr;
  cnl::Tuning o;
  if (int rc = resolve_options(opt, o)) return rc;
  if (int rc = check_batch(batch)) return rc;
  if (o.float32_refine)
    return fail(CNL_ERR_ARG, "cnl_create_f32: tuning float32_refine makes a Float64 handle on a Float32 factor: it is read by cnl_create_ex, not here");
  if (int rc = check_f32_options(o, "cnl_create_f32")) return rc;
  if (int rc = check_no_general_blocked(o, "cnl_create_f32")) return rc;
  if (int rc = check_subtree_ladder(o, true, "cnl_create_f32")) return rc;
  if (!o.band_kernel && !o.float32_general)
    return fail(CNL_ERR_ARG, "cnl_create_f32: cnl_options.band_kernel = 0, and Float32 handles run on the band kernels only (tuning float32_general = 1: "
                             "the general multifrontal kernel)");
  // The band kernels first (band_kernel != 0).  The throughput analysis whatever the batch: there is nothing but the band program to
  // run.  The analysis is host work, so a pattern the band kernels refuse is refused with that reason whether or not a device is there.
  cnl_plan* plan = nullptr;
  if (o.band_kernel) {
    if (int rc = plan_create_impl(&plan, N, nnz, rows1, cols1, nvar, nequ, ncon, 0, 0, 0, o)) return rc;
    if (!band_program(plan, true).ok) {   // (the analysis builds it next to the Float64 program; not for a pattern the Float64 handles serve otherwise)
      build_band_programs(plan, rows1, cols1, (int)sizeof(float));
      band_summaries(plan);
    }
    if (!band_program(plan, true).ok) {
      const std::string why = plan->band_prog[1][1].B.why.empty() ? plan->band_prog[1][0].B.why : plan->band_prog[1][1].B.why;
      cnl_plan_destroy(plan);
      plan = nullptr;
      if (!o.float32_general)
        return fail(CNL_ERR_ARG, "cnl_create_f32: the pattern is not served by the band kernels (build_band_plan: " + why +
                                     "); Float32 stays on the CPU backend for it (or tuning float32_general = 1: the general multifrontal kernel)");
    }
  }
  if (int rc = check_device(device)) { cnl_plan_destroy(plan); return rc; }
  if (plan) {
    if (int rc = create_f32_from_plan(hout, plan, rows1, cols1, batch, device)) return rc;
    if (*hout) return CNL_OK;   // (else: the program does not fit the band kernels, and float32_general is set)
  }
  // tuning float32_general: the general multifrontal kernel in float, on the plan f32_general_plan makes of the options (capi_plan.cpp)
  return create_f32_general(hout, N, nnz, rows1, cols1, nvar, nequ, ncon, batch, device, o);
}

int cnl_destroy(cnl_handle* h) {
  if (!h) return CNL_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : h->dev_allocs) (void)hipFree(p);
  if (h->pin) (void)hipHostFree(h->pin);
  cnl::dense_destroy(h->dense);
  cnl::dense_destroy(h->gdense);
  if (h->tail) { cnl_destroy(h->tail); h->tail = nullptr; (void)hipSetDevice(h->device); }
  if (h->inner) { cnl_destroy(h->inner); h->inner = nullptr; (void)hipSetDevice(h->device); }
  if (h->aux_stream) { (void)hipStreamSynchronize(h->aux_stream); (void)hipStreamDestroy(h->aux_stream); }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  for (hipEvent_t e : h->pipe_ev) (void)hipEventDestroy(e);
  for (hipStream_t st : h->pipe_stream) if (st) (void)hipStreamDestroy(st);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  cnl_plan_destroy(h->plan);
  delete h;
  return CNL_OK;
}

const cnl_plan* cnl_get_plan(const cnl_handle* h) { return h ? h->plan : nullptr; }

int cnl_dataflow_timeouts(cnl_handle* h, int64_t* count) {
  if (!h || !count) return fail(CNL_ERR_ARG, "null argument");
  *count = 0;
  if (h->d_status) {
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    int v = 0;
    HIPCHK(hipMemcpy(&v, h->d_status, sizeof(int), hipMemcpyDeviceToHost));
    *count = v;
  }
  if (h->tail) {
    int64_t tc = 0;
    const int rc = cnl_dataflow_timeouts(h->tail, &tc);
    if (rc) return rc;
    *count += tc;
  }
  return CNL_OK;
}

int cnl_get_refine_norms(cnl_handle* h, double* norms, int64_t* steps) {
  if (!h || !norms || !steps) return fail(CNL_ERR_ARG, "null argument");
  if (!h->inner) return fail(CNL_ERR_STATE, "cnl_get_refine_norms: the handle was created without tuning float32_refine");
  if (!h->r_norms_valid) return fail(CNL_ERR_STATE, "cnl_get_refine_norms before a cnl_newton_system or cnl_solve call of the handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(norms, h->r_norms, (size_t)h->full_batch * (size_t)h->refine_k * sizeof(double), hipMemcpyDeviceToHost));
  *steps = h->refine_k;
  return CNL_OK;
}

int cnl_layout_len(const cnl_handle* h, int which, int64_t* doubles) {
  if (!h || !doubles) return fail(CNL_ERR_ARG, "null argument");
  int64_t len = 0;
  if (int rc = layout_rowlen(h, which, &len)) return rc;
  *doubles = cnl::band_il_len(h->full_batch, len);   // (of the created batch, whatever cnl_set_active_batch says)
  return CNL_OK;
}
int cnl_interleave_dev(cnl_handle* h, int which, const double* d_src, double* d_dst, void* stream) {
  CNL_NEED_F64(h);
  return convert_layout(h, which, d_src, d_dst, 1, stream);
}
int cnl_deinterleave_dev(cnl_handle* h, int which, const double* d_src, double* d_dst, void* stream) {
  CNL_NEED_F64(h);
  return convert_layout(h, which, d_src, d_dst, 0, stream);
}
int cnl_interleave_f32_dev(cnl_handle* h, int which, const float* d_src, float* d_dst, void* stream) {
  CNL_NEED_F32(h);
  return convert_layout(h, which, d_src, d_dst, 1, stream);
}
int cnl_deinterleave_f32_dev(cnl_handle* h, int which, const float* d_src, float* d_dst, void* stream) {
  CNL_NEED_F32(h);
  return convert_layout(h, which, d_src, d_dst, 0, stream);
}

// The handle works on its first nb problems from here on: every device-pointer entry point launches over nb problems instead of the
// created batch, on the same arrays (every kernel of the path is per problem and guards its problem index against the batch it is
// given, and every per-problem array of the handle is addressed from problem 0: a prefix needs no other address).  Served where a
// call is one classic launch — the band kernels, the register-front or the general kernel with their condensation passes; executions
// that cut the batch themselves (staged / dataflow counters sized by the batch, split batches, the dense backend's tiles) refuse.
int cnl_set_active_batch(cnl_handle* h, int64_t nb) {
  if (!h) return fail(CNL_ERR_ARG, "null handle");
  if (nb < 1 || nb > h->full_batch)
    return fail(CNL_ERR_ARG, "cnl_set_active_batch: nb = " + std::to_string(nb) + " is outside [1, " + std::to_string(h->full_batch) + "] (the created batch)");
  if (h->inner) {   // a refined handle: its inner handle decides (the dense routes refuse), and both work on the same problems
    if (int rc = cnl_set_active_batch(h->inner, nb)) return rc;
    h->batch = nb;
    return CNL_OK;
  }
  if (nb == h->batch) return CNL_OK;
  const bool dense_route = h->route == cnl::Route::Dense || h->route == cnl::Route::GeneralDense;
  if (dense_route) return fail(CNL_ERR_STATE, "cnl_set_active_batch: this handle runs on the dense backend, which is sized by the created batch");
  if (h->route != cnl::Route::Band) {
    if (h->tail || h->split_halves || h->split_staged > 0)
      return fail(CNL_ERR_STATE, "cnl_set_active_batch: this handle runs its batch split (tail handle, halves or concurrent parts)");
    if (h->staged || h->d_dep)
      return fail(CNL_ERR_STATE, "cnl_set_active_batch: this handle runs staged / dataflow (task counters sized by the created batch)");
  }
  h->batch = nb;
  return CNL_OK;
}

int cnl_get_active_batch(const cnl_handle* h, int64_t* nb) {
  if (!h || !nb) return fail(CNL_ERR_ARG, "null argument");
  *nb = h->batch;
  return CNL_OK;
}

int cnl_set_timing(cnl_handle* h, int enable) {
  if (!h) return fail(CNL_ERR_ARG, "null handle");
  h->timing = enable != 0;
  return CNL_OK;
}

int cnl_last_kernel_ms(cnl_handle* h, float* ms) {
  if (!h || !ms) return fail(CNL_ERR_ARG, "null argument");
  *ms = h->last_ms;
  return CNL_OK;
}

int cnl_get_config(const cnl_handle* h, int64_t cfg[8]) {
  if (!h || !cfg) return fail(CNL_ERR_ARG, "null argument");
  if (h->inner) {
    // a refined handle (tuning float32_refine): the words of its inner handle, as a Float64 handle (bit 27 clear) with bit 38 set and
    // the refinement steps in bits 39 .. 41; row f1 (bit 7) is the outer handle's own
    if (int rc = cnl_get_config(h->inner, cfg)) return rc;
    cfg[5] &= ~(((int64_t)1 << 27) | (int64_t)128);
    cfg[5] |= ((int64_t)1 << 38) | ((int64_t)h->refine_k << 39);
    if (h->djt.rv_ntiles > 0) cfg[5] |= 128;
    return CNL_OK;
  }
  std::memset(cfg, 0, 8 * sizeof(int64_t));
  const bool on_band = h->route == cnl::Route::Band, dense_route = h->route == cnl::Route::Dense || h->route == cnl::Route::GeneralDense;
  if (h->f32 && on_band) {   // Float32 handle on the band kernels
    cfg[5] = 64 | ((int64_t)h->band_nl << 8) | ((int64_t)h->bd.nparts << 16) | ((int64_t)h->layout << 25) | ((int64_t)1 << 27) | ((int64_t)h->band_npiece << 28);
    if (h->djt.rv_ntiles > 0) cfg[5] |= 128;
    cfg[5] |= (int64_t)(h->plan->opt.cgls_wide & 3) << 45;
    return CNL_OK;
  }
  cfg[0] = h->cfg.tpp; cfg[1] = h->cfg.ppb; cfg[2] = (int64_t)h->cfg.lds_bytes; cfg[3] = h->cfg.lds_work;
  cfg[4] = (h->full_batch + h->cfg.ppb - 1) / h->cfg.ppb;
  cfg[5] = dense_route ? 3 : (h->use_v2 ? (h->staged ? 4 : 2) : 1);
  if (h->f32) cfg[5] |= (int64_t)1 << 27;                // a Float32 handle on the general kernel (tuning float32_general): bit 6 clear
  if (h->cond_resident) cfg[5] |= (int64_t)1 << 35;      // ... whose condensation runs the resident condense kernel (tuning float32_condense = 1)
  if (h->route == cnl::Route::Direct) cfg[5] |= (int64_t)1 << 36;                 // the Direct route (call_shape.h), either element type
  if (h->route == cnl::Route::Direct && h->v2_solve) cfg[5] |= (int64_t)1 << 37;  // ... on which solve_ldl! runs on the register-front kernel too
  if (h->cfg.blocked && !h->use_v2 && !dense_route && !on_band) cfg[5] |= (int64_t)1 << (h->f32 ? 48 : 47);   // newton_system / factorize run a blocked instance of the general kernel (bit 47: Float64, tuning general_blocked; bit 48: Float32, tuning float32_blocked)
  if (h->subtrees) cfg[5] |= (int64_t)1 << (h->f32 ? 50 : 49);   // the three calls run the general kernel's subtree instances stage by stage (bit 49: Float64, tuning general_subtrees; bit 50: Float32, tuning float32_subtrees; where the key acts)
  if (h->subtrees) cfg[5] |= (int64_t)(h->ladder_rungs & 127) << 51;   // ... with this many rungs of the rho ladder enqueued behind the first attempt of newton_system (bits 51 .. 57: tuning subtree_ladder, 0 .. 64, where the subtree key acts)
  if (h->subtrees) {   // tuning subtree_wide / subtree_lds_panels: bit 58 — at least one stage factorises with 1024 threads at the created batch; bit 59 — at least one stage runs the LPAN instance
    for (int st = 0; st + 1 < (int)h->gstage_ptr.size(); st++) {
      const cnl::SubtreeStageShape sh = subtree_stage_shape(h, st, h->full_batch);
      if (sh.tpp != h->cfg.tpp) cfg[5] |= (int64_t)1 << 58;
      if (h->gstage_lpan[st]) cfg[5] |= (int64_t)1 << 59;
    }
    cfg[5] |= (int64_t)(h->solve_panels & 3) << 60;   // tuning subtree_solve_panels: the mask of the solve sweeps that run in panels of 16 pivots (bit 60: backward stages, bit 61: forward stages of solve_ldl!)
  }
  if (h->lean && !dense_route) cfg[5] |= 16;  // newton_system / factorize run the kernels' LEAN instantiation
  if (h->staged && h->use_v2 && !dense_route) {          // staged handles: how the stages run
    if (h->d_dep) cfg[5] |= (int64_t)1 << 42;            // dataflow counters present (one launch per phase where the rule allows)
    cfg[5] |= (int64_t)(h->lad_mode & 3) << 43;          // the in-kernel ladder: 0 none (sequential launch behind the attempt), 1, 2 fused
  }
  if (h->tail) cfg[5] |= 32;                          // the remainder of the batch runs on a handle of its own (split_tail)
  if (on_band) cfg[5] |= 64 | ((int64_t)h->band_nl << 8) | ((int64_t)h->bd.nparts << 16) | ((int64_t)h->band_resident << 24) | ((int64_t)h->layout << 25) | ((int64_t)h->band_npiece << 28) | ((int64_t)h->band_mover << 34) | ((int64_t)(h->band_policy & 31) << 18);   // newton_system runs on the band kernels (csrc/band.h): problems per workgroup, parts (bits 16 / 17: one or two), layout, operand pieces per epoch, mover table (bit 34: bit 27 marks a Float32 handle), cache policy of the mover-table instance (bits 18 .. 22: tuning band_cache_policy, 0 on every other instance)
  if (h->djt.rv_ntiles > 0) cfg[5] |= 128;               // row f1 runs on column tiles (kernels.h: DevJt::rv_*)
  cfg[5] |= (int64_t)(h->plan->opt.cgls_wide & 3) << 45;    // row f4: tuning cgls_wide (1: the wide instance above 1024 constraints, 2: always)
  cfg[6] = h->wpb2;
  cfg[7] = (int64_t)h->lds2;
  return CNL_OK;
}

int cnl_subtree_stage_shape(const cnl_handle* h, int32_t* tpp, int32_t* lds_bytes, int64_t* nstages) {
  if (!h || !nstages) return fail(CNL_ERR_ARG, "null argument");
  if (!h->subtrees) return fail(CNL_ERR_ARG, "cnl_subtree_stage_shape: not a subtree handle (cnl_get_config bits 49 / 50)");
  const int nst = (int)h->gstage_ptr.size() - 1;
  *nstages = nst;
  for (int s = 0; s < nst; s++) {
    const cnl::SubtreeStageShape sh = subtree_stage_shape(h, s, h->batch);
    if (tpp) tpp[s] = sh.tpp;
    if (lds_bytes) lds_bytes[s] = sh.lds_bytes;
  }
  return CNL_OK;
}

}  // extern "C"
