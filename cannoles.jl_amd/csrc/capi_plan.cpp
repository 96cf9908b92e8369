// capi_plan.cpp — options, default parameters and the symbolic plan of the C ABI (include/cannoles_hip.h): cnl_options -> the internal
// switch set, plan creation (analysis, direct records, band programs and their summaries), cnl_plan_info / _get / _destroy, and the
// library's error text.  Nothing here touches the device.
#include "handle.h"

thread_local std::string g_err;

// the names cnl_plan_get answers for band_prog[f32][wide]: "band_*" / "band4_*" keep describing the 15-piece program
static const char* const kBandPrefix[2][2] = {{"band_", "bandw_"}, {"band4_", "bandw4_"}};
static const char* const kBandResPrefix = "bandr_";   // ... and for band_res, a prefix of its own
static const char* const kBandMovPrefix = "bandm_";   // the mover table of band_res: "bandm_info" = {has one, words per epoch, typed sets}, "bandm_table<q>"

// band programs -> the summaries cnl_plan_get returns as "<prefix>info" / "<prefix>part<q>"
void band_summaries(cnl_plan* p) {
  cnl_plan::BandSlot* const all[5] = {&p->band_prog[0][0], &p->band_prog[0][1], &p->band_prog[1][0], &p->band_prog[1][1], &p->band_res};
  for (cnl_plan::BandSlot* sp : all) {
    cnl_plan::BandSlot& s = *sp;
    const cnl::BandPlan& Bp = s.B;
    // (the last word: the piece count of a wide program; 0 = the fifteen of "band_*" / "band4_*", as it always was)
    s.info = {Bp.ok ? 1 : 0, Bp.nparts, Bp.m0, Bp.n, Bp.N, Bp.nnz, (int32_t)Bp.lsize, Bp.ok && Bp.npiece != cnl::BAND_NPIECE ? Bp.npiece : 0};
    for (int q = 0; q < 2; q++) s.pinfo[q] = {Bp.part[q].nsteps, Bp.part[q].nepochs, Bp.part[q].npiv, Bp.part[q].nevents, (int32_t)Bp.part[q].loff};
  }
  p->band_mov_info = {p->band_res.B.mover_ok ? 1 : 0, cnl::BAND_MOV_EW, cnl::BAND_MOV_FVALS, cnl::BAND_MOV_BVALS, cnl::BAND_MOV_BFACTOR};
}

// The band programs of a pattern for one element size: the 15-piece program whenever the pattern fits it, word for word what it always
// was; the wide one only where it does not fit (tuning band_pieces = 0), never (15), or also where 15 fit (20: the wide kernel
// instances then run the handle — same steps, same arithmetic, bit-equal outputs).
void build_band_programs(cnl_plan* p, const int64_t* rows1, const int64_t* cols1, int esz) {
  const cnl::Tuning& o = p->opt;
  const int64_t N = p->N, nnz = p->nnz, nvar = p->nvar, nequ = p->nequ, ncon = p->ncon;
  cnl::BandPlan &B15 = p->band_prog[esz == 4][0].B, &Bw = p->band_prog[esz == 4][1].B;
  const int nparts = o.band_kernel == 2 ? 1 : 2;
  cnl::build_band_plan(B15, N, nnz, rows1, cols1, nvar, nequ, ncon, nparts, esz, cnl::BAND_NPIECE);
  Bw = cnl::BandPlan();
  Bw.why = B15.ok ? "fifteen operand pieces per epoch suffice" : B15.why;
  if (o.band_pieces != 15 && (B15.ok ? o.band_pieces == 20 : B15.pieces_short))
    cnl::build_band_plan(Bw, N, nnz, rows1, cols1, nvar, nequ, ncon, nparts, esz, cnl::BAND_NPIECE_WIDE);
  if (esz == 8) {
    cnl::BandPlan& Br = p->band_res.B;
    Br = cnl::BandPlan();
    Br.why = !o.band_resident ? "tuning band_resident = 0" : B15.why;
    if (B15.ok && o.band_resident) cnl::build_band_plan(Br, N, nnz, rows1, cols1, nvar, nequ, ncon, nparts, esz, cnl::BAND_NPIECE, true);
    // its mover table (band.h, BAND_MK_*): Br itself stays word for word what it was
    if (Br.ok && o.band_mover_table) cnl::build_band_mover(Br);
    else Br.mover_why = Br.ok ? "tuning band_mover_table = 0" : Br.why;
  }
}
// the program a handle runs: the wide one where the plan has it (the pattern needs it, or tuning band_pieces = 20)
const cnl::BandPlan& band_program(const cnl_plan* plan, bool f32) {
  return plan->band_prog[f32][plan->band_prog[f32][1].B.ok].B;
}

// public options -> the internal switch set: the defaults, the public fields, then the `tuning` pairs (which may name any switch of
// options.h, public ones included); rejects a struct of another ABI revision and unknown keys
int resolve_options(const cnl_options* in, cnl::Tuning& out) {
  out = cnl::Tuning();
  if (!in) return CNL_OK;
  if (in->struct_size != (int32_t)sizeof(cnl_options)) return fail(CNL_ERR_ARG, "cnl_options.struct_size does not match this library (use cnl_options_init)");
  out.plan_kind = in->plan_kind; out.staged_max_batch = in->staged_max_batch; out.verbose = in->verbose; out.band_kernel = in->band_kernel;
  out.dense_backend = in->dense_backend; out.staged = in->staged; out.dataflow = in->dataflow; out.device_ladder = in->device_ladder;
  out.host_ladder = in->host_ladder; out.split_tail = in->split_tail; out.multi_share_plan = in->multi_share_plan; out.batch_layout = in->batch_layout;
  std::memcpy(out.force_order, in->force_order, sizeof(out.force_order));
  out.force_order[sizeof(out.force_order) - 1] = 0;
  char tun[sizeof(in->tuning) + 1];
  std::memcpy(tun, in->tuning, sizeof(in->tuning));
  tun[sizeof(in->tuning)] = 0;
  const std::string err = cnl::tuning_parse(out, tun);
  if (!err.empty()) return fail(CNL_ERR_ARG, err);
  if (out.band_pieces != 0 && out.band_pieces != cnl::BAND_NPIECE && out.band_pieces != cnl::BAND_NPIECE_WIDE)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: band_pieces must be 0 (automatic), 15 or 20");
  if (out.band_cache_policy < 0 || out.band_cache_policy > 31 || ((out.band_cache_policy & 4) && (out.band_cache_policy & 8)))
    return fail(CNL_ERR_ARG, "cnl_options.tuning: band_cache_policy is a bit mask, 0 .. 31 (1 vals loads, 2 factor loads, 4 record stores non-temporal, 8 record stores written through, "
                             "16 d stores non-temporal); bits 4 and 8 exclude each other");
  if (!cnl::band_policy_built(out.band_cache_policy))
    return fail(CNL_ERR_ARG, "cnl_options.tuning: band_cache_policy = " + std::to_string(out.band_cache_policy) + ": the band kernel has no instance under this mask");
  if (out.float32_refine < 0 || out.float32_refine > 4)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: float32_refine is the number of refinement steps, 0 (none) .. 4");
  if (out.float32_refine && !out.float32_general)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: float32_refine needs float32_general = 1 (the refined handle owns a Float32 general handle, which keeps a factor; "
                             "the band kernels keep none)");
  if (out.float32_refine && out.batch_layout == CNL_LAYOUT_INTERLEAVED)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: float32_refine takes problem-major arrays: batch_layout = CNL_LAYOUT_INTERLEAVED is the band kernels' layout");
  if (out.refine_rows < 0 || out.refine_rows > 2)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: refine_rows is 0 (by the pattern), 1 (a row per lane) or 2 (a row per wavefront)");
  if (out.general_blocked < 0 || out.general_blocked > 1)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: general_blocked is 0 or 1 (the general kernel eliminates large fronts in panels of 16 pivots)");
  if (out.general_subtrees < 0 || out.general_subtrees > 1)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: general_subtrees is 0 or 1 (the general kernel runs the subtrees of the elimination tree on workgroups of their own, stage by stage)");
  if (out.subtree_ladder < 0 || out.subtree_ladder > 64)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: subtree_ladder is the number of rungs of the rho ladder a subtree handle enqueues behind the first attempt, 0 (none) .. 64");
  if (out.subtree_ladder && !out.general_subtrees && !out.float32_subtrees)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: subtree_ladder needs general_subtrees = 1 (Float64 handles) or float32_subtrees = 1 (Float32 general handles): the rungs run on the subtree instances of the general kernel");
  if (out.subtree_ladder && out.float32_refine)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: subtree_ladder does not go with float32_refine (no refined handle over a subtree factor)");
  if (out.subtree_wide < 0 || out.subtree_wide > 4096)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: subtree_wide is the task fmax from which a stage of a subtree handle factorises with 1024 threads per workgroup, 1 .. 4096, or 0 (off)");
  if (out.subtree_lds_panels != 0 && (out.subtree_lds_panels < 16 || out.subtree_lds_panels > 4096))
    return fail(CNL_ERR_ARG, "cnl_options.tuning: subtree_lds_panels is the task fmax up to which a stage of a blocked subtree handle eliminates its dependent pivot panels in LDS, 16 .. 4096, or 0 (off)");
  if ((out.subtree_wide || out.subtree_lds_panels) && !out.general_subtrees && !out.float32_subtrees)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: subtree_wide and subtree_lds_panels need general_subtrees = 1 (Float64 handles) or float32_subtrees = 1 (Float32 general handles): they shape the stage launches of the subtree instances");
  if ((out.subtree_wide || out.subtree_lds_panels) && out.float32_refine)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: subtree_wide and subtree_lds_panels do not go with float32_refine (no refined handle over a subtree factor)");
  if (out.subtree_lds_panels && !out.general_blocked && !out.float32_blocked)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: subtree_lds_panels needs general_blocked = 1 (Float64 handles) or float32_blocked = 1 (Float32 general handles): the pivot panels are those of the blocked instances");
  if (out.subtree_solve_panels < 0 || out.subtree_solve_panels > 3)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: subtree_solve_panels is a bit mask, 0 .. 3: bit 0 the backward stage launches of a subtree handle in panels of 16 pivots, bit 1 the forward stage launches of solve_ldl!");
  if (out.subtree_solve_panels && !out.general_subtrees && !out.float32_subtrees)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: subtree_solve_panels needs general_subtrees = 1 (Float64 handles) or float32_subtrees = 1 (Float32 general handles): it shapes the solve sweeps of the subtree instances");
  if (out.subtree_solve_panels && out.float32_refine)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: subtree_solve_panels does not go with float32_refine (no refined handle over a subtree factor)");
  if (out.cgls_wide < 0 || out.cgls_wide > 2)
    return fail(CNL_ERR_ARG, "cnl_options.tuning: cgls_wide is 0 (the LDS instance, ncon <= 1024), 1 (the wide instance where ncon > 1024) or 2 (the wide instance always)");
  return CNL_OK;
}

// latency != 0: plan for a small batch — order chosen by the critical path, tree cut into tasks (par = wavefront slots per
// group of four problems)
int plan_create_impl(cnl_plan** plan, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar,
                     int64_t nequ, int64_t ncon, int latency, int par, double slots, const cnl::Tuning& o) {
  if (!plan || !rows1 || !cols1) return fail(CNL_ERR_ARG, "null argument");
  cnl_plan* p = new cnl_plan();
  p->N = N; p->nnz = nnz; p->nvar = nvar; p->nequ = nequ; p->ncon = ncon;
  p->latency = latency != 0;
  p->opt = o;
  const bool verbose = o.verbose != 0 || getenv("CNL_VERBOSE") != nullptr;  // logging only
  std::string msg;
  cnl::Options opt;
  opt.latency = latency; opt.par = std::max(1, par); opt.slots = slots;
  opt.order_mode = o.order_mode; opt.nd_leaf = o.nd_leaf; opt.relax = o.relax; opt.task_cap = o.task_cap;
  opt.early = o.multipliers_early; opt.register_front = o.register_front; opt.ubig = o.ubig; opt.wait_thr = o.wait_thr;
  opt.verbose = verbose ? 1 : 0; opt.force_order = o.force_order; opt.threads = o.analysis_threads;
  opt.general_subtrees = o.general_subtrees; opt.gsub_rows = o.general_blocked ? 16 : 2;   // (the staging rows choose_config sizes)
  const auto t_start = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {   // (verbose log: seconds since the analysis started)
    if (verbose) fprintf(stderr, "[cnl] analysis %-28s %.3f s\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count());
  };
  int rc = cnl::build_condensation(p->C, N, nnz, rows1, cols1, nvar, nequ, ncon, msg, o.condense != 0);
  lap("condensation");
  if (!rc) {
    if (p->C.active)
      rc = cnl::build_plan(p->P, p->C.N2, p->C.ncs + nvar, p->C.rows2.data(), p->C.cols2.data(), nvar, p->C.nequ2, ncon, opt, msg);
    else
      rc = cnl::build_plan(p->P, N, nnz, rows1, cols1, nvar, nequ, ncon, opt, msg);
  }
  lap("ordering + plan");
  if (rc) {
    delete p;
    *plan = nullptr;
    return fail(rc, msg);
  }
  // register-front kernel on a condensed system: rewrite the assembly lists against the ORIGINAL arrays, so
  // that the kernel condenses on the fly and the separate condense pass disappears (CNL_NO_DIRECT=1 keeps it)
  if (p->C.active && p->P.v2_ok && o.direct_records) {
    cnl::DirectLists D{p->C.c_ptr.data(), p->C.c_a.data(), p->C.c_b.data(), p->C.c_d.data(), (int32_t)nnz, (int32_t)N};
    const int32_t old_len = p->P.rec_maxlen;
    const size_t old_words = p->P.rec.size();
    p->P.row_products = o.row_products != 0;
    p->P.band_form = o.band_form != 0;
    // A plan whose fronts are ALL fast-class row-form fronts runs the kernels' lean instantiation and recovers the residual
    // components in its backward sweep (no post-pass): worth more than the few rounds small fronts save with product lists, so
    // every front is given the row form when that makes the whole plan lean.  A front whose residual rows do not fit the row form's
    // sixteen lanes is cut in two (same order, one more front) and the records are written again.
    // (round 6: such plans are written with the row form at once — the records with the lists' threshold of 72 products were
    //  written first and thrown away, one of five passes over the records of a latency plan)
    const bool fast_only = p->P.ncls[1] == 0 && p->P.ncls[2] == 0;
    const bool want_lean = o.row_products && o.lean_kernel && fast_only;
    p->P.row_min_products = want_lean ? 1 : 72;
    int drc = cnl::write_forward_records(p->P, &D);
    if (!drc && want_lean && p->P.listprod_fronts > 0) {
      if (!drc && p->P.listprod_fronts > 0 && !p->P.rows_overflow.empty() && p->P.rows_overflow.size() <= 64) {
        cnl::Options opt2 = opt;
        opt2.split_positions = p->P.rows_overflow;
        opt2.force_order = p->P.order_name;   // the same order, one more front: only that candidate is built again
        cnl::Plan P2;
        std::string msg2;
        if (cnl::build_plan(P2, p->C.N2, p->C.ncs + nvar, p->C.rows2.data(), p->C.cols2.data(), nvar, p->C.nequ2, ncon, opt2, msg2) == 0 &&
            P2.v2_ok && P2.ncls[1] == 0 && P2.ncls[2] == 0) {
          P2.row_products = true; P2.row_min_products = 1; P2.band_form = o.band_form != 0;
          if (cnl::write_forward_records(P2, &D) == 0 && P2.listprod_fronts == 0) {
            if (verbose) fprintf(stderr, "[cnl] %zu front(s) with more than 16 residual rows cut in two: %d -> %d fronts\n", p->P.rows_overflow.size(), p->P.nsuper, P2.nsuper);
            p->P = std::move(P2);
          }
        }
      }
      if (!drc && p->P.listprod_fronts > 0) {  // some front cannot take the row form: the lists' threshold again
        p->P.row_min_products = 72;
        drc = cnl::write_forward_records(p->P, &D);
      }
    }
    if (!drc) {
      // the backward records name the solution component of every pivot: switch them to the caller's numbering, so
      // that the kernel writes the kept components straight into `d` (no reduced solution vector, no copy pass)
      std::vector<int32_t>& br = p->P.brec;
      size_t r0 = 0;
      while (r0 + cnl::B_HDR <= br.size() && br[r0 + cnl::B_RECLEN] > 0) {
        const int32_t npiv = br[r0 + cnl::B_NPIV], nupd = br[r0 + cnl::B_NUPD];
        // a task root of a staged plan names the solution components of its update rows too
        const int32_t i0 = br[r0 + cnl::B_PXOFF] == cnl::B_PX_GLOBAL ? 1 : nupd + 1;
        for (int32_t i = i0; i < 1 + nupd + npiv; i++) br[r0 + cnl::B_HDR + i] = p->C.orig_of[br[r0 + cnl::B_HDR + i]];
        r0 += (size_t)br[r0 + cnl::B_RECLEN];
      }
      p->P.d_outer = true;
      cnl::finalize_tasks(p->P);  // the records moved
      // plans the lean kernel takes: the residual components of the rows a front owns are recovered in its backward step
      if (o.lean_kernel && o.rows_in_backward && p->P.ncls[1] == 0 && p->P.ncls[2] == 0 && p->P.listprod_fronts == 0) {
        const cnl::Cond& Cc = p->C;
        cnl::BackRowsIn in{Cc.r_orig.data(), Cc.r_dsrc.data(), Cc.r_ptr.data(), Cc.r_jsrc.data(), Cc.r_jx.data(), (int32_t)Cc.r_orig.size()};
        const int brc = cnl::write_backward_rows(p->P, in);
        if (verbose) fprintf(stderr, "[cnl] backward rows: %s\n", brc ? "not possible" : "ok");
      }
    } else {
      p->P.tasks.clear();  // staged execution needs the direct records
    }
    if (verbose)
      fprintf(stderr, "[cnl] direct records: %s, rec words %zu -> %zu, longest %d -> %d\n", drc ? "not possible" : "ok", old_words,
              p->P.rec.size(), old_len, p->P.rec_maxlen);
  }
  // A latency order that cannot run staged (setup_v2's conditions: tasks, direct records, solution components in the caller's
  // numbering, every condensed pivot counted by a front) would run on the single sequential stream, where it is only a worse
  // order — more total work, chosen for a critical path nothing exploits: take the throughput analysis instead.
  if (latency && p->opt.plan_kind != CNL_PLAN_LATENCY) {
    const bool stageable = o.staged && !p->P.tasks.empty() && p->P.v2_ok && p->P.rec_direct && p->P.d_outer &&
                           p->P.d_owned == (int64_t)p->C.r_dsrc.size();
    if (!stageable) {
      if (verbose) fprintf(stderr, "[cnl] latency plan cannot be staged: falling back to the throughput analysis\n");
      delete p;
      return plan_create_impl(plan, N, nnz, rows1, cols1, nvar, nequ, ncon, 0, 0, 0, o);
    }
  }
  if (o.dense_backend) cnl::detect_dense(p->D, N, nnz, rows1, cols1, nvar, nequ, ncon);
  lap("records");
  // (round 5) large batches of band-structured problems: the sliding-window elimination with one lane per (problem, part)
  if (!latency && o.band_kernel && p->C.active && !p->D.active) {
    build_band_programs(p, rows1, cols1, 8);
    const cnl::BandPlan &b15 = p->band_prog[0][0].B, &bw = p->band_prog[0][1].B;
    if (verbose) fprintf(stderr, "[cnl] band program: %s%s\n", b15.ok ? "ok" : "no: ", b15.ok ? "" : b15.why.c_str());
    if (verbose && b15.ok) fprintf(stderr, "[cnl] resident band program: %s%s\n", p->band_res.B.ok ? "ok" : "no: ", p->band_res.B.ok ? "" : p->band_res.B.why.c_str());
    if (verbose && !b15.ok && b15.pieces_short)
      fprintf(stderr, "[cnl] wide band program (%d pieces): %s%s\n", cnl::BAND_NPIECE_WIDE, bw.ok ? "ok" : "no: ", bw.ok ? "" : bw.why.c_str());
    // the programs for 4-byte elements (Float32 handles): the same blocks, every LDS offset scaled
    if (b15.ok || bw.ok) build_band_programs(p, rows1, cols1, 4);
  }
  band_summaries(p);
  // Irregular sparsity: when the fill makes fronts larger than the register-front kernel takes and the condensed system is of
  // moderate order, one dense LDL^T of the whole condensed matrix beats the general multifrontal kernel by far
  // (csrc/dense.h; chosen at handle creation for small batches; CNL_NO_GDENSE=1 disables)
  // (round 5) ... and so does a latency plan whose fronts reach the 64 class while the whole condensed system is of order <= 512: the
  // dense route costs 0.075 ms + 0.28 us per unit of order for one system (tools/time_dense_route.py), the staged walk over fronts of
  // that size 0.2 ms and more (n = 133, fronts up to 59: 0.215 against 0.106 ms).  The handle takes it for batches up to 16.
  p->prefer_dense = latency && p->P.v2_ok && p->P.ncls[2] > 0 && p->C.N2 <= 512;
  if (p->C.active && !p->D.active && (!p->P.v2_ok || p->prefer_dense || o.general_dense == 2) && p->C.N2 >= 96 && p->C.N2 <= 4096 && o.general_dense) {
    p->gpos.resize(p->C.ncs);
    for (int64_t s2 = 0; s2 < p->C.ncs; s2++) p->gpos[s2] = (int32_t)((p->C.rows2[s2] - 1) + p->C.N2 * (p->C.cols2[s2] - 1));
  }
  // elimination order in the reference's numbering: condensed residual nodes first
  if (p->C.active) {
    p->perm_outer.assign(p->C.r_orig.begin(), p->C.r_orig.end());
    for (int32_t e : p->P.perm) p->perm_outer.push_back(p->C.orig_of[e]);
    std::vector<int64_t>().swap(p->C.rows2);
    std::vector<int64_t>().swap(p->C.cols2);
  } else {
    p->perm_outer = p->P.perm;
  }
  lap("band program + done");
  p->pat_rows.resize((size_t)nnz); p->pat_cols.resize((size_t)nnz);   // (validated by the analysis: every index is inside [1, N])
  for (int64_t e = 0; e < nnz; e++) { p->pat_rows[e] = (int32_t)(rows1[e] - 1); p->pat_cols[e] = (int32_t)(cols1[e] - 1); }
  *plan = p;
  return CNL_OK;
}

const cnl::KktRows& kkt_rows(const cnl_plan* plan) {
  std::call_once(plan->kkt_once, [&] { cnl::build_kkt_rows(plan->kkt, plan->N, plan->nnz, plan->pat_rows.data(), plan->pat_cols.data()); });
  return plan->kkt;
}

int check_f32_options(const cnl::Tuning& o, const char* fn) {
  const std::string f(fn);
  if (o.float32_dense && !o.float32_general)
    return fail(CNL_ERR_ARG, f + ": tuning float32_dense = 1 needs float32_general = 1 (the dense backend in float serves Float32 general handles)");
  if (o.float32_general_dense && !o.float32_general)
    return fail(CNL_ERR_ARG, f + ": tuning float32_general_dense needs float32_general = 1 (the general form of the dense backend in float serves Float32 general handles)");
  if (o.float32_general_dense < 0 || o.float32_general_dense > 2)
    return fail(CNL_ERR_ARG, f + ": tuning float32_general_dense is 0, 1 (plans with a front above order 64) or 2 (wherever the order and the batch allow)");
  if (o.float32_staged < 0 || o.float32_staged > 1)
    return fail(CNL_ERR_ARG, f + ": tuning float32_staged is 0 or 1 (latency plans of Float32 general handles run stage by stage)");
  if (o.float32_staged && !o.float32_general)
    return fail(CNL_ERR_ARG, f + ": tuning float32_staged = 1 needs float32_general = 1 (staged execution in float serves Float32 general handles)");
  if (o.float32_staged && o.float32_refine)
    return fail(CNL_ERR_ARG, f + ": tuning float32_staged = 1 does not go with float32_refine (no refined handle over a staged Float32 factor)");
  if (o.float32_latency < 0 || o.float32_latency > 1)
    return fail(CNL_ERR_ARG, f + ": tuning float32_latency is 0 or 1 (latency plans of Float32 general handles on the lean, dataflow and fused-ladder float instances)");
  if (o.float32_latency && !o.float32_general)
    return fail(CNL_ERR_ARG, f + ": tuning float32_latency = 1 needs float32_general = 1 (the latency path in float serves Float32 general handles)");
  if (o.float32_latency && o.float32_refine)
    return fail(CNL_ERR_ARG, f + ": tuning float32_latency = 1 does not go with float32_refine (no refined handle over a staged Float32 factor)");
  if (o.float32_blocked < 0 || o.float32_blocked > 1)
    return fail(CNL_ERR_ARG, f + ": tuning float32_blocked is 0 or 1 (the general kernel in float eliminates large fronts in panels of 16 pivots)");
  if (o.float32_blocked && !o.float32_general)
    return fail(CNL_ERR_ARG, f + ": tuning float32_blocked = 1 needs float32_general = 1 (the blocked float instances of the general kernel serve Float32 general handles)");
  if (o.float32_blocked && o.float32_refine)
    return fail(CNL_ERR_ARG, f + ": tuning float32_blocked = 1 does not go with float32_refine (no refined handle over a blocked Float32 factor)");
  if (o.float32_subtrees < 0 || o.float32_subtrees > 1)
    return fail(CNL_ERR_ARG, f + ": tuning float32_subtrees is 0 or 1 (the general kernel in float runs the subtrees of the elimination tree on workgroups of their own, stage by stage)");
  if (o.float32_subtrees && !o.float32_general)
    return fail(CNL_ERR_ARG, f + ": tuning float32_subtrees = 1 needs float32_general = 1 (the float subtree instances of the general kernel serve Float32 general handles)");
  if (o.float32_subtrees && o.float32_refine)
    return fail(CNL_ERR_ARG, f + ": tuning float32_subtrees = 1 does not go with float32_refine (no refined handle over a subtree Float32 factor)");
  return CNL_OK;
}

int check_no_general_blocked(const cnl::Tuning& o, const char* fn) {
  if (o.general_blocked)
    return fail(CNL_ERR_ARG, std::string(fn) + ": tuning general_blocked = 1 is served by Float64 handles only (a Float32 general handle takes its blocked instances with tuning float32_blocked)");
  if (o.general_subtrees)   // (tuning general_subtrees: the same rule — the float subtree instances have a key of their own, float32_subtrees; the message is kept word for word)
    return fail(CNL_ERR_ARG, std::string(fn) + ": tuning general_subtrees = 1 is served by Float64 handles only (the general kernel has no Float32 subtree instances)");
  return CNL_OK;
}

int check_subtree_ladder(const cnl::Tuning& o, bool f32, const char* fn) {
  if (o.subtree_ladder && !(f32 ? o.float32_subtrees : o.general_subtrees))
    return fail(CNL_ERR_ARG, std::string(fn) + (f32 ? ": tuning subtree_ladder needs float32_subtrees = 1 at a Float32 creator (the rungs run on the float subtree instances)"
                                                    : ": tuning subtree_ladder needs general_subtrees = 1 at a Float64 creator (the rungs run on the Float64 subtree instances)"));
  // tuning subtree_wide, subtree_lds_panels: the same rule, and the panels need the creator's own blocked key
  if ((o.subtree_wide || o.subtree_lds_panels) && !(f32 ? o.float32_subtrees : o.general_subtrees))
    return fail(CNL_ERR_ARG, std::string(fn) + (f32 ? ": tuning subtree_wide / subtree_lds_panels need float32_subtrees = 1 at a Float32 creator (they shape the stage launches of the float subtree instances)"
                                                    : ": tuning subtree_wide / subtree_lds_panels need general_subtrees = 1 at a Float64 creator (they shape the stage launches of the Float64 subtree instances)"));
  if (o.subtree_lds_panels && !(f32 ? o.float32_blocked : o.general_blocked))
    return fail(CNL_ERR_ARG, std::string(fn) + (f32 ? ": tuning subtree_lds_panels needs float32_blocked = 1 at a Float32 creator (the pivot panels are those of the float blocked instances)"
                                                    : ": tuning subtree_lds_panels needs general_blocked = 1 at a Float64 creator (the pivot panels are those of the Float64 blocked instances)"));
  // tuning subtree_solve_panels: the creator's own subtree key again
  if (o.subtree_solve_panels && !(f32 ? o.float32_subtrees : o.general_subtrees))
    return fail(CNL_ERR_ARG, std::string(fn) + (f32 ? ": tuning subtree_solve_panels needs float32_subtrees = 1 at a Float32 creator (it shapes the solve sweeps of the float subtree instances)"
                                                    : ": tuning subtree_solve_panels needs general_subtrees = 1 at a Float64 creator (it shapes the solve sweeps of the Float64 subtree instances)"));
  return CNL_OK;
}

cnl::Tuning f32_unstaged_options(const cnl::Tuning& o) {
  cnl::Tuning u = o;
  u.float32_staged = 0; u.float32_latency = 0; u.float32_register_front = 1; u.float32_direct_records = 1;
  if (!u.float32_condense) u.float32_condense = 1;
  return u;
}

bool f32_general_dense_fits(const cnl_plan* plan, int64_t batch) {
  return batch <= 16 || (double)batch * 3.0 * 16384.0 * std::pow(std::ceil((double)plan->C.N2 / 64.0), 2) <= 8e9;
}

int f32_general_plan(cnl_plan** plan, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar, int64_t nequ, int64_t ncon,
                     const cnl::Tuning& o, cnl::Tuning* used, int64_t batch) {
  if (o.float32_staged || o.float32_latency) {
    // Tuning float32_staged: the latency analysis exactly where plan_create_tuned makes it for a Float64 handle, with the tuning of
    // the float direct records plus staged execution — no split plan, no tail.  A plan that cannot run staged (the conditions of
    // plan_create_impl: tasks, direct records, d in the caller's numbering, every condensed pivot counted by a front), a batch
    // planned for throughput, and every pattern float32_dense / float32_general_dense serve get the plan they get without the key.
    const cnl::Tuning u = f32_unstaged_options(o);
    int latency = 0;
    if (o.plan_kind == CNL_PLAN_LATENCY) latency = 1;
    else if (o.plan_kind == CNL_PLAN_AUTO) latency = batch >= 1 && batch <= (o.staged_max_batch > 0 ? o.staged_max_batch : 4096);
    else if (o.plan_kind != CNL_PLAN_THROUGHPUT) return fail(CNL_ERR_ARG, "unknown plan_kind");
    if (latency && batch < 1) return fail(CNL_ERR_ARG, "a latency plan needs the batch size");
    if (latency && ((u.float32_dense && u.dense_backend) || u.float32_general_dense)) {
      if (int rc = f32_general_plan(plan, N, nnz, rows1, cols1, nvar, nequ, ncon, u, used, batch)) return rc;
      const cnl_plan* p = *plan;
      const int gd = u.float32_general_dense;
      if (p->D.active || (gd && p->C.active && !p->gpos.empty() && (gd == 2 || p->P.fmax > 64) && f32_general_dense_fits(p, batch))) return CNL_OK;
      cnl_plan_destroy(*plan);
      *plan = nullptr;
    }
    if (latency) {
      cnl::Tuning g = u;
      g.float32_staged = 1;
      g.condense = 1; g.register_front = 1; g.direct_records = 1; g.lean_kernel = 0; g.rows_in_backward = 0;
      // Tuning float32_latency on top: the caller's lean_kernel / rows_in_backward go through, so that
      // plan_create_impl shapes the plan for the lean float instances as it does for a Float64 handle — the row form on every front
      // where that makes the plan lean, fronts with more than 16 residual rows cut in two, backward rows
      if (o.float32_latency) { g.float32_latency = 1; g.lean_kernel = o.lean_kernel; g.rows_in_backward = o.rows_in_backward; }
      g.dense_backend = 0; g.general_dense = 0; g.band_kernel = 0; g.staged = 1;
      const int nquads = (int)((batch + 3) / 4);
      if (int rc = plan_create_impl(plan, N, nnz, rows1, cols1, nvar, nequ, ncon, 1, std::max(1, 2048 / nquads), 2048.0 / nquads, g)) return rc;
      const cnl_plan* p = *plan;
      const bool stageable = p->latency && !p->P.tasks.empty() && p->P.v2_ok && p->P.rec_direct && p->P.d_outer &&
                             p->P.d_owned == (int64_t)p->C.r_dsrc.size();
      if (stageable) { if (used) *used = g; return CNL_OK; }
      cnl_plan_destroy(*plan);
      *plan = nullptr;
    }
    return f32_general_plan(plan, N, nnz, rows1, cols1, nvar, nequ, ncon, u, used, batch);
  }
  // The throughput analysis with nothing but the general kernel to run, whatever the caller's options say: no condensation (a call
  // is then the one classic launch) unless tuning float32_condense asks for it (the call is then that launch between the float
  // condensation passes), no register-front records, no dense routes, no staged execution, no band program.
  cnl::Tuning g = o;
  g.condense = o.float32_condense ? 1 : 0; g.register_front = 0; g.dense_backend = 0; g.general_dense = 0; g.staged = 0; g.band_kernel = 0;
  // tuning float32_subtrees: the analysis cuts the tree for the general kernel (Options::general_subtrees) and gives every task region
  // the staging rows choose_config sizes for this handle (Options::gsub_rows: 16 with float32_blocked, else 2).  The creators refuse the
  // caller's own general_subtrees / general_blocked before they come here, so both keys of g are the analysis's alone; the handle reads
  // float32_subtrees and float32_blocked (setup_subtrees, choose_config).  Plan::gwork and the offsets count elements: floats here.
  if (o.float32_subtrees) { g.general_subtrees = 1; g.general_blocked = o.float32_blocked ? 1 : 0; }
  // (a dense residual block holds nvar * nequ Jacobian entries, nequ diagonal entries and the nvar rho slots at least: a pattern
  //  with fewer entries is not analysed a second time for the question)
  if (o.float32_dense && o.dense_backend && nequ > 0 && nnz / nequ >= nvar) {
    // tuning float32_dense: a dense residual block goes to the dense backend in float, whatever the batch (as a Float64 handle's
    // does).  The uncondensed analysis runs detect_dense on the validated pattern; a pattern it does not accept — and every pattern
    // with cnl_options.dense_backend = 0 — goes on to exactly the handle it gets without the key.
    cnl::Tuning gd = g;
    gd.condense = 0; gd.float32_condense = 0; gd.float32_register_front = 0; gd.float32_direct_records = 0; gd.dense_backend = 1;
    if (int rc = plan_create_impl(plan, N, nnz, rows1, cols1, nvar, nequ, ncon, 0, 0, 0, gd)) return rc;
    if ((*plan)->D.active) { if (used) *used = gd; return CNL_OK; }
    cnl_plan_destroy(*plan);
    *plan = nullptr;
  }
  if (o.float32_register_front) {
    // ... or, tuning float32_register_front, with the register-front records of the condensed system: the call is the float
    // condensation passes around ONE launch of the register-front kernel in float (solve_ldl!: of the general kernel, which
    // reads the same panels).  Implies float32_condense.
    if (!g.float32_condense) g.float32_condense = 1;
    g.condense = 1; g.register_front = 1; g.direct_records = 0;
    // ... or, tuning float32_direct_records on top, with DIRECT records: the kernel condenses on the fly from the caller's vals and
    // the call is that one launch and the post-pass.  No lean or solve-only float instance exists, so the plan is not shaped for
    // one (no row form forced on every front, no backward rows).
    if (o.float32_direct_records) { g.direct_records = 1; g.lean_kernel = 0; g.rows_in_backward = 0; }
  }
  if (o.float32_general_dense) {
    // ... or, tuning float32_general_dense, as ONE dense matrix: the analysis keeps the position of every slot of the condensed
    // system wherever its order is 96 .. 4096 (plan->gpos), and the handle decides by the fronts and the batch
    // (create_f32_general_from_plan).  Implies float32_condense.
    if (!g.float32_condense) g.float32_condense = 1;
    g.condense = 1; g.general_dense = 2;
  }
  if (used) *used = g;
  return plan_create_impl(plan, N, nnz, rows1, cols1, nvar, nequ, ncon, 0, 0, 0, g);
}

int plan_create_tuned(cnl_plan** plan, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar,
                      int64_t nequ, int64_t ncon, int64_t batch, const cnl::Tuning& o) {
  int rc = CNL_OK;
  int latency = 0;
  if (o.plan_kind == CNL_PLAN_LATENCY) latency = 1;
  else if (o.plan_kind == CNL_PLAN_AUTO) latency = batch >= 1 && batch <= (o.staged_max_batch > 0 ? o.staged_max_batch : 4096);
  else if (o.plan_kind != CNL_PLAN_THROUGHPUT) return fail(CNL_ERR_ARG, "unknown plan_kind");
  if (!latency) {
    rc = plan_create_impl(plan, N, nnz, rows1, cols1, nvar, nequ, ncon, 0, 0, 0, o);
    // Between one and two wavefronts per SIMD the single stream leaves wavefront slots idle (686 k systems/s at 5120 problems of
    // cfg3's pattern between 958 k at 4096 and 964 k at 8192): when the bidirectional chain is available at the throughput
    // order's cost, the handle runs part of the batch on it and the rest single-stream, concurrently (capi_run.cpp, run_split).
    const int64_t smb = o.staged_max_batch > 0 ? o.staged_max_batch : 4096;
    if (rc == CNL_OK && o.plan_kind == CNL_PLAN_AUTO && o.split_batch && batch > smb && batch <= 2 * smb - smb / 8 && o.force_order[0] == 0) {
      cnl::Tuning o2 = o;
      std::snprintf(o2.force_order, sizeof(o2.force_order), "ndc2+early");
      cnl_plan* alt = nullptr;
      const int nq = (int)((smb + 3) / 4);
      if (plan_create_impl(&alt, N, nnz, rows1, cols1, nvar, nequ, ncon, 1, std::max(1, 2048 / nq), 2048.0 / nq, o2) == CNL_OK) {
        const bool same_work = alt->latency && alt->P.order_name == "ndc2+early" && alt->P.tasks.size() >= 2 &&
                               alt->P.cost <= 1.05 * (*plan)->P.cost && alt->P.nsuper <= (*plan)->P.nsuper + 8;
        if (same_work) {
          alt->split_mode = true;
          std::memset(alt->opt.force_order, 0, sizeof(alt->opt.force_order));
          cnl_plan_destroy(*plan);
          *plan = alt;
        } else {
          cnl_plan_destroy(alt);
        }
      }
    }
    return rc;
  }
  if (batch < 1) return fail(CNL_ERR_ARG, "a latency plan needs the batch size");
  const int nquads = (int)((batch + 3) / 4);
  return plan_create_impl(plan, N, nnz, rows1, cols1, nvar, nequ, ncon, 1, std::max(1, 2048 / nquads), 2048.0 / nquads, o);
}

extern "C" {

const char* cnl_last_error(void) { return g_err.c_str(); }
// 0.2.0 (round 4: in-kernel device ladder, cnl_options grew); 0.3.0: cnl_set_active_batch, cnl_outer_compact_dev;
// 0.3.1: tuning float32_general (Float32 handles on the general multifrontal kernel), no new symbol
// 0.4.0: cnl_outer_ctl, cnl_outer_*_ex_dev, cnl_outer_hess_mask_dev
// 0.4.1: tuning float32_register_front (the register-front kernel in float for Float32 general handles), no new symbol
// 0.4.2: tuning float32_direct_records (Float32 general handles on the Direct route), cnl_get_config bits 36 / 37, no new symbol
// 0.4.3: tuning float32_dense (Float32 general handles with a dense residual block on the dense backend in float), no new symbol
// 0.4.4: tuning float32_general_dense (Float32 general handles with large fronts on the general form of the dense backend in float), no new symbol
// 0.5.0: tuning float32_refine (Float64 handles on a Float32 factor, refined with a Float64 residual), cnl_kkt_residual_dev,
//        cnl_get_refine_norms, cnl_plan_get "kkt_row_*", cnl_get_config bits 38 .. 41
// 0.5.1: tuning float32_staged (latency plans of Float32 general handles run stage by stage on the float register-front kernel), no new symbol
// 0.5.2: tuning float32_latency (lean, dataflow and fused-ladder float instances of the register-front kernel behind float32_staged),
//        cnl_get_config bits 42 .. 44, no new symbol
// 0.5.3: tuning cgls_wide (row f4 with its ncon-vectors in the global workspace: more than 1024 constraints), cnl_get_config bits 45 / 46,
//        no new symbol
// 0.5.4: tuning general_blocked (the general kernel's blocked instances, Float64), cnl_get_config bit 47, no new symbol
// 0.5.5: tuning float32_blocked (the general kernel's blocked instances in float, for Float32 general handles), cnl_get_config bit 48,
//        no new symbol
// 0.5.6: tuning general_subtrees (the general kernel stage by stage, one workgroup per problem and task of the elimination tree, Float64),
//        cnl_get_config bit 49, cnl_plan_get "gtasks" / "gstage_ptr" / "gfronts" / "ginfo", no new symbol
// 0.5.7: tuning float32_subtrees (the general kernel stage by stage in float, for Float32 general handles), cnl_get_config bit 50,
//        no new symbol
// 0.5.8: tuning subtree_ladder (subtree handles of either element type climb R rungs of the rho ladder stage by stage), cnl_get_config
//        bits 51 .. 57, no new symbol
// 0.5.9: tuning subtree_wide (1024-thread factorising stages on 256-thread subtree handles, the float instances among them) and
//        subtree_lds_panels (dependent pivot panels of blocked subtree handles in LDS), cnl_get_config bits 58 / 59, cnl_subtree_stage_shape
// 0.5.10: tuning subtree_solve_panels (the solve sweeps of subtree handles in panels of 16 pivots, entries of their own), cnl_get_config
//        bits 60 / 61, no new symbol
// 0.5.11: tuning band_cache_policy (cache policy of the band kernel's mover-table instance), cnl_get_config bits 18 .. 22 (bits 16 / 17
//        keep the parts of the chain), no new symbol
int32_t cnl_version(void) { return 511; }

void cnl_default_params(double p[9]) {
  const double eps = 2.220446049250313e-16;  // eps(Float64); src/CaNNOLeS.jl:48-62
  p[0] = eps;
  p[1] = std::sqrt(eps);
  p[2] = 1.0 / 3.0;
  p[3] = 8.0;
  p[4] = std::min(100.0, 8.0 * 16.0);
  p[5] = std::pow(eps, 1.0 / 3.0);  // the reference writes eps^T(1/3): pow with the exponent 0.333..., NOT cbrt (2.5 ulp apart)
  p[6] = std::pow(eps, -2.0);
  p[7] = std::sqrt(eps);
  p[8] = std::pow(eps, 0.25);
}

void cnl_options_init(cnl_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  const cnl::Tuning t;   // the defaults live in options.h
  o->struct_size = (int32_t)sizeof(cnl_options);
  o->plan_kind = t.plan_kind;
  // measured on MI355X (cfg3 pattern, tools/cmp_staged_threshold.py): latency plans with a few large canonical parts reach
  // 600 k systems/s at 2048 problems and 613 k at 4096 (the single stream: 342 k and 567 k); from 5120 on the single stream wins
  o->staged_max_batch = t.staged_max_batch;
  o->verbose = t.verbose; o->band_kernel = t.band_kernel; o->dense_backend = t.dense_backend; o->staged = t.staged; o->dataflow = t.dataflow;
  o->device_ladder = t.device_ladder; o->host_ladder = t.host_ladder; o->split_tail = t.split_tail; o->multi_share_plan = t.multi_share_plan;
  o->batch_layout = t.batch_layout;
}

void cnl_default_params_f32(float p[9]) {
  // src/CaNNOLeS.jl:48-62 with T = Float32, each value what Julia computes on Float32 operands, rounded once
  const float eps = FLT_EPSILON;   // eps(Float32) = 2^-23
  p[0] = eps;
  p[1] = std::sqrt(eps);
  p[2] = 1.0f / 3.0f;
  p[3] = 8.0f;
  p[4] = std::min(100.0f, (float)(sizeof(float) * 16));   // sizeof(T) * 16 = 64
  p[5] = (float)std::pow((double)eps, (double)(1.0f / 3.0f));   // eps^(T(1)/3), the Float32 exponent
  p[6] = (float)std::pow((double)eps, -2.0);
  p[7] = std::sqrt(eps);
  p[8] = (float)std::pow((double)eps, 0.25);
}

int cnl_plan_create_ex(cnl_plan** plan, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar,
                       int64_t nequ, int64_t ncon, int64_t batch, const cnl_options* opt) {
  cnl::Tuning o;
  int rc = resolve_options(opt, o);
  if (rc) return rc;
  if (o.float32_refine) {   // the plan of the refined handle is its inner Float32 general handle's
    if ((rc = check_f32_options(o, "cnl_plan_create_ex"))) return rc;
    if ((rc = check_no_general_blocked(o, "cnl_plan_create_ex (the inner Float32 handle of tuning float32_refine)"))) return rc;
    if (!plan) return fail(CNL_ERR_ARG, "null argument");
    return f32_general_plan(plan, N, nnz, rows1, cols1, nvar, nequ, ncon, o);
  }
  if (o.float32_staged || o.float32_latency) {   // the plan cnl_create_f32_ex makes behind the band kernels for this batch
    if ((rc = check_f32_options(o, "cnl_plan_create_ex"))) return rc;
    if (!plan) return fail(CNL_ERR_ARG, "null argument");
    return f32_general_plan(plan, N, nnz, rows1, cols1, nvar, nequ, ncon, o, nullptr, batch);
  }
  return plan_create_tuned(plan, N, nnz, rows1, cols1, nvar, nequ, ncon, batch, o);
}

int cnl_plan_create(cnl_plan** plan, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar,
                    int64_t nequ, int64_t ncon) {
  return cnl_plan_create_ex(plan, N, nnz, rows1, cols1, nvar, nequ, ncon, 0, nullptr);
}

int cnl_plan_create_for_batch(cnl_plan** plan, int64_t N, int64_t nnz, const int64_t* rows1, const int64_t* cols1, int64_t nvar,
                              int64_t nequ, int64_t ncon, int64_t batch) {
  if (batch < 1) return fail(CNL_ERR_ARG, "batch out of range");
  return cnl_plan_create_ex(plan, N, nnz, rows1, cols1, nvar, nequ, ncon, batch, nullptr);
}

void cnl_plan_destroy(cnl_plan* plan) {
  if (plan && plan->refs.fetch_sub(1) == 1) delete plan;
}

int cnl_plan_info(const cnl_plan* plan, int64_t info[16]) {
  if (!plan || !info) return fail(CNL_ERR_ARG, "null argument");
  const cnl::Plan& P = plan->P;
  std::memset(info, 0, 16 * sizeof(int64_t));
  info[0] = plan->N; info[1] = plan->nnz; info[2] = P.nnzK; info[3] = P.nsuper; info[4] = P.nnzL; info[5] = P.nnzL_exact;
  if (plan->C.active) {  // the L rows of the condensed residual pivots (J_r / d_r) belong to the factor too
    info[4] += (int64_t)plan->C.r_jsrc.size();
    info[5] += (int64_t)plan->C.r_jsrc.size();
  }
  info[6] = P.lsize; info[7] = P.fmax; info[8] = P.fwd_peak; info[9] = P.bwd_peak; info[10] = P.panel_max;
  info[11] = (int64_t)P.flops; info[12] = (int64_t)P.asm_src.size();
  info[13] = P.v2_ok ? ((int64_t)P.ncls[0] | ((int64_t)P.ncls[1] << 20) | ((int64_t)P.ncls[2] << 40)) : -1;
  info[14] = P.v2_ok ? ((int64_t)P.u2_peak | ((int64_t)P.fs2_max << 20) | ((int64_t)std::max(P.rec_maxlen, P.brec_maxlen) << 40)) : -1;
  info[15] = plan->C.active ? (int64_t)plan->C.r_orig.size() : 0;  // condensed residual nodes
  return CNL_OK;
}

const char* cnl_plan_order_name(const cnl_plan* plan) { return plan ? plan->P.order_name.c_str() : ""; }

int cnl_plan_get(const cnl_plan* plan, const char* name, int32_t* out, int64_t* count) {
  if (!plan || !name || !count) return fail(CNL_ERR_ARG, "null argument");
  const cnl::Plan& P = plan->P;
  const int32_t* src = nullptr;
  int64_t n = 0;
  std::string s(name);
  const cnl::Cond& C = plan->C;
  if (s == "perm") { src = plan->perm_outer.data(); n = (int64_t)plan->perm_outer.size(); }
  else if (s == "inner_perm") { src = P.perm.data(); n = (int64_t)P.perm.size(); }
  else if (s == "c_ptr") { src = C.c_ptr.data(); n = (int64_t)C.c_ptr.size(); }
  else if (s == "c_a") { src = C.c_a.data(); n = (int64_t)C.c_a.size(); }
  else if (s == "c_b") { src = C.c_b.data(); n = (int64_t)C.c_b.size(); }
  else if (s == "c_d") { src = C.c_d.data(); n = (int64_t)C.c_d.size(); }
  else if (s == "orig_of") { src = C.orig_of.data(); n = (int64_t)C.orig_of.size(); }
  else if (s == "r_orig") { src = C.r_orig.data(); n = (int64_t)C.r_orig.size(); }
  else if (s == "r_dsrc") { src = C.r_dsrc.data(); n = (int64_t)C.r_dsrc.size(); }
  else if (s == "r_ptr") { src = C.r_ptr.data(); n = (int64_t)C.r_ptr.size(); }
  else if (s == "r_jsrc") { src = C.r_jsrc.data(); n = (int64_t)C.r_jsrc.size(); }
  else if (s == "r_jx") { src = C.r_jx.data(); n = (int64_t)C.r_jx.size(); }
  // rows of the full symmetric matrix (refine.h: KktRows), built on first request
  else if (s == "kkt_row_ptr") { const cnl::KktRows& R = kkt_rows(plan); src = R.ptr.data(); n = (int64_t)R.ptr.size(); }
  else if (s == "kkt_row_slot") { const cnl::KktRows& R = kkt_rows(plan); src = R.slot.data(); n = (int64_t)R.slot.size(); }
  else if (s == "kkt_row_col") { const cnl::KktRows& R = kkt_rows(plan); src = R.col.data(); n = (int64_t)R.col.size(); }
  else if (s == "cond_info") {
    // which condense kernel serves the plan (kernels_aux.hip): {1 the LDS-tiled kernel / 0 the plain slot kernel, largest tile in
    // elements, largest contribution and slot count of a chunk, chunks}; empty where the plan is not condensed
    static thread_local int32_t ci[5];
    const int32_t v[5] = {C.tiled_ok ? 1 : 0, C.tile_max, C.chunk_ncon_max, C.chunk_nslot_max, C.ch_region[3]};
    std::memcpy(ci, v, sizeof(ci));
    src = ci; n = C.active ? 5 : 0;
  }
  else if (s == "fronts") { src = reinterpret_cast<const int32_t*>(P.fronts.data()); n = (int64_t)P.fronts.size() * 16; }
  else if (s == "seg_ptr") { src = P.seg_ptr.data(); n = (int64_t)P.seg_ptr.size(); }
  else if (s == "asm_pos") { src = P.asm_pos.data(); n = (int64_t)P.asm_pos.size(); }
  else if (s == "asm_src") { src = P.asm_src.data(); n = (int64_t)P.asm_src.size(); }
  else if (s == "child_idx") { src = P.child_idx.data(); n = (int64_t)P.child_idx.size(); }
  else if (s == "rel_idx") { src = P.rel_idx.data(); n = (int64_t)P.rel_idx.size(); }
  else if (s == "tasks") { src = reinterpret_cast<const int32_t*>(P.tasks.data()); n = (int64_t)P.tasks.size() * 8; }  // struct Task, csrc/plan.h
  else if (s == "stage_ptr") { src = P.stage_ptr.data(); n = (int64_t)P.stage_ptr.size(); }
  // subtree execution of the general kernel (tuning general_subtrees; plan.h: GTask): empty without the key
  else if (s == "gtasks") { src = reinterpret_cast<const int32_t*>(P.gtasks.data()); n = (int64_t)P.gtasks.size() * 8; }
  else if (s == "gstage_ptr") { src = P.gstage_ptr.data(); n = (int64_t)P.gstage_ptr.size(); }
  else if (s == "gfronts") { src = reinterpret_cast<const int32_t*>(P.gfronts.data()); n = (int64_t)P.gfronts.size() * 16; }
  else if (s == "ginfo") {
    // {gwork: elements of work area per problem with every task region side by side, tasks, stages, tasks of the first stage, cap}
    static thread_local int32_t gi[5];
    const int32_t nst = (int32_t)P.gstage_ptr.size() - 1;
    const int32_t v[5] = {(int32_t)P.gwork, (int32_t)P.gtasks.size(), nst < 0 ? 0 : nst, nst >= 1 ? P.gstage_ptr[1] : 0, P.gcap};
    std::memcpy(gi, v, sizeof(gi));
    src = gi; n = P.gtasks.empty() ? 0 : 5;
  }
  else if (s == "rec") { src = P.rec.data(); n = P.v2_ok ? (int64_t)P.rec.size() : 0; }     // record streams of the
  else if (s == "brec") { src = P.brec.data(); n = P.v2_ok ? (int64_t)P.brec.size() : 0; }  // register-front kernel
  else if (s.rfind("band", 0) == 0) {
    // band programs (csrc/band.h): "band_*" the 15-piece program, "band4_*" the same for 4-byte elements, "bandw_*" / "bandw4_*" the
    // wide program (its piece count: info[7]); "<prefix>info", and per part q "<prefix>part<q>", "fops<q>", "bops<q>", "epochs<q>", "borders<q>"
    // (every prefix ends with the '_' another has a letter or digit at: at most one matches)
    const cnl_plan::BandSlot* f = nullptr;
    size_t plen = 0;
    for (int t = 0; t < 2; t++)
      for (int w = 0; w < 2; w++)
        if (s.rfind(kBandPrefix[t][w], 0) == 0) { f = &plan->band_prog[t][w]; plen = std::strlen(kBandPrefix[t][w]); }
    // "bandr_*": the resident form of "band_*" (band.h; info[0] = 0 where the plan has none)
    if (s.rfind(kBandResPrefix, 0) == 0) { f = &plan->band_res; plen = std::strlen(kBandResPrefix); }
    // "bandm_*": the mover table of "bandr_*" (band.h, BAND_MK_*): "bandm_info", "bandm_table<q>" (empty where the plan has none)
    const bool mov = s.rfind(kBandMovPrefix, 0) == 0;
    if (mov) { f = &plan->band_res; plen = std::strlen(kBandMovPrefix); }
    if (!f) return fail(CNL_ERR_ARG, "unknown plan array: " + s);
    const std::string rest = s.substr(plen);
    if (mov) {
      if (rest == "info") { src = plan->band_mov_info.data(); n = (int64_t)plan->band_mov_info.size(); }
      else if (rest == "table0" || rest == "table1") { const cnl::BandPart& Q = f->B.part[rest.back() - '0']; src = Q.mover.data(); n = (int64_t)Q.mover.size(); }
      else return fail(CNL_ERR_ARG, "unknown plan array: " + s);
    }
    else if (rest == "info") { src = f->info.data(); n = (int64_t)f->info.size(); }
    else if (!rest.empty() && (rest.back() == '0' || rest.back() == '1')) {
      const int q = rest.back() - '0';
      const cnl::BandPart& Q = f->B.part[q];
      const std::string k = rest.substr(0, rest.size() - 1);
      if (k == "part") { src = f->pinfo[q].data(); n = (int64_t)f->pinfo[q].size(); }
      else if (k == "fops") { src = Q.fops.data(); n = (int64_t)Q.fops.size(); }
      else if (k == "bops") { src = Q.bops.data(); n = (int64_t)Q.bops.size(); }
      else if (k == "epochs") { src = Q.epochs.data(); n = (int64_t)Q.epochs.size(); }
      else if (k == "borders") { src = Q.borders.data(); n = (int64_t)Q.borders.size(); }
      else return fail(CNL_ERR_ARG, "unknown plan array: " + s);
    }
    else return fail(CNL_ERR_ARG, "unknown plan array: " + s);
  }
  else return fail(CNL_ERR_ARG, "unknown plan array: " + s);
  if (out) {
    if (*count < n) return fail(CNL_ERR_ARG, "buffer too small");
    std::memcpy(out, src, (size_t)n * sizeof(int32_t));
  }
  *count = n;
  return CNL_OK;
}

}  // extern "C"
