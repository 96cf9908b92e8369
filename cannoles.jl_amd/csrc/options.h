// options.h — every plan / execution switch of the library, internal.
//
// The PUBLIC structure (include/cannoles_hip.h: cnl_options) carries the dozen switches a caller or a test may reasonably want
// — plan kind, batch threshold, verbosity, which kernel families and executions are allowed — plus a `tuning` string of
// "key=value" pairs for everything else below (measurement tools, ablations, the randomised option fuzz).  Inside the library
// there is only this structure; nothing here is read from the environment.
//
// Measured-slower experiments stay reachable through `tuning` only (device_ladder_fused = 1, split_batch = 2); switches that had
// become no-ops (staged_large_fronts) or whose two settings measured equal (band_wide_pieces) were removed in round 6.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

namespace cnl {

// name, default.  (plan_kind: CNL_PLAN_AUTO = 0)
#define CNL_TUNING_INT_FIELDS(X)                                                                                              \
  X(plan_kind, 0)            /* CNL_PLAN_*                                                                                  */ \
  X(order_mode, -1)          /* -1 auto (cost model over all candidates), 0 canonical, 1 nested dissection, 2 minimum degree */ \
  X(nd_leaf, 0)              /* nested-dissection leaf size, 0 = sweep                                                      */ \
  X(relax, -1)               /* relaxed-amalgamation budget (explicit zeros per merged column), -1 = default                */ \
  X(task_cap, 0)             /* fronts per bottom task of a latency plan (and of the cut of general_subtrees), 0 = default  */ \
  X(multipliers_early, 1)    /* candidates with every multiplier right behind the last variable it touches are considered   */ \
  X(condense, 1)             /* static condensation of the -I block                                                         */ \
  X(direct_records, 1)       /* the register-front kernel condenses on the fly (no separate condense pass)                  */ \
  X(register_front, 1)       /* the register-front kernel may serve the plan (fronts of order <= 64)                        */ \
  X(dense_backend, 1)        /* dense residual blocks go to the dense backend                                               */ \
  X(general_dense, 1)        /* small batches of irregular plans with fronts > 64 as ONE dense matrix; 2: wherever possible */ \
  X(staged, 1)               /* latency plans run their first attempt stage by stage                                        */ \
  X(dataflow, 1)             /* smallest batches run all tasks in one launch per phase, waiting on device counters          */ \
  X(dataflow_waves, 1024)    /* at most this many wavefronts run in dataflow fashion                                        */ \
  X(dataflow_spin_limit, 1 << 22) /* polls before a dataflow wait gives up (counted: cnl_dataflow_timeouts; the call is redone) */ \
  X(waves_per_block, 0)      /* register-front kernel: wavefronts per workgroup, 0 = default (1)                            */ \
  X(v1_tpp, -1) X(v1_ppb, -1) X(v1_lds, -1) /* general kernel: threads per problem, problems per workgroup, work area in LDS */ \
  X(v1_solve, 0)             /* cnl_solve always runs on the general kernel                                                 */ \
  X(lds_pad, 1)              /* per-problem LDS areas 32 banks apart                                                        */ \
  X(ubig, 17)                /* update matrices of order above this live in global scratch                                  */ \
  X(wait_thr, 2)             /* ... and those that wait for more than this many fronts                                      */ \
  X(dense_graph, 1)          /* the dense backend replays its launch sequence as a hipGraph                                 */ \
  X(dense_syrk_wgs, 0)       /* workgroups of the J'WJ kernel, 0 = default                                                  */ \
  X(verbose, 0)              /* log plan decisions on stderr                                                                */ \
  X(multi_share_plan, 1)     /* cnl_multi_create analyses the pattern once for all shards of equal plan kind                */ \
  X(row_products, 1)         /* condensation products of small fronts organised per residual row (plan.h, RF_ROWS)          */ \
  X(split_batch, 1)          /* batches between one and two wavefronts per SIMD: 1 two halves on the chain, 2 chain || single stream (slower), 0 single stream */ \
  X(lean_kernel, 1)          /* plans of fast-class row-form fronts run the kernels' instantiation without the cold paths   */ \
  X(rows_in_backward, 1)     /* the lean kernel recovers the residual components in its backward sweep (no post-pass)       */ \
  X(dense_panel_blocks, 1)   /* dense backend, dn_panel2: 0 never, 1 while the step is latency-bound, 2 always              */ \
  X(host_ladder, 1)          /* host-pointer newton_system drives the rho ladder from the host where no device ladder runs  */ \
  X(device_ladder, 1)        /* staged handles climb the rho ladder inside one fused launch                                 */ \
  X(device_ladder_fused, 0)  /* that launch also makes the first attempt (measured slower: 0.140 against 0.118 ms)          */ \
  X(band_form, 1)            /* fast fronts with band-structured pivot rows skip the structurally zero row updates          */ \
  X(split_tail, 1)           /* the remainder of a batch above a machine-filling one runs on a handle of its own            */ \
  X(band_kernel, 1)          /* band-structured throughput handles run on the band kernels (band.h); 2: chain in one part   */ \
  X(band_problems_per_group, 0) /* band kernels: problems per workgroup (8, 16, 32); 0 = by batch                           */ \
  X(band_pieces, 0)          /* band program: operand pieces per epoch — 0: 15, the wide form (20) where a pattern needs it; 15: never wide; 20: wide wherever a band */ \
  X(band_resident, 1)        /* band program: the resident form (aligned blocks of vals kept in LDS, band.h) runs the handles it serves; 0: never built */ \
  X(band_mover_table, 1)     /* resident band program: the mover follows the host-built mover table (band.h, BAND_MK_*); 0: the resident instance decodes descriptors */ \
  X(analysis_threads, 0)     /* host threads of the symbolic analysis (candidate orders); 0 = by the hardware, at most 16      */ \
  X(f1_tiles, 1)             /* row f1 streams column tiles through LDS where the pattern allows; 0: gather kernel          */ \
  X(batch_layout, 0)         /* CNL_LAYOUT_*: layout of `vals` at the device-pointer entry points (band handles)            */ \
  X(band_rhs_interleaved, 0) /* measurement: the band kernels also take `rhs` interleaved (batch_layout = 1 handles)        */ \
  X(band_cache_policy, 7)    /* mover-table instance of the band kernel: cache policy mask over its once-touched streams (band.hip, BAND_POL_*) — 1 typed vals loads non-temporal, 2 typed factor loads non-temporal, 4 record stores non-temporal, 8 record stores written through (not with 4), 16 d stores non-temporal; only the masks that are built (band_policy_built: 0 and 7); every other instance ignores it; 7 measured 5.1 % faster than 0 at 16 384 problems */ \
  X(float32_general, 0)      /* cnl_create_f32: a pattern (or option set) the band kernels do not serve runs on the general kernel in float */ \
  X(float32_condense, 0)     /* ... on the condensed system (the -I block eliminated by the condensation passes in float); only with float32_general */ \
  X(float32_register_front, 0) /* ... with the register-front kernel in float between the condensation passes (implies float32_condense; fronts of order <= 64, else the float32_condense handle); only with float32_general */ \
  X(float32_direct_records, 0) /* ... on direct records: the float register-front kernel condenses on the fly from the caller's vals, and solve_ldl! stays on it where every front is of the fast class; only with float32_general and float32_register_front */ \
  X(float32_dense, 0)        /* cnl_create_f32: a dense residual block (the pattern detect_dense accepts) runs on the dense backend in float (dense_f32.hip), at any batch; every other pattern gets the handle it gets without the key; only with float32_general, and with dense_backend != 0 */ \
  X(float32_general_dense, 0) /* cnl_create_f32: a condensed system of order 96 .. 4096 whose plan has a front above order 64 runs as ONE dense matrix on the dense backend in float (dense_f32.hip, the general form), while the tiles fit (batch <= 16, or 3 float matrices of tiles within 8 GB); 2: whatever the fronts; implies float32_condense; every other pattern gets the handle it gets without the key; only with float32_general */ \
  X(float32_staged, 0)       /* cnl_create_f32: a batch a Float64 handle would plan for latency (plan_kind, staged_max_batch) gets a latency plan on direct records and runs it stage by stage on the float register-front kernel, one launch per stage (no dataflow, no in-kernel ladder; the problems that fail the first attempt climb the rho ladder in the classic launch behind it); implies float32_register_front, float32_direct_records and float32_condense; every other pattern or batch gets the handle it gets without the key; only with float32_general, not with float32_refine */ \
  X(float32_latency, 0)      /* cnl_create_f32: float32_staged, and the latency plan honours the switches a Float64 handle honours — lean_kernel, rows_in_backward, dataflow, dataflow_waves, dataflow_spin_limit, device_ladder, device_ladder_fused, by the Float64 defaults and rules: the lean, dataflow and fused-ladder float instances of the register-front kernel; implies float32_staged and what that implies; every plan that cannot run staged gets the handle it gets without the key; only with float32_general, not with float32_refine */ \
  X(float32_refine, 0)       /* cnl_create_ex / cnl_plan_create_ex: k = 1 .. 4: a Float64 handle on an inner Float32 general handle (made as cnl_create_f32_ex makes it from the same options, band_kernel forced to 0), whose solution is refined k times with a Float64 residual (refine.h); only with float32_general */ \
  X(refine_rows, 0)          /* the KKT residual kernel (refine.h): 0 by the pattern, 1 a row per lane, 2 a row per wavefront */ \
  X(general_blocked, 0)      /* general kernel, Float64: 1 = fronts with 16 pivots or more leave in panels of 16, trailing updates on the f64 matrix cores (configurations with 256 or 1024 threads per problem; the others run as without the key); Float64 handles only: cnl_create_f32* and float32_refine refuse it (the Float32 instances have a key of their own, float32_blocked) */ \
  X(float32_blocked, 0)      /* cnl_create_f32: general_blocked for a Float32 general handle: where its newton_system / factorize launches are the general kernel in float with 256 threads per problem, fronts with 16 pivots or more leave in panels of 16, trailing updates on the f32 matrix cores; selects no route: every handle gets the route it gets without the key, and 64 threads per problem run unblocked; 0 or 1; only with float32_general, not with float32_refine; a Float64 creator without float32_refine reads nothing of it, as of float32_condense */ \
  X(general_subtrees, 0)     /* general kernel, Float64: 1 = the elimination tree is cut into tasks (bottom subtrees of at most task_cap fronts, default 8; every front above on its own) and the three calls of the plugin surface run stage by stage, one workgroup per (problem, task), dependencies by launch order alone; acts where the launch is the general kernel with one problem per workgroup of 256 or 1024 threads, the first stage has two tasks or more and batch x gwork x 8 <= 8e9 bytes — every other handle is the one without the key; selects no route, combines with general_blocked; Float64 handles only: cnl_create_f32* and float32_refine refuse it */ \
  X(float32_subtrees, 0)     /* cnl_create_f32: general_subtrees for a Float32 general handle: the forced analysis cuts the tree (task_cap as there) and, where the newton_system / factorize launch is the general kernel in float with one problem per workgroup of 256 threads, the first stage has two tasks or more and batch x gwork x 4 <= 8e9 bytes, the three calls run stage by stage on the float subtree instances; selects no route: every other handle is the one without the key; combines with float32_blocked; 0 or 1; only with float32_general, not with float32_refine; a Float64 creator without float32_refine reads nothing of it, as of float32_condense */ \
  X(subtree_ladder, 0)       /* subtree handles of either element type: R = 0 .. 64 rungs of the rho ladder are enqueued behind the first attempt of newton_system, each stage by stage like it, one rung-decide launch behind each; problems still climbing after R rungs resume in the climbers' launch; (R + 2) S + R + 3 launches; valid only with general_subtrees = 1 (Float64 creators) or float32_subtrees = 1 (Float32 creators), never with float32_refine; selects no route and changes no plan: it acts where the subtree key acts */ \
  X(subtree_wide, 0)         /* subtree handles of either element type with 256 threads per workgroup: W = 1 .. 4096: the factorising forward launch of a stage (newton_system, factorize, the rungs of subtree_ladder) runs with 1024 threads per workgroup where the stage's largest task fmax F_s >= W and tasks_s x batch <= 2 x the device's CU count; every other launch keeps 256 (backward stages, solve_ldl!, climbers, decide and commit kernels); in float the only way to a 1024-thread instance; the factor and every output are bit-equal to W = 0; 0: off; valid only with general_subtrees = 1 (Float64 creators) or float32_subtrees = 1 (Float32 creators), never with float32_refine; selects no route and changes no plan */ \
  X(subtree_lds_panels, 0)   /* blocked subtree handles of either element type: M = 16 .. 4096: the factorising forward launch of a stage with F_s <= M, a front of at least 16 pivots and (16 + 32 F_s) elements within the device's LDS per workgroup (at most 160 KB) runs the LPAN instance, which eliminates the dependent pivot panels of its fronts in LDS (the panel's rows and their unscaled copies) with the statements of the global-memory loop in their order: bit-equal factor; 0: off; valid only with the creator's subtree key and its blocked key (general_blocked, float32_blocked), never with float32_refine; combines with subtree_wide; selects no route and changes no plan */ \
  X(subtree_solve_panels, 0) /* subtree handles of either element type, blocked or not, 256 threads per workgroup or a 1024-thread Float64 handle: a bit mask P = 0 .. 3 over the solve sweeps, which run in panels of 16 pivots on entries of their own (subtree_solve_kernel), the front's vector in dynamic LDS, the stored panel read in place — bit 0: the backward stage launches of newton_system and solve_ldl! (outer part of a panel: 16 dot products on lane groups, reduced by shuffles; its triangle on one wavefront; d agrees with P = 0 to rounding and is a fixed function of the front); bit 1: the forward stage launches of solve_ldl! (every operation of the unpanelled loop on every element in its order: bit-equal to P = 0); a stage whose (round4(F_s) + 288) elements exceed the device's LDS per workgroup (at most 160 KB) keeps today's launch; factorising launches, rungs, decide / commit kernels and climbers are untouched; 0: off; valid only with general_subtrees = 1 (Float64 creators) or float32_subtrees = 1 (Float32 creators), never with float32_refine; selects no route, changes no plan, allocation or launch count */ \
  X(cgls_wide, 0)          /* row f4: 0 the ncon-vectors in LDS, more than 1024 constraints are CNL_ERR_DIM; 1 in the global workspace where ncon > 1024; 2 there always */

struct Tuning {
#define X(name, dflt) int32_t name = dflt;
  CNL_TUNING_INT_FIELDS(X)
#undef X
  int64_t staged_max_batch = 4096;   // CNL_PLAN_AUTO: largest batch planned for latency
  char force_order[32] = {0};        // name of an ordering candidate to force ("" = none)
};

// sets one field by name; false: no such key
inline bool tuning_set(Tuning& t, const std::string& key, long long value) {
#define X(name, dflt) if (key == #name) { t.name = (int32_t)value; return true; }
  CNL_TUNING_INT_FIELDS(X)
#undef X
  if (key == "staged_max_batch") { t.staged_max_batch = value; return true; }
  return false;
}

// "key=value[,key=value...]" (separators: comma, semicolon, blank); returns "" or what is wrong
inline std::string tuning_parse(Tuning& t, const char* text) {
  std::string s(text ? text : "");
  size_t i = 0;
  while (i < s.size()) {
    while (i < s.size() && (s[i] == ',' || s[i] == ';' || s[i] == ' ')) i++;
    if (i >= s.size()) break;
    size_t j = i;
    while (j < s.size() && s[j] != ',' && s[j] != ';' && s[j] != ' ') j++;
    const std::string item = s.substr(i, j - i);
    i = j;
    const size_t eq = item.find('=');
    if (eq == std::string::npos || eq == 0 || eq + 1 >= item.size()) return "cnl_options.tuning: expected key=value, got '" + item + "'";
    const std::string key = item.substr(0, eq), val = item.substr(eq + 1);
    if (key == "force_order") {
      std::memset(t.force_order, 0, sizeof(t.force_order));
      std::strncpy(t.force_order, val.c_str(), sizeof(t.force_order) - 1);
      continue;
    }
    char* end = nullptr;
    const long long v = std::strtoll(val.c_str(), &end, 0);
    if (!end || *end != 0) return "cnl_options.tuning: value of '" + key + "' is not an integer";
    if (!tuning_set(t, key, v)) return "cnl_options.tuning: unknown key '" + key + "'";
  }
  return "";
}

}  // namespace cnl
