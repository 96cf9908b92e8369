// call_shape.h — what ONE call on a handle consists of, as a table: call_shape() maps the handle's route (decided once, at creation)
// and the call's mode to the passes, arrays and launch form run() executes (capi_run.cpp).  Pure host code, no HIP include:
// tests/c_abi/call_shape_table.cpp compiles it alone and prints the table.
#pragma once
namespace cnl {
// Which backend serves the three calls of a handle.  Plain: no condensation; Direct: the register-front kernel condenses on the
// fly; Condensed: the stand-alone condensation passes surround the launch; GeneralDense: ... surround the dense LDL^T.
enum class Route { Band, Dense, GeneralDense, Plain, Direct, Condensed };
enum { CALL_NEWTON = 0, CALL_FACTOR = 1, CALL_SOLVE = 2 };   // (kernels.h: MODE_* — capi_run.cpp asserts they agree)
// which slots of the condensed buffer the condense pass forms: the values are the tiled kernel's mask (1 matrix, 2 rho, 4 rhs slots)
enum CondensePart { NO_CONDENSE = 0, MATRIX_ONLY = 3, RHS_ONLY = 4, WHOLE_SYSTEM = 7 };
// Kernel: one classic launch; Staged: the register-front kernel stage by stage + follow-up; Subtrees: the general kernel stage by stage,
// one workgroup per (problem, task), + decide and climbers (tuning general_subtrees)
enum class Launch { Band, Dense, GeneralDense, Kernel, Staged, Subtrees };

struct RouteFacts {
  Route route;
  // read on the Direct route alone — the kernel counts the condensed pivots itself; it writes the kept components of d itself;
  // solve_ldl! runs on it too; its lean instantiation recovers the residual components (no post-pass); the call runs stage by stage
  bool count_d, d_outer, v2_solve, lean_rows, staged;
  // read where the launch is the general kernel's (Plain, Condensed, and solve_ldl! of a Direct handle off the register-front kernel):
  // the handle runs it as subtree tasks, all three calls
  bool subtrees = false;
};

struct CallShape {
  CondensePart condense;  // pre-pass: condense these slots (SOLVE: from the last factorisation's values)
  bool inertia;           // pre-pass: count the condensed pivots
  bool from_cbuf;         // the launch reads the condensed buffer (else the caller's arrays; SOLVE on Band / Direct: last_vals),
  bool d_to_d2;           // writes the reduced solution (else the caller's d),
  bool extra_counts;      // and adds the inertia pass's counts to its own
  Launch launch;
  bool expand;            // post-pass, with: the reduced solution (else the kernel wrote the kept components), the success flags,
  bool expand_d2, expand_success, copy_rho_tail;   // and the rho slots copied back into the caller's vals
  bool needs_last_vals, sets_last_vals;   // the call reads the values of the last factorisation (an error before there was one) / makes its vals those
};

inline CallShape call_shape(const RouteFacts& f, int mode) {
  const bool newton = mode == CALL_NEWTON, factor = mode == CALL_FACTOR, solve = mode == CALL_SOLVE;
  CallShape s{NO_CONDENSE, false, false, false, false, Launch::Kernel, false, false, false, false, false, false};
  if (f.route == Route::Plain) { if (f.subtrees) s.launch = Launch::Subtrees; return s; }
  if (f.route == Route::Dense) { s.launch = Launch::Dense; return s; }   // (the dense backend keeps its own factor)
  s.needs_last_vals = solve; s.sets_last_vals = factor;
  if (f.route == Route::Band) { s.launch = Launch::Band; return s; }   // (no stored factor: the solve factorises the last values again)
  if (f.route == Route::Direct && (!solve || f.v2_solve)) {   // (solve_ldl! on the general kernel: as on a Condensed handle)
    s.launch = f.staged ? Launch::Staged : Launch::Kernel;
    s.inertia = s.extra_counts = !solve && !f.count_d;
    s.d_to_d2 = newton && !f.d_outer;
    s.expand = !factor && !f.lean_rows;
    s.expand_d2 = s.expand && s.d_to_d2;
    s.expand_success = s.expand && newton;
    return s;
  }
  // the condensation passes around a launch on the condensed system
  if (f.route == Route::GeneralDense) s.launch = Launch::GeneralDense;
  else if (f.subtrees) s.launch = Launch::Subtrees;
  s.condense = newton ? WHOLE_SYSTEM : factor ? MATRIX_ONLY : RHS_ONLY;
  s.inertia = s.extra_counts = !solve;
  s.from_cbuf = true;
  s.d_to_d2 = s.expand = s.expand_d2 = !factor;
  s.expand_success = newton;
  s.copy_rho_tail = newton && s.launch != Launch::GeneralDense;   // (the dense route writes the rho slots of the caller's vals itself)
  return s;
}

}  // namespace cnl
