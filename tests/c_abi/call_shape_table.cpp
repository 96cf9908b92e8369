// Prints the table of csrc/call_shape.h, one line per (route facts, mode): tests/test_call_shape_cpu.py compares the lines with the
// rows it holds as literals.  Host only — the header includes nothing of HIP.  The flags only the Direct route reads are run through
// all 32 combinations there; on the other routes all clear and all set, which must give the same line.
#include <cstdio>

#include "../../cannoles.jl_amd/csrc/call_shape.h"

int main() {
  using namespace cnl;
  const Route routes[] = {Route::Band, Route::Dense, Route::GeneralDense, Route::Plain, Route::Direct, Route::Condensed};
  const char* route_name[] = {"Band", "Dense", "GeneralDense", "Plain", "Direct", "Condensed"};
  const char* mode_name[] = {"NEWTON", "FACTOR", "SOLVE"};
  const char* launch_name[] = {"band", "dense", "general_dense", "kernel", "staged"};
  for (int r = 0; r < 6; r++)
    for (int bits = 0; bits < 32; bits++) {
      if (routes[r] != Route::Direct && bits != 0 && bits != 31) continue;
      const RouteFacts f{routes[r], (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0};
      for (int mode = CALL_NEWTON; mode <= CALL_SOLVE; mode++) {
        const CallShape s = call_shape(f, mode);
        const char* cond = s.condense == NO_CONDENSE ? "-" : s.condense == MATRIX_ONLY ? "matrix" : s.condense == RHS_ONLY ? "rhs" : s.condense == WHOLE_SYSTEM ? "whole" : "?";
        std::printf("%s count_d=%d d_outer=%d v2_solve=%d lean_rows=%d staged=%d %s: condense=%s inertia=%d in=%s d=%s extra=%d launch=%s ", route_name[r], f.count_d,
                    f.d_outer, f.v2_solve, f.lean_rows, f.staged, mode_name[mode], cond, s.inertia, s.from_cbuf ? "cbuf" : "caller", s.d_to_d2 ? "d2" : "caller",
                    s.extra_counts, launch_name[(int)s.launch]);
        if (s.expand) std::printf("expand=%s,%s,%d ", s.expand_d2 ? "d2" : "null", s.expand_success ? "success" : "null", s.copy_rho_tail);
        else std::printf("expand=- ");
        std::printf("last_vals=%s%s\n", s.needs_last_vals ? "needed" : "", s.sets_last_vals ? "set" : (s.needs_last_vals ? "" : "unchanged"));
      }
    }
  return 0;
}
