// refine.h — mixed-precision refinement (tuning float32_refine): the row lists of the full symmetric KKT matrix, and the launchers of
// csrc/refine.hip.  A refined handle factorises in Float32 (its inner Float32 general handle) and recovers a Float64-accurate d with
// a few passes  g = rhs + K d  (Float64 data, double accumulation, g written as float),  e = solve(g)  on the kept Float32 factor,
// d += e.  The residual kernel is also a public call of its own (cnl_kkt_residual_dev).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

namespace cnl {

// CSR of the FULL matrix of a lower-triangular COO pattern: row i lists (slot, column) for every COO entry in row i or — mirrored,
// strict-lower entries only — in column i, in ascending slot order.  Duplicates stay separate entries: the gather sums them.
struct KktRows {
  std::vector<int32_t> ptr, slot, col;   // [N + 1], [nnz + strict-lower entries] twice
  int32_t max_row = 0;                   // entries of the longest row
};
void build_kkt_rows(KktRows& R, int64_t N, int64_t nnz, const int32_t* rows0, const int32_t* cols0);

// From this many entries per row ON AVERAGE the residual kernel gives every row a wavefront (lanes stride over the row's entries),
// below it a lane.  Measured on one MI355X at 4 096 problems (tools/time_f32_refine.py --rows): mean row 14.8
// (random_structure(60, 80, 4, 0.1, 1)): lane 0.054 ms, wavefront 0.111 ms; mean row 124.8 (dense_structure(100, 160)): lane 1.435 ms,
// wavefront 0.628 ms.  40 is the geometric middle of the two; the crossover itself has not been measured.
constexpr int KKT_WAVE_ROW_THRESHOLD = 40;
// the rows of a problem are cut into chunks, a workgroup each, until a launch has about this many workgroups
constexpr int KKT_TARGET_WORKGROUPS = 2048;

struct DevKktRows {
  const int32_t *ptr = nullptr, *slot = nullptr, *col = nullptr;
  int32_t N = 0;
  int64_t nnz = 0;
  int32_t wave_rows = 0;   // the instance: 0 a row per lane, 1 a row per wavefront
  // small batches: nchunk workgroups share a problem, rows_per_chunk consecutive rows each; the norm then is the maximum of
  // partial[b * nchunk + chunk], taken by a second, tiny launch (no atomics)
  int32_t nchunk = 1, rows_per_chunk = 0;
  double* partial = nullptr;   // [created batch][nchunk], nchunk > 1 only
};

// g[b] = rhs[b] + K(vals[b]) d[b], norms[b * norm_stride] = max |g[b]| (of the double sums), problems [0, batch); success != nullptr:
// problems with success[b] == 0 get g[b] = 0 and the norm -1.  norms may be null.  No atomics: every row has one owner.
hipError_t launch_kkt_residual(const DevKktRows& R, const double* vals, const double* rhs, const double* d, double* g, double* norms,
                               int64_t norm_stride, const int32_t* success, int batch, hipStream_t stream);
hipError_t launch_kkt_residual(const DevKktRows& R, const double* vals, const double* rhs, const double* d, float* g, double* norms,
                               int64_t norm_stride, const int32_t* success, int batch, hipStream_t stream);

// dst[i] = (float)src[i], i < n.  A value beyond FLT_MAX becomes inf (round to nearest): the Float32 factorisation then reports
// success = 0 for that problem — its data do not fit the factor's element type, and that is the honest answer.
hipError_t launch_refine_demote(const double* src, float* dst, int64_t n, hipStream_t stream);

// d[b] (+)= (double)e[b] where success[b] != 0 (success == nullptr: everywhere); rows of N elements; assign != 0: d[b] = (double)e[b]
hipError_t launch_refine_update(double* d, const float* e, const int32_t* success, int N, int batch, int assign, hipStream_t stream);

// what newton_system leaves beside d: rho[b], rho_old[b] widened (a float is exact in double), and the rho tail of the caller's
// Float64 vals = the widened tail of the float vals where the ladder wrote it (nfact[b] > 1)
hipError_t launch_refine_widen_rho(const float* rho32, const float* rho_old32, double* rho, double* rho_old, const float* vals32, double* vals,
                                   int64_t nnz, int nvar, const int32_t* nfact, int batch, hipStream_t stream);

}  // namespace cnl
