// refine.hip — the kernels of mixed-precision refinement (refine.h): the KKT residual g = rhs + K d of a batch that shares one
// pattern, the double -> float conversion of the inputs, and the masked update d += e.
//
// The residual gathers along the rows of the full matrix (KktRows: the host mirrors the strict-lower entries once per plan), so
// every output element has one owner and a fixed summation order: no atomics, bit-equal from call to call.  A workgroup of 256
// threads owns a problem, or — small batches — a chunk of its rows; the norm max |g[b]| is a reduction inside the workgroup
// (wavefront shuffles, then LDS) and, over chunks, a second tiny launch.  The index lists are the same for every problem and stay
// in L2.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "refine.h"

namespace cnl {

namespace {

constexpr int NT = 256, WAVE = 64, NW = NT / WAVE;

// fixed-shape butterfly over the 64 lanes of a wavefront: every lane ends with the same value, in the same order of additions for
// every call
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, WAVE));
  return v;
}

// WAVE_ROWS == 0: a row per lane (short rows).  WAVE_ROWS == 1: a row per wavefront — lanes stride over the row's entries, partial
// sums meet in wave_sum (long rows: a dense Jacobian gives rows of nvar or nequ entries).  Accumulation in double; TOut = float is
// the form the refinement loop uses (g goes straight into the inner handle's right-hand side).
// grid: (chunks of rows, problems — strided: clamped to the launch limit); problems at or beyond `batch` are not touched.
template <int WAVE_ROWS, class TOut>
__global__ void __launch_bounds__(NT) kkt_residual_kernel(DevKktRows R, const double* __restrict__ vals, const double* __restrict__ rhs,
                                                          const double* __restrict__ d, TOut* __restrict__ g, double* __restrict__ norms,
                                                          long long norm_stride, const int* __restrict__ success, int batch) {
  __shared__ double wmax[NW];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int r0 = blockIdx.x * R.rows_per_chunk, r1 = min(R.N, r0 + R.rows_per_chunk);
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    TOut* gb = g + (long long)b * R.N;
    // where the workgroup leaves its maximum: the norm itself, or its slot of the partial maxima
    double* nout = !norms ? nullptr : R.nchunk > 1 ? R.partial + (long long)b * R.nchunk + blockIdx.x : norms + (long long)b * norm_stride;
    if (success && !success[b]) {   // (uniform over the workgroup)
      for (int i = r0 + threadIdx.x; i < r1; i += NT) gb[i] = (TOut)0;
      if (nout && threadIdx.x == 0) *nout = -1.0;
      continue;
    }
    const double* vb = vals + (long long)b * R.nnz;
    const double* rb = rhs + (long long)b * R.N;
    const double* db = d + (long long)b * R.N;
    double mx = 0.0;
    if (WAVE_ROWS) {
      for (int i = r0 + wave; i < r1; i += NW) {
        const int q0 = R.ptr[i], q1 = R.ptr[i + 1];
        double s = 0.0;
        for (int q = q0 + lane; q < q1; q += WAVE) s = fma(vb[R.slot[q]], db[R.col[q]], s);
        s = rb[i] + wave_sum(s);
        if (lane == 0) gb[i] = (TOut)s;
        mx = fmax(mx, fabs(s));   // (NaN: fmax keeps the other operand; a NaN residual shows in g)
      }
    } else {
      for (int i = r0 + threadIdx.x; i < r1; i += NT) {
        const int q0 = R.ptr[i], q1 = R.ptr[i + 1];
        double s = 0.0;
        for (int q = q0; q < q1; q++) s = fma(vb[R.slot[q]], db[R.col[q]], s);
        s += rb[i];
        gb[i] = (TOut)s;
        mx = fmax(mx, fabs(s));
      }
    }
    if (nout) {   // (uniform)
      mx = wave_max(mx);
      if (lane == 0) wmax[wave] = mx;
      __syncthreads();
      if (threadIdx.x == 0) {
        double m = wmax[0];
#pragma unroll
        for (int w = 1; w < NW; w++) m = fmax(m, wmax[w]);
        *nout = m;
      }
      __syncthreads();   // wmax is written again for the workgroup's next problem
    }
  }
}

// norms[b] = the maximum of the problem's partial maxima (a chunked launch); a thread per problem
__global__ void __launch_bounds__(NT) kkt_norm_reduce_kernel(const double* __restrict__ partial, int nchunk, double* __restrict__ norms, long long norm_stride,
                                                             int batch) {
  const int b = blockIdx.x * NT + threadIdx.x;
  if (b >= batch) return;
  double m = partial[(long long)b * nchunk];
  for (int c = 1; c < nchunk; c++) m = fmax(m, partial[(long long)b * nchunk + c]);
  norms[(long long)b * norm_stride] = m;
}

// 16-byte loads (two doubles) and 8-byte stores (two floats) over the body, a scalar tail; vec == 0 (the launcher found src or dst
// not aligned for that): element by element.  (double)x -> float rounds to nearest: beyond FLT_MAX it gives inf.
__global__ void __launch_bounds__(NT) refine_demote_kernel(const double* __restrict__ src, float* __restrict__ dst, long long n, int vec) {
  const long long stride = (long long)gridDim.x * NT, t = (long long)blockIdx.x * NT + threadIdx.x;
  if (!vec) {
    for (long long i = t; i < n; i += stride) dst[i] = (float)src[i];
    return;
  }
  const long long pairs = n / 2;
  const double2* s2 = reinterpret_cast<const double2*>(src);
  float2* d2 = reinterpret_cast<float2*>(dst);
  for (long long i = t; i < pairs; i += stride) {
    const double2 v = s2[i];
    d2[i] = make_float2((float)v.x, (float)v.y);
  }
  if ((n & 1) && t == 0) dst[n - 1] = (float)src[n - 1];
}

// grid: (chunks of a row, problems)
__global__ void __launch_bounds__(NT) refine_update_kernel(double* __restrict__ d, const float* __restrict__ e, const int* __restrict__ success, int N,
                                                           int batch, int assign) {
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    if (success && !success[b]) continue;
    double* db = d + (long long)b * N;
    const float* eb = e + (long long)b * N;
    for (int i = blockIdx.x * NT + threadIdx.x; i < N; i += gridDim.x * NT) db[i] = assign ? (double)eb[i] : db[i] + (double)eb[i];
  }
}

__global__ void __launch_bounds__(NT) refine_widen_rho_kernel(const float* __restrict__ rho32, const float* __restrict__ rho_old32, double* __restrict__ rho,
                                                              double* __restrict__ rho_old, const float* __restrict__ vals32, double* __restrict__ vals,
                                                              long long nnz, int nvar, const int* __restrict__ nfact, int batch) {
  for (int b = blockIdx.y; b < batch; b += gridDim.y) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { rho[b] = (double)rho32[b]; rho_old[b] = (double)rho_old32[b]; }
    if (nfact[b] <= 1) continue;
    const long long t0 = (long long)b * nnz + (nnz - nvar);
    for (int i = blockIdx.x * NT + threadIdx.x; i < nvar; i += gridDim.x * NT) vals[t0 + i] = (double)vals32[t0 + i];
  }
}

template <class TOut>
hipError_t launch_kkt_residual_t(const DevKktRows& R, const double* vals, const double* rhs, const double* d, TOut* g, double* norms, int64_t norm_stride,
                                 const int32_t* success, int batch, hipStream_t stream) {
  if (batch <= 0 || R.N <= 0) return hipSuccess;
  if (R.nchunk < 1 || (long long)R.nchunk * R.rows_per_chunk < R.N || (R.nchunk > 1 && !R.partial)) return hipErrorInvalidValue;
  const dim3 grid(R.nchunk, std::min(batch, 65535)), block(NT);
  if (R.wave_rows)
    hipLaunchKernelGGL((kkt_residual_kernel<1, TOut>), grid, block, 0, stream, R, vals, rhs, d, g, norms, (long long)norm_stride, success, batch);
  else
    hipLaunchKernelGGL((kkt_residual_kernel<0, TOut>), grid, block, 0, stream, R, vals, rhs, d, g, norms, (long long)norm_stride, success, batch);
  if (norms && R.nchunk > 1)
    hipLaunchKernelGGL(kkt_norm_reduce_kernel, dim3((batch + NT - 1) / NT), block, 0, stream, R.partial, R.nchunk, norms, (long long)norm_stride, batch);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_kkt_residual(const DevKktRows& R, const double* vals, const double* rhs, const double* d, double* g, double* norms, int64_t norm_stride,
                               const int32_t* success, int batch, hipStream_t stream) {
  return launch_kkt_residual_t(R, vals, rhs, d, g, norms, norm_stride, success, batch, stream);
}
hipError_t launch_kkt_residual(const DevKktRows& R, const double* vals, const double* rhs, const double* d, float* g, double* norms, int64_t norm_stride,
                               const int32_t* success, int batch, hipStream_t stream) {
  return launch_kkt_residual_t(R, vals, rhs, d, g, norms, norm_stride, success, batch, stream);
}

hipError_t launch_refine_demote(const double* src, float* dst, int64_t n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>(((n + 1) / 2 + NT - 1) / NT, 8192);
  const int vec = reinterpret_cast<uintptr_t>(src) % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 8 == 0;
  hipLaunchKernelGGL(refine_demote_kernel, dim3((unsigned)blocks), dim3(NT), 0, stream, src, dst, (long long)n, vec);
  return hipGetLastError();
}

hipError_t launch_refine_update(double* d, const float* e, const int32_t* success, int N, int batch, int assign, hipStream_t stream) {
  if (N <= 0 || batch <= 0) return hipSuccess;
  hipLaunchKernelGGL(refine_update_kernel, dim3(std::min(64, (N + NT - 1) / NT), std::min(batch, 65535)), dim3(NT), 0, stream, d, e, success, N, batch, assign);
  return hipGetLastError();
}

hipError_t launch_refine_widen_rho(const float* rho32, const float* rho_old32, double* rho, double* rho_old, const float* vals32, double* vals, int64_t nnz,
                                   int nvar, const int32_t* nfact, int batch, hipStream_t stream) {
  if (batch <= 0) return hipSuccess;
  hipLaunchKernelGGL(refine_widen_rho_kernel, dim3(std::max(1, std::min(64, (nvar + NT - 1) / NT)), std::min(batch, 65535)), dim3(NT), 0, stream, rho32,
                     rho_old32, rho, rho_old, vals32, vals, (long long)nnz, nvar, nfact, batch);
  return hipGetLastError();
}

}  // namespace cnl
