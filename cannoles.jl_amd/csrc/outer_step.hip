// outer_step.hip — the per-problem bookkeeping of the batched outer / inner loop, as four device kernels.
//
// cannoles.jl_amd/device_loop.py runs B problems of one model family through the reference's `solve!`
// (/root/reference/src/CaNNOLeS.jl:612-864) in lockstep, every quantity a [B, ...] array in HBM and every branch a mask.  Until
// round 4 the masks and the masked state updates were ~150 framework launches per global step (2.3 ms of launch chains for
// batches of any size); here they are four kernels working IN PLACE on the state the caller describes with `cnl_outer_state`:
//   cnl_outer_begin_dev        start of an outer iteration (:612-626), who needs a Newton system, the step's branch flags
//   cnl_outer_newton_done_dev  takes the Newton system's results (:633-652: d, rho_old, counters, `broken`), extrapolation eps (:659)
//   cnl_outer_trial_done_dev   acceptance test at the trial point and the state update (:733-763), end-of-inner-loop tests (:765-800)
//   cnl_outer_end_dev          statuses, outer-iteration counters (:800-857)
//   cnl_outer_compact_dev      (no counterpart in the reference) the active problems to the front of every per-problem array, so that
//                              the next steps run on them alone
//   cnl_outer_hess_mask_dev    which problems refresh their residual Hessian under :Newton_vanishing (hessian_approx.jl:55-60)
// begin, trial_done, ls_test and end also come as `_ex` entry points with a control block `cnl_outer_ctl` (the keywords of `solve!` that
// the plain calls leave at "off": always_accept_extrapolation, max_iter, max_eval with its per-problem evaluation counter).  One kernel
// template serves both: it takes the block by value, and the plain entry points pass the block with everything off.
// The arithmetic of every test is the reference's, in its operation order; minimum / maximum propagate NaN as the framework's
// (and Julia's) do.  The model callbacks, the line search and the rare small-residual branch stay with the caller.
//
// Element types.  Every kernel is a template on the state structure: cnl_outer_state (T = double, cnl_outer_*_dev) and
// cnl_outer_state_f32 (T = float, cnl_outer_*_f32_dev), what `solve!` is for T = Float64 and T = Float32.
//   * Element-wise arithmetic is in T, every literal rounded to T first, as the reference writes T(0.99), T(1e3), T(100.0)
//     (src/CaNNOLeS.jl:532, 623, 659, 664, 736, 750, 760-761, 1106): T(0.99) * combined, never the double product rounded afterwards.
//   * T(1e60) (:638, 647) is Inf32 for T = Float32: `huge<float>()` is infinity, so a finite fx never breaks a Float32 problem.
//   * Reductions — block_sum and the sequential sums over p, which feed |Ft|^2, the three merit sums, g'dx, the non-finite count,
//     sum |lam| and sum c^2 — accumulate in double from the exactly widened T operands (a product of two floats is exact in double)
//     and are rounded to T once.  For T = double that is the plain sum, as before.  For T = float the reference's dot products have
//     no prescribed order, and a once-rounded double sum is within one rounding of any of them; it also makes the decisions
//     independent of the summation order, which the comparison with the framework form of the loop relies on.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/cannoles_hip.h"

// every product and sum rounded separately, as the scalar (and the framework's element-wise) code the decisions are compared with
#pragma clang fp contract(off)

namespace {

template <class ST> struct elem_of;
template <> struct elem_of<cnl_outer_state> { using type = double; };
template <> struct elem_of<cnl_outer_state_f32> { using type = float; };
template <class ST> using elem_t = typename elem_of<ST>::type;

template <class T> __device__ __forceinline__ T tmax(T a, T b) { return (a != a || b != b) ? T(NAN) : (a > b ? a : b); }
template <class T> __device__ __forceinline__ T tmin(T a, T b) { return (a != a || b != b) ? T(NAN) : (a < b ? a : b); }
__device__ __forceinline__ double tsqrt(double a) { return sqrt(a); }
__device__ __forceinline__ float tsqrt(float a) { return sqrtf(a); }
__device__ __forceinline__ double tabs(double a) { return fabs(a); }
__device__ __forceinline__ float tabs(float a) { return fabsf(a); }
// T(1e60), src/CaNNOLeS.jl:638, 647
template <class T> __device__ __forceinline__ T huge();
template <> __device__ __forceinline__ double huge<double>() { return 1e60; }
template <> __device__ __forceinline__ float huge<float>() { return INFINITY; }

// sum over the workgroup (256 threads), result in every thread; fixed order.  Always in double: the callers widen their terms
// and round the result to the element type once
__device__ double block_sum(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// the control block of a plain call: nothing accepted early, no limits, no evaluation counter
cnl_outer_ctl ctl_off() {
  cnl_outer_ctl c{};
  c.struct_size = (int32_t)sizeof(cnl_outer_ctl);
  c.max_iter = -1;
  c.max_eval = -1;
  return c;
}
__device__ __forceinline__ bool over_eval(const cnl_outer_ctl& C, long long b) { return C.neval && C.max_eval >= 0 && C.neval[b] > C.max_eval; }

template <class ST>
__global__ void __launch_bounds__(256) outer_begin_kernel(const ST S, const cnl_outer_ctl C) {
  using T = elem_t<ST>;
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= S.B) return;
  const bool act = S.status[b] == 0;
  const bool so = act && S.phase0[b];
  long long inner = S.inner[b];
  if (so) {  // start of an outer iteration, src/CaNNOLeS.jl:612-626
    const T nd = S.normdual[b], np_ = S.normprimal[b];
    const T comb = nd + np_;
    S.combined[b] = comb;
    S.delta[b] = tmax(tmin(S.delta_dec * S.delta[b], comb), S.dmin);
    inner = 0;
    S.inner[b] = 0;
    S.combined_hat[b] = T(INFINITY);
    S.ndh[b] = nd; S.nph[b] = np_;
    S.phase0[b] = 0;
  }
  // the iteration right behind a rejected extrapolation reuses d (:627); with always_accept_extrapolation it took the point, so d is due
  const bool need = act && (inner != 1 || C.always_accept_extrapolation);
  S.act[b] = act; S.need[b] = need; S.brk[b] = 0;
  if (act) atomicOr(S.flags + 0, 1);
  if (need) atomicOr(S.flags + 1, 1);
  if (act && inner == 0) atomicOr(S.flags + 2, 1);
  if (act && inner > 0) atomicOr(S.flags + 3, 1);
}

// one workgroup per problem
template <class ST>
__global__ void __launch_bounds__(256) outer_newton_done_kernel(const ST S, int did_newton) {
  using T = elem_t<ST>;
  __shared__ double sh[4];
  const long long b = blockIdx.x;
  const int t = threadIdx.x;
  bool act = S.act[b] != 0;
  if (did_newton) {
    const bool need = S.need[b] != 0;
    const T* dn = S.d_new + b * S.N;
    double bad = 0.0;
    for (long long k = t; k < S.N; k += 256) bad += isfinite(dn[k]) ? 0.0 : 1.0;
    bad = block_sum(bad, sh);
    if (need) {
      T* d = S.d + b * S.N;
      for (long long k = t; k < S.N; k += 256) d[k] = dn[k];
    }
    if (t == 0) {
      if (need) {
        S.rho_old[b] = S.ro_tmp[b];
        S.nfact[b] += S.nf_new[b];
        S.nlin[b] += 1;
      }
      // `broken` (:638-652): the inner loop is left at once, the end-of-iteration tests still run for the problem
      const bool brk = need && (S.rho_new[b] > S.rhomax || S.ok_new[b] == 0 || bad != 0.0 || S.fx[b] >= huge<T>());
      S.brk[b] = brk;
      if (brk) { act = false; S.act[b] = 0; }
    }
    __syncthreads();
    act = S.act[b] != 0;
  }
  // multipliers of the line search's merit function, lam - c / delta (:1066), for every problem (used where lsm)
  if (S.lam_ls) {
    const T dl = S.delta[b];
    for (long long k = t; k < S.P; k += 256) S.lam_ls[b * S.P + k] = S.p > 0 ? S.lam[b * S.P + k] - S.cx[b * S.P + k] / dl : S.lam[b * S.P + k];
  }
  if (t == 0) {
    const long long inner = S.inner[b];
    const bool ext = act && inner == 0, lsm = act && inner > 0;
    S.ext[b] = ext; S.lsm[b] = lsm;
    if (ext) {  // :659
      const T e = S.epsk[b];
      S.epsk[b] = tmax(tmin(T(1e3) * S.delta[b], 99 * e / 100), 9 * e / 10);
    }
  }
}

// the extrapolation's trial point (cnl_trial_point_dev wrote xt_e, rt_e, lamt_e for every problem) goes to the problems of `ext`
template <class ST>
__global__ void __launch_bounds__(256) outer_extrapolated_kernel(const ST S) {
  const long long b = blockIdx.x;
  if (!S.ext[b]) return;
  const int t = threadIdx.x;
  for (long long k = t; k < S.n; k += 256) S.xt[b * S.n + k] = S.xt_e[b * S.n + k];
  for (long long k = t; k < S.m; k += 256) S.rt[b * S.m + k] = S.rt_e[b * S.m + k];
  for (long long k = t; k < S.P; k += 256) S.lamt[b * S.P + k] = S.lamt_e[b * S.P + k];
}

template <class ST>
__global__ void __launch_bounds__(256) outer_trial_done_kernel(const ST S, const cnl_outer_ctl C) {
  using T = elem_t<ST>;
  __shared__ double sh[4];
  __shared__ int dec[4];
  const long long b = blockIdx.x;
  const int t = threadIdx.x;
  const bool act = S.act[b] != 0, brk = S.brk[b] != 0;
  const long long inner0 = S.inner[b];
  // f(xt) = |F(xt)|^2 / 2
  const T* Ft = S.Ft + b * S.m;
  double ssd = 0.0;
  for (long long k = t; k < S.m; k += 256) ssd += (double)Ft[k] * (double)Ft[k];
  const T ss = (T)block_sum(ssd, sh);
  if (t == 0) {
    T ndh = S.ndh[b], nph = S.nph[b], chat = S.combined_hat[b];
    if (act) { ndh = S.nrm_t[2 * b]; nph = S.nrm_t[2 * b + 1]; chat = ndh + nph; }   // optimality measures at the trial point, :722-732
    S.ndh[b] = ndh; S.nph[b] = nph; S.combined_hat[b] = chat;
    const T epsk = S.epsk[b];
    const bool good = chat <= T(0.99) * S.combined[b] + epsk;                        // :733
    const bool acc_state = act && (inner0 > 0 || C.always_accept_extrapolation || good);   // :735
    const bool acc_lam = act && good;
    if (C.neval && S.ext[b]) C.neval[b] += C.evals_per_point;   // the extrapolation's trial point was evaluated (the line search counts its own)
    if (acc_state) S.fx[b] = T(0.5) * ss;
    const T delta = S.delta[b];
    T delta_next = delta;
    if (S.p > 0) {                                                                   // :758-763
      const bool dr = act && inner0 > 0 && (ndh <= T(0.99) * S.normdual[b] + epsk / 2) && (nph > T(0.99) * S.normprimal[b] + epsk / 2);
      if (dr) delta_next = tmax(delta / 10, S.dmin);
    }
    const long long inner = inner0 + (act ? 1 : 0);
    S.inner[b] = inner;
    const bool tired = inner > S.max_inner || over_eval(C, b);
    const bool done_in = (act && (good || tired)) || brk;
    if (done_in) { S.normdual[b] = ndh; S.normprimal[b] = nph; }
    S.delta[b] = delta_next;
    const bool rej = act && !good;
    S.rej[b] = rej; S.done_in[b] = done_in; S.tired[b] = tired;
    dec[0] = acc_state; dec[1] = acc_lam; dec[2] = done_in;
    if (rej) atomicOr(S.flags + 4, 1);
  }
  __syncthreads();
  const bool acc_state = dec[0] != 0, acc_lam = dec[1] != 0, done_in = dec[2] != 0;
  if (acc_state) {
    for (long long k = t; k < S.n; k += 256) S.x[b * S.n + k] = S.xt[b * S.n + k];
    for (long long k = t; k < S.m; k += 256) { S.r[b * S.m + k] = S.rt[b * S.m + k]; S.Fx[b * S.m + k] = S.Ft[b * S.m + k]; }
    for (long long k = t; k < S.P; k += 256) S.cx[b * S.P + k] = S.ct[b * S.P + k];
    for (long long k = t; k < S.nnzjF; k += 256) S.Jv[b * S.nnzjF + k] = S.Jt[b * S.nnzjF + k];
    if (S.Jcv != S.Jct) for (long long k = t; k < S.nnzjc; k += 256) S.Jcv[b * S.nnzjc + k] = S.Jct[b * S.nnzjc + k];
  }
  if (acc_lam) for (long long k = t; k < S.P; k += 256) S.lam[b * S.P + k] = S.lamt[b * S.P + k];
  if (act) for (long long k = t; k < S.N; k += 256) S.rhs_cur[b * S.N + k] = S.rhs_t[b * S.N + k];
  __syncthreads();
  if (t == 0) {
    // end of the inner loop -> end of the outer iteration, :765-800
    double sld = 0.0, scd = 0.0;
    for (long long k = 0; k < S.p; k++) { sld += (double)tabs(S.lam[b * S.P + k]); const double c = S.cx[b * S.P + k]; scd += c * c; }
    const T sl = (T)sld, sc = (T)scd;
    const T ds = S.p > 0 ? tmax(sl / (T)S.p, S.smax) / S.smax : T(1);
    const bool first_order = tmax(S.normdual[b] / ds, S.normprimal[b]) <= S.epstol[b];
    const bool small_res = (2 * tsqrt(S.fx[b]) <= S.epsF[b]) && (tsqrt(sc) <= S.epsc[b]);
    S.small_res[b] = small_res;
    const bool chk = done_in && small_res && !first_order;
    S.chk[b] = chk;
    if (chk) atomicOr(S.flags + 5, 1);
  }
}

// ---- Armijo line search on the merit function phi(x) = |F|^2 / 2 - lam'c + eta |c|^2 / 2, src/CaNNOLeS.jl:1054-1112 ----------------
// The model callbacks (F, c at the trial points) are the caller's; these kernels do the rest of a round for every problem at once.
template <class ST, class T>
__device__ T merit(const ST& S, long long b, const T* F, const T* c, T eta, double* sh) {
  const int t = threadIdx.x;
  double sfd = 0.0, slcd = 0.0, sccd = 0.0;
  for (long long k = t; k < S.m; k += 256) sfd += (double)F[b * S.m + k] * (double)F[b * S.m + k];
  if (S.p > 0)
    for (long long k = t; k < S.p; k += 256) { const double cv = c[b * S.P + k]; slcd += (double)S.lam[b * S.P + k] * cv; sccd += cv * cv; }
  const T sf = (T)block_sum(sfd, sh);
  const T slc = (T)block_sum(slcd, sh);
  const T scc = (T)block_sum(sccd, sh);
  T phi = T(0.5) * sf;
  if (S.p > 0) { phi = phi - slc; phi = phi + eta * scc / 2; }
  return phi;
}

// Dphi = g'dx with g = Jx'F - Jc'(lam - c / delta) (the dual part cnl_residual_vectors_dev left in ls_g), eta, phi(x), alpha = 1,
// first trial point xl = x + dx
template <class ST>
__global__ void __launch_bounds__(256) outer_ls_begin_kernel(const ST S) {
  using T = elem_t<ST>;
  __shared__ double sh[4];
  const long long b = blockIdx.x;
  const int t = threadIdx.x;
  const T* g = S.ls_g + b * S.N;
  const T* dx = S.d + b * S.N;
  double dpd = 0.0;
  for (long long k = t; k < S.n; k += 256) dpd += (double)g[k] * (double)dx[k];
  const T dp = (T)block_sum(dpd, sh);
  T eta = S.eta[b];
  if (S.p > 0 && S.lsm[b]) eta = T(1) / S.delta[b];
  const T phix = merit<ST, T>(S, b, S.Fx, S.cx, eta, sh);
  if (t == 0) { S.Dphi[b] = dp; S.eta[b] = eta; S.phix[b] = phix; S.alpha[b] = T(1); }
  for (long long k = t; k < S.n; k += 256) S.xl[b * S.n + k] = S.x[b * S.n + k] + dx[k];
}

// Armijo test at (Fl, cl) = (F(xl), c(xl)); first != 0: the first test (every lsm problem), else a backtracking round's
template <class ST>
__global__ void __launch_bounds__(256) outer_ls_test_kernel(const ST S, int first, const cnl_outer_ctl C) {
  using T = elem_t<ST>;
  __shared__ double sh[4];
  const long long b = blockIdx.x;
  const bool cand = first ? S.lsm[b] != 0 : S.bt[b] != 0;
  if (!cand) { if (first && threadIdx.x == 0) S.bt[b] = 0; return; }
  const T phil = merit<ST, T>(S, b, S.Fl, S.cl, S.eta[b], sh);
  if (threadIdx.x == 0) {
    if (C.neval) C.neval[b] += C.evals_per_point;   // F and c at this candidate's xl
    const T alpha = S.alpha[b];
    bool bt = !(phil <= S.phix[b] + S.gammaA * alpha * S.Dphi[b]);
    if (!first) bt = bt && (alpha >= S.eps2);
    S.bt[b] = bt;
    if (bt) atomicOr(S.flags + 6, 1);
  }
}

// one backtracking step for the problems of bt: alpha / 4, xl = x + alpha dx (:1098-1105)
template <class ST>
__global__ void __launch_bounds__(256) outer_ls_step_kernel(const ST S) {
  using T = elem_t<ST>;
  const long long b = blockIdx.x;
  if (!S.bt[b]) return;
  const int t = threadIdx.x;
  const T alpha = S.alpha[b] / 4;
  const T* dx = S.d + b * S.N;
  for (long long k = t; k < S.n; k += 256) S.xl[b * S.n + k] = S.x[b * S.n + k] + alpha * dx[k];
  if (t == 0) { S.alpha[b] = alpha; S.nbk[b] += 1; }
}

// the accepted point of the line search becomes the trial point of the problems of lsm
template <class ST>
__global__ void __launch_bounds__(256) outer_ls_take_kernel(const ST S) {
  const long long b = blockIdx.x;
  if (!S.lsm[b]) return;
  const int t = threadIdx.x;
  for (long long k = t; k < S.n; k += 256) S.xt[b * S.n + k] = S.xl[b * S.n + k];
  for (long long k = t; k < S.m; k += 256) S.rt[b * S.m + k] = S.Fl[b * S.m + k];
  for (long long k = t; k < S.P; k += 256) S.lamt[b * S.P + k] = S.lam_ls[b * S.P + k];
}

template <class ST>
__global__ void __launch_bounds__(256) outer_end_kernel(const ST S, const cnl_outer_ctl C) {
  using T = elem_t<ST>;
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= S.B) return;
  const bool done_in = S.done_in[b] != 0;
  if (!done_in) return;
  double sld = 0.0;
  for (long long k = 0; k < S.p; k++) sld += (double)tabs(S.lam[b * S.P + k]);
  const T sl = (T)sld;
  const T ds = S.p > 0 ? tmax(sl / (T)S.p, S.smax) / S.smax : T(1);
  const bool first_order = tmax(S.normdual[b] / ds, S.normprimal[b]) <= S.epstol[b];
  const int32_t it = S.it[b] + 1;
  S.it[b] = it;
  // get_status (src/CaNNOLeS.jl:836-847) in the order of outer_loop.solve: 4 (max_eval) is the evaluation count alone, 6 (max_iter) the
  // outer-iteration count; an inner loop left at its iteration limit is `stalled` (:846) -> 5.  `tired` holds either cause of leaving
  // the inner loop, and the evaluation count is tested first, so 5 is reached by the iteration limit only
  const bool max_it = C.max_iter >= 0 && it > C.max_iter;
  S.status[b] = first_order ? 1 : (S.small_res[b] ? 2 : (S.brk[b] ? 3 : (over_eval(C, b) ? 4 : (max_it ? 6 : (S.tired[b] ? 5 : 0)))));
  S.phase0[b] = 1;
}

// :Newton_vanishing (hessian_approx.jl:55-60): the residual Hessian of a problem is refreshed only while dot(Fx, Fx) > 1e-8.  One
// workgroup per problem; the dot product by the file's reduction rule, then compared with the double literal
template <class ST>
__global__ void __launch_bounds__(256) outer_hess_mask_kernel(const ST S, const cnl_outer_ctl C) {
  using T = elem_t<ST>;
  __shared__ double sh[4];
  const long long b = blockIdx.x;
  const T* Fx = S.Fx + b * S.m;
  double ssd = 0.0;
  for (long long k = threadIdx.x; k < S.m; k += 256) ssd += (double)Fx[k] * (double)Fx[k];
  const T ss = (T)block_sum(ssd, sh);
  if (threadIdx.x == 0) C.hess_upd[b] = (double)ss > 1e-8;
}

// ---- compaction of the loop's state: the active problems become the first rows (cnl_outer_compact_dev) -----------------------------
// A problem that has finished (status != 0) is still a row of every [B, ...] array, and every kernel of a global step still runs over
// it.  With A = the number of active rows below Bc = S.B: the k-th finished row below A (ascending) and the k-th active row at or above
// A (ascending) change places, in every per-problem array — afterwards rows 0 .. A-1 are exactly the active problems and the caller
// goes on with B = A.  Both sets have the same size, sources and destinations are disjoint, so the swap is in place and all B rows
// stay a permutation of what they were (the caller's d_orig row says which problem a row holds).
// Two launches back to back on the stream: one workgroup counts, scans and writes the pair list; the swap kernel reads the pair count
// from the device (the host never learns it) and strides over the pairs.
constexpr int COMPACT_MAX_ARRAYS = 112, COMPACT_MAX_EXTRA = 24, CP_THREADS = 1024, CP_MAX_GRID = 2048;
struct CompactArrays {
  int n, nsmall;                       // arrays; the first nsmall have rows of at most 16 bytes (one thread moves a row)
  unsigned bytes[COMPACT_MAX_ARRAYS];  // row bytes
  char* base[COMPACT_MAX_ARRAYS];
};

// counts = {A, Bc after the call}; work = [pair count, -, (finished row, active row) x pairs]
__global__ void __launch_bounds__(CP_THREADS) compact_pair_kernel(const int32_t* __restrict__ status, int Bc, long long min_finished,
                                                                  int32_t* __restrict__ counts, int32_t* __restrict__ work) {
  __shared__ int wsum[CP_THREADS / 64];
  __shared__ int below_A;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int per = (Bc + CP_THREADS - 1) / CP_THREADS;
  const int b0 = min((long long)t * per, (long long)Bc), b1 = min((long long)b0 + per, (long long)Bc);
  int c = 0;
  for (int b = b0; b < b1; b++) c += status[b] == 0;
  int v = c;   // inclusive scan over the wavefront, then over the wavefronts' totals
  for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
  int before = v - c, A = 0;   // active rows below b0; active rows in all
  for (int w = 0; w < CP_THREADS / 64; w++) { if (w < wave) before += wsum[w]; A += wsum[w]; }
  if ((long long)Bc - A < min_finished) {   // not worth a pass yet: nothing moves
    if (t == 0) { counts[0] = A; counts[1] = Bc; work[0] = 0; }
    return;
  }
  // (min_finished >= 1: A < Bc, so one thread's range holds row A)
  if (b0 <= A && A < b1) {
    int q = before;
    for (int b = b0; b < A; b++) q += status[b] == 0;
    below_A = q;
  }
  __syncthreads();
  const int act_below = below_A;   // active rows below A; A - act_below finished rows there = active rows at or above A = pairs
  if (t == 0) { counts[0] = A; counts[1] = A; work[0] = A - act_below; }
  int q = before;
  for (int b = b0; b < b1; b++) {
    const bool active = status[b] == 0;
    if (!active && b < A) work[2 + 2 * (b - q)] = b;                  // finished rows before b: b - q, all of them below A
    if (active && b >= A) work[2 + 2 * (q - act_below) + 1] = b;
    q += active;
  }
}

template <class V>
__device__ __forceinline__ void swap_vectors(char* a, char* b, unsigned nv, unsigned first, unsigned step) {
  V* pa = reinterpret_cast<V*>(a);
  V* pb = reinterpret_cast<V*>(b);
  for (unsigned i = first; i < nv; i += step) { const V x = pa[i], y = pb[i]; pa[i] = y; pb[i] = x; }
}
// Two rows of nb bytes change places, moved by threads first, first + step, ...: the widest vector both addresses allow (rows are
// element-aligned only: 16-byte vectors where both rows happen to start on 16 bytes, else 8, 4, 2, 1), the rest of a row that is
// no multiple of that width in ever narrower pieces.
__device__ __forceinline__ void swap_rows(char* a, char* b, unsigned nb, unsigned first, unsigned step) {
  const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u;
  const unsigned w = m == 0 ? 16 : (m & 7) == 0 ? 8 : (m & 3) == 0 ? 4 : (m & 1) == 0 ? 2 : 1;
  const unsigned nv = nb / w;
  switch (w) {
    case 16: swap_vectors<uint4>(a, b, nv, first, step); break;
    case 8: swap_vectors<uint2>(a, b, nv, first, step); break;
    case 4: swap_vectors<uint32_t>(a, b, nv, first, step); break;
    case 2: swap_vectors<uint16_t>(a, b, nv, first, step); break;
    default: swap_vectors<uint8_t>(a, b, nv, first, step); break;
  }
  unsigned off = nv * w, rem = nb - off;   // rem < w; off is a multiple of w: each piece below is aligned to its own width
  if (rem && first == 0) {
    if (rem & 8) { swap_vectors<uint2>(a + off, b + off, 1, 0, 1); off += 8; }
    if (rem & 4) { swap_vectors<uint32_t>(a + off, b + off, 1, 0, 1); off += 4; }
    if (rem & 2) { swap_vectors<uint16_t>(a + off, b + off, 1, 0, 1); off += 2; }
    if (rem & 1) swap_vectors<uint8_t>(a + off, b + off, 1, 0, 1);
  }
}

// one workgroup per pair (grid-stride: the grid is sized for the worst case the host knows, min(Bc / 2, CP_MAX_GRID), and a workgroup
// without a pair leaves at once): the short rows one thread each, the long rows by the whole workgroup
__global__ void __launch_bounds__(256) compact_swap_kernel(const CompactArrays L, const int32_t* __restrict__ work) {
  const int npairs = work[0], t = threadIdx.x;
  for (int k = blockIdx.x; k < npairs; k += gridDim.x) {
    const long long ra = work[2 + 2 * k], rb = work[2 + 2 * k + 1];
    for (int i = t; i < L.nsmall; i += 256) swap_rows(L.base[i] + ra * L.bytes[i], L.base[i] + rb * L.bytes[i], L.bytes[i], 0, 1);
    for (int i = L.nsmall; i < L.n; i++) swap_rows(L.base[i] + ra * L.bytes[i], L.base[i] + rb * L.bytes[i], L.bytes[i], t, 256);
  }
}

// every array of the state the kernels dereference must be there (the header promises CNL_ERR_ARG for a missing array, not an
// asynchronous fault).  The members are named one by one (walking the struct as an array of pointers would read a scalar
// member added later as a pointer).  The multiplier / constraint arrays (lam, cx, ct, lamt, lamt_e, cl, lam_ls) have rows of
// P = max(p, 1) entries and are walked over P: they are required also when p == 0 (include/cannoles_hip.h says so); only the
// constraint-Jacobian value arrays Jcv / Jct may be NULL when nnzjc == 0.  The line-search entries also need theirs (check_ls).
template <class ST>
int check(const ST* st) {
  if (!st || st->B <= 0) return CNL_ERR_ARG;
#define CNL_NEED(m) if (!st->m) return CNL_ERR_ARG;
  CNL_NEED(status) CNL_NEED(it) CNL_NEED(flags) CNL_NEED(nf_new) CNL_NEED(ok_new)
  CNL_NEED(inner) CNL_NEED(nfact) CNL_NEED(nlin)
  CNL_NEED(phase0) CNL_NEED(act) CNL_NEED(need) CNL_NEED(brk) CNL_NEED(ext) CNL_NEED(lsm) CNL_NEED(rej) CNL_NEED(chk) CNL_NEED(done_in) CNL_NEED(tired) CNL_NEED(small_res)
  CNL_NEED(normdual) CNL_NEED(normprimal) CNL_NEED(combined) CNL_NEED(combined_hat) CNL_NEED(delta) CNL_NEED(ndh) CNL_NEED(nph) CNL_NEED(fx)
  CNL_NEED(epsk) CNL_NEED(epstol) CNL_NEED(epsF) CNL_NEED(epsc) CNL_NEED(rho_old)
  CNL_NEED(d) CNL_NEED(d_new) CNL_NEED(ro_tmp) CNL_NEED(rho_new)
  CNL_NEED(x) CNL_NEED(r) CNL_NEED(Fx) CNL_NEED(Jv) CNL_NEED(rhs_cur)
  CNL_NEED(xt) CNL_NEED(rt) CNL_NEED(Ft) CNL_NEED(Jt) CNL_NEED(rhs_t) CNL_NEED(nrm_t)
  CNL_NEED(xt_e) CNL_NEED(rt_e)
  CNL_NEED(cx) CNL_NEED(lam) CNL_NEED(ct) CNL_NEED(lamt) CNL_NEED(lamt_e)
  if (st->nnzjc > 0) { CNL_NEED(Jcv) CNL_NEED(Jct) }
  return 0;
}
template <class ST>
int check_ls(const ST* st) {
  if (check(st)) return CNL_ERR_ARG;
  CNL_NEED(ls_g) CNL_NEED(xl) CNL_NEED(Fl) CNL_NEED(cl) CNL_NEED(lam_ls) CNL_NEED(alpha) CNL_NEED(Dphi) CNL_NEED(phix) CNL_NEED(eta) CNL_NEED(nbk) CNL_NEED(bt)
#undef CNL_NEED
  return 0;
}
int done() { return hipGetLastError() == hipSuccess ? CNL_OK : CNL_ERR_HIP; }
// a caller's control block: its size as this library knows it, the evaluation counter, evals_per_point 1 (residual) or 2 (residual and
// constraints); NULL stands for the plain call
int check_ctl(const cnl_outer_ctl* ctl) {
  if (!ctl) return 0;
  if (ctl->struct_size != (int32_t)sizeof(cnl_outer_ctl) || !ctl->neval || (ctl->evals_per_point != 1 && ctl->evals_per_point != 2)) return CNL_ERR_ARG;
  return 0;
}

// the entry points, for either state structure; ctl == nullptr: the plain call
template <class ST> int begin_impl(const ST* st, const cnl_outer_ctl* ctl, void* stream) {
  if (check(st) || check_ctl(ctl)) return CNL_ERR_ARG;
  if (hipMemsetAsync(st->flags, 0, 8 * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return CNL_ERR_HIP;
  hipLaunchKernelGGL(outer_begin_kernel<ST>, dim3((unsigned)((st->B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *st, ctl ? *ctl : ctl_off());
  return done();
}
template <class ST> int newton_done_impl(const ST* st, int did_newton, void* stream) {
  if (check(st)) return CNL_ERR_ARG;
  hipLaunchKernelGGL(outer_newton_done_kernel<ST>, dim3((unsigned)st->B), dim3(256), 0, (hipStream_t)stream, *st, did_newton);
  return done();
}
template <class ST> int extrapolated_impl(const ST* st, void* stream) {
  if (check(st)) return CNL_ERR_ARG;
  hipLaunchKernelGGL(outer_extrapolated_kernel<ST>, dim3((unsigned)st->B), dim3(256), 0, (hipStream_t)stream, *st);
  return done();
}
template <class ST> int trial_done_impl(const ST* st, const cnl_outer_ctl* ctl, void* stream) {
  if (check(st) || check_ctl(ctl)) return CNL_ERR_ARG;
  hipLaunchKernelGGL(outer_trial_done_kernel<ST>, dim3((unsigned)st->B), dim3(256), 0, (hipStream_t)stream, *st, ctl ? *ctl : ctl_off());
  return done();
}
template <class ST> int ls_begin_impl(const ST* st, void* stream) {
  if (check_ls(st)) return CNL_ERR_ARG;
  hipLaunchKernelGGL(outer_ls_begin_kernel<ST>, dim3((unsigned)st->B), dim3(256), 0, (hipStream_t)stream, *st);
  return done();
}
template <class ST> int ls_test_impl(const ST* st, int first, const cnl_outer_ctl* ctl, void* stream) {
  if (check_ls(st) || check_ctl(ctl)) return CNL_ERR_ARG;
  if (hipMemsetAsync(st->flags + 6, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return CNL_ERR_HIP;
  hipLaunchKernelGGL(outer_ls_test_kernel<ST>, dim3((unsigned)st->B), dim3(256), 0, (hipStream_t)stream, *st, first, ctl ? *ctl : ctl_off());
  return done();
}
template <class ST> int ls_step_impl(const ST* st, void* stream) {
  if (check_ls(st)) return CNL_ERR_ARG;
  hipLaunchKernelGGL(outer_ls_step_kernel<ST>, dim3((unsigned)st->B), dim3(256), 0, (hipStream_t)stream, *st);
  return done();
}
template <class ST> int ls_take_impl(const ST* st, void* stream) {
  if (check_ls(st)) return CNL_ERR_ARG;
  hipLaunchKernelGGL(outer_ls_take_kernel<ST>, dim3((unsigned)st->B), dim3(256), 0, (hipStream_t)stream, *st);
  return done();
}
template <class ST> int end_impl(const ST* st, const cnl_outer_ctl* ctl, void* stream) {
  if (check(st) || check_ctl(ctl)) return CNL_ERR_ARG;
  hipLaunchKernelGGL(outer_end_kernel<ST>, dim3((unsigned)((st->B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *st, ctl ? *ctl : ctl_off());
  return done();
}
// (the mask kernel has no plain form: its output array is a member of the control block)
template <class ST> int hess_mask_impl(const ST* st, const cnl_outer_ctl* ctl, void* stream) {
  if (check(st) || !ctl || check_ctl(ctl) || !ctl->hess_upd) return CNL_ERR_ARG;
  hipLaunchKernelGGL(outer_hess_mask_kernel<ST>, dim3((unsigned)st->B), dim3(256), 0, (hipStream_t)stream, *st, *ctl);
  return done();
}

// cnl_outer_compact_dev: the per-problem arrays of the state (every element, counter and mask member; `flags` is global), the caller's
// extra arrays and d_orig, each once (the loop hands one array over as Jcv and Jct: a row that is swapped twice is back where it was),
// the short rows in front
template <class ST> int compact_impl(const ST* st, int64_t nextra, void* const* extra, const int64_t* extra_row_bytes, int64_t min_finished,
                                     int32_t* d_orig, int32_t* d_counts, int32_t* d_work, void* stream) {
  using T = elem_t<ST>;
  if (check(st) || st->B > 0x7fffffffLL) return CNL_ERR_ARG;
  if (nextra < 0 || nextra > COMPACT_MAX_EXTRA || (nextra > 0 && (!extra || !extra_row_bytes))) return CNL_ERR_ARG;
  if (min_finished < 1 || !d_orig || !d_counts || !d_work) return CNL_ERR_ARG;
  for (int64_t i = 0; i < nextra; i++)
    if (!extra[i] || extra_row_bytes[i] <= 0 || extra_row_bytes[i] > 0x7fffffffLL) return CNL_ERR_ARG;
  struct Entry { char* p; int64_t bytes; };
  Entry all[COMPACT_MAX_ARRAYS];
  int n = 0;
  auto add = [&](const void* p, int64_t bytes) {
    if (!p || bytes <= 0) return;   // (an optional array that is not there, a row of no entries)
    for (int i = 0; i < n; i++) if (all[i].p == p) return;
    all[n++] = Entry{static_cast<char*>(const_cast<void*>(p)), bytes};
  };
  const int64_t e = sizeof(T);
#define CNL_ROW(m, bytes) add(st->m, (bytes));
  CNL_ROW(status, 4) CNL_ROW(it, 4) CNL_ROW(nf_new, 4) CNL_ROW(ok_new, 4)
  CNL_ROW(inner, 8) CNL_ROW(nfact, 8) CNL_ROW(nlin, 8) CNL_ROW(nbk, 8)
  CNL_ROW(phase0, 1) CNL_ROW(act, 1) CNL_ROW(need, 1) CNL_ROW(brk, 1) CNL_ROW(ext, 1) CNL_ROW(lsm, 1) CNL_ROW(rej, 1) CNL_ROW(chk, 1)
  CNL_ROW(done_in, 1) CNL_ROW(tired, 1) CNL_ROW(small_res, 1) CNL_ROW(bt, 1)
  CNL_ROW(normdual, e) CNL_ROW(normprimal, e) CNL_ROW(combined, e) CNL_ROW(combined_hat, e) CNL_ROW(delta, e) CNL_ROW(ndh, e) CNL_ROW(nph, e)
  CNL_ROW(fx, e) CNL_ROW(epsk, e) CNL_ROW(epstol, e) CNL_ROW(epsF, e) CNL_ROW(epsc, e) CNL_ROW(rho_old, e) CNL_ROW(ro_tmp, e) CNL_ROW(rho_new, e)
  CNL_ROW(alpha, e) CNL_ROW(Dphi, e) CNL_ROW(phix, e) CNL_ROW(eta, e) CNL_ROW(nrm_t, 2 * e)
  CNL_ROW(d, e * st->N) CNL_ROW(d_new, e * st->N) CNL_ROW(rhs_cur, e * st->N) CNL_ROW(rhs_t, e * st->N) CNL_ROW(ls_g, e * st->N)
  CNL_ROW(x, e * st->n) CNL_ROW(xt, e * st->n) CNL_ROW(xt_e, e * st->n) CNL_ROW(xl, e * st->n)
  CNL_ROW(r, e * st->m) CNL_ROW(Fx, e * st->m) CNL_ROW(rt, e * st->m) CNL_ROW(Ft, e * st->m) CNL_ROW(rt_e, e * st->m) CNL_ROW(Fl, e * st->m)
  CNL_ROW(cx, e * st->P) CNL_ROW(lam, e * st->P) CNL_ROW(ct, e * st->P) CNL_ROW(lamt, e * st->P) CNL_ROW(lamt_e, e * st->P) CNL_ROW(cl, e * st->P)
  CNL_ROW(lam_ls, e * st->P)
  CNL_ROW(Jv, e * st->nnzjF) CNL_ROW(Jt, e * st->nnzjF) CNL_ROW(Jcv, e * st->nnzjc) CNL_ROW(Jct, e * st->nnzjc)
#undef CNL_ROW
  static_assert(COMPACT_MAX_ARRAYS >= 72 + COMPACT_MAX_EXTRA + 1, "room for every member, the extra arrays and d_orig");
  for (int64_t i = 0; i < nextra; i++) add(extra[i], extra_row_bytes[i]);
  add(d_orig, 4);
  for (int i = 0; i < n; i++) if (all[i].bytes > 0x7fffffffLL) return CNL_ERR_ARG;
  CompactArrays L{};
  for (int pass = 0; pass < 2; pass++) {
    for (int i = 0; i < n; i++)
      if ((all[i].bytes <= 16) == (pass == 0)) { L.base[L.n] = all[i].p; L.bytes[L.n] = (unsigned)all[i].bytes; L.n++; }
    if (pass == 0) L.nsmall = L.n;
  }
  hipLaunchKernelGGL(compact_pair_kernel, dim3(1), dim3(CP_THREADS), 0, (hipStream_t)stream, st->status, (int)st->B, (long long)min_finished,
                     d_counts, d_work);
  if (hipGetLastError() != hipSuccess) return CNL_ERR_HIP;
  const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>(st->B / 2, 1), CP_MAX_GRID);
  hipLaunchKernelGGL(compact_swap_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, L, d_work);
  return done();
}

}  // namespace

extern "C" {

int cnl_outer_begin_dev(const cnl_outer_state* st, void* stream) { return begin_impl(st, nullptr, stream); }
int cnl_outer_newton_done_dev(const cnl_outer_state* st, int did_newton, void* stream) { return newton_done_impl(st, did_newton, stream); }
int cnl_outer_extrapolated_dev(const cnl_outer_state* st, void* stream) { return extrapolated_impl(st, stream); }
int cnl_outer_trial_done_dev(const cnl_outer_state* st, void* stream) { return trial_done_impl(st, nullptr, stream); }
int cnl_outer_ls_begin_dev(const cnl_outer_state* st, void* stream) { return ls_begin_impl(st, stream); }
int cnl_outer_ls_test_dev(const cnl_outer_state* st, int first, void* stream) { return ls_test_impl(st, first, nullptr, stream); }
int cnl_outer_ls_step_dev(const cnl_outer_state* st, void* stream) { return ls_step_impl(st, stream); }
int cnl_outer_ls_take_dev(const cnl_outer_state* st, void* stream) { return ls_take_impl(st, stream); }
int cnl_outer_end_dev(const cnl_outer_state* st, void* stream) { return end_impl(st, nullptr, stream); }
int cnl_outer_begin_ex_dev(const cnl_outer_state* st, const cnl_outer_ctl* ctl, void* stream) { return begin_impl(st, ctl, stream); }
int cnl_outer_trial_done_ex_dev(const cnl_outer_state* st, const cnl_outer_ctl* ctl, void* stream) { return trial_done_impl(st, ctl, stream); }
int cnl_outer_ls_test_ex_dev(const cnl_outer_state* st, int first, const cnl_outer_ctl* ctl, void* stream) { return ls_test_impl(st, first, ctl, stream); }
int cnl_outer_end_ex_dev(const cnl_outer_state* st, const cnl_outer_ctl* ctl, void* stream) { return end_impl(st, ctl, stream); }
int cnl_outer_hess_mask_dev(const cnl_outer_state* st, const cnl_outer_ctl* ctl, void* stream) { return hess_mask_impl(st, ctl, stream); }

int cnl_outer_compact_dev(const cnl_outer_state* st, int64_t nextra, void* const* d_extra, const int64_t* extra_row_bytes, int64_t min_finished,
                          int32_t* d_orig, int32_t* d_counts, int32_t* d_work, void* stream) {
  return compact_impl(st, nextra, d_extra, extra_row_bytes, min_finished, d_orig, d_counts, d_work, stream);
}

int cnl_outer_begin_f32_dev(const cnl_outer_state_f32* st, void* stream) { return begin_impl(st, nullptr, stream); }
int cnl_outer_newton_done_f32_dev(const cnl_outer_state_f32* st, int did_newton, void* stream) { return newton_done_impl(st, did_newton, stream); }
int cnl_outer_extrapolated_f32_dev(const cnl_outer_state_f32* st, void* stream) { return extrapolated_impl(st, stream); }
int cnl_outer_trial_done_f32_dev(const cnl_outer_state_f32* st, void* stream) { return trial_done_impl(st, nullptr, stream); }
int cnl_outer_ls_begin_f32_dev(const cnl_outer_state_f32* st, void* stream) { return ls_begin_impl(st, stream); }
int cnl_outer_ls_test_f32_dev(const cnl_outer_state_f32* st, int first, void* stream) { return ls_test_impl(st, first, nullptr, stream); }
int cnl_outer_ls_step_f32_dev(const cnl_outer_state_f32* st, void* stream) { return ls_step_impl(st, stream); }
int cnl_outer_ls_take_f32_dev(const cnl_outer_state_f32* st, void* stream) { return ls_take_impl(st, stream); }
int cnl_outer_end_f32_dev(const cnl_outer_state_f32* st, void* stream) { return end_impl(st, nullptr, stream); }
int cnl_outer_begin_ex_f32_dev(const cnl_outer_state_f32* st, const cnl_outer_ctl* ctl, void* stream) { return begin_impl(st, ctl, stream); }
int cnl_outer_trial_done_ex_f32_dev(const cnl_outer_state_f32* st, const cnl_outer_ctl* ctl, void* stream) { return trial_done_impl(st, ctl, stream); }
int cnl_outer_ls_test_ex_f32_dev(const cnl_outer_state_f32* st, int first, const cnl_outer_ctl* ctl, void* stream) { return ls_test_impl(st, first, ctl, stream); }
int cnl_outer_end_ex_f32_dev(const cnl_outer_state_f32* st, const cnl_outer_ctl* ctl, void* stream) { return end_impl(st, ctl, stream); }
int cnl_outer_hess_mask_f32_dev(const cnl_outer_state_f32* st, const cnl_outer_ctl* ctl, void* stream) { return hess_mask_impl(st, ctl, stream); }

int cnl_outer_compact_f32_dev(const cnl_outer_state_f32* st, int64_t nextra, void* const* d_extra, const int64_t* extra_row_bytes,
                              int64_t min_finished, int32_t* d_orig, int32_t* d_counts, int32_t* d_work, void* stream) {
  return compact_impl(st, nextra, d_extra, extra_row_bytes, min_finished, d_orig, d_counts, d_work, stream);
}

}  // extern "C"
