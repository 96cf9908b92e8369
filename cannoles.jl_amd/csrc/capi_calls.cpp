// capi_calls.cpp — the numeric entry points of the C ABI (include/cannoles_hip.h): rows f1 / f2 / f4 and the trial point on device
// pointers, factorize / solve / newton_system on device pointers and on host pointers (staging, the chunked pipeline, the
// host-driven rho ladder).  One implementation per call for both element types: every extern "C" entry point checks the handle's
// element type and forwards to a template on it; the routes only Float64 handles can take are Float64 functions.
#include "handle.h"

#include <climits>

namespace {

const char* const kHostLayout = "host-pointer calls take the reference's problem-major arrays: this handle was created with batch_layout = "
                                "CNL_LAYOUT_INTERLEAVED (device-pointer entry points only)";

// the handle's pinned host block (results of host-pointer calls), at least `bytes` long
int ensure_pinned(cnl_handle* h, size_t bytes) {
  if (h->pin && h->pin_bytes >= bytes) return CNL_OK;
  if (h->pin) (void)hipHostFree(h->pin);
  h->pin = nullptr;
  HIPCHK(hipHostMalloc(&h->pin, bytes, hipHostMallocDefault));
  h->pin_bytes = bytes;
  return CNL_OK;
}

// rows [b][N] of the problems with ok(b) from the device to the host, one copy per maximal run of them (one in the common case): the
// reference leaves d untouched where the factorisation failed (src/CaNNOLeS.jl:1049)
template <class T, class Ok>
hipError_t copy_rows_where(Ok ok, T* dst, const T* d_src, size_t B, size_t N, hipStream_t stream) {
  size_t b0 = 0;
  while (b0 < B) {
    while (b0 < B && !ok(b0)) b0++;
    size_t b1 = b0;
    while (b1 < B && ok(b1)) b1++;
    if (b1 > b0)
      if (hipError_t e = hipMemcpyAsync(dst + b0 * N, d_src + b0 * N, (b1 - b0) * N * sizeof(T), hipMemcpyDeviceToHost, stream)) return e;
    b0 = b1;
  }
  return hipSuccess;
}

// Staging of the host-pointer calls, in the handle's element type T: device copies of vals, rhs and d, and the per-problem results
// of a call in ONE block, [rho | rho_old | nfact | success] (+ 64 spare bytes) and [npos | nzero]: a small host-pointer call brings
// each group back with one copy (every copy of a few bytes is a transfer of its own on the stream: ~8 us).
// Results<T>: where a call leaves its per-problem results; Stage<T>: the typed view of the handle's staging blocks.
template <class T>
struct Results {
  T *rho_old = nullptr, *rho = nullptr;
  int32_t *nfact = nullptr, *success = nullptr;
  int64_t *npos = nullptr, *nzero = nullptr;
};
template <class T>
struct Stage : Results<T> {
  T *vals, *rhs, *d;
};
template <class T>
Stage<T> stage(const cnl_handle* h) {   // (of the whole handle: not inside a SubBatch view, which changes h->batch)
  const size_t B = (size_t)h->batch;
  Stage<T> s;
  s.vals = static_cast<T*>(h->d_vals); s.rhs = static_cast<T*>(h->d_rhs); s.d = static_cast<T*>(h->d_d);
  s.rho = static_cast<T*>(h->d_res); s.rho_old = s.rho + B;
  s.nfact = reinterpret_cast<int32_t*>(s.rho_old + B); s.success = s.nfact + B;
  s.npos = h->d_npos; s.nzero = h->d_npos + B;
  return s;
}
int ensure_staging(cnl_handle* h) {
  if (h->d_vals) return CNL_OK;
  const cnl_plan& P = *h->plan;
  const size_t B = (size_t)h->batch;
  void* vals;
  char* res;
  int rc;
  if ((rc = dalloc_elems(h, &vals, B * P.nnz))) return rc;
  if ((rc = dalloc_elems(h, &h->d_rhs, B * P.N))) return rc;
  if ((rc = dalloc_elems(h, &h->d_d, B * P.N))) return rc;
  if ((rc = dalloc(h, &res, B * (2 * h->esz() + 2 * sizeof(int32_t)) + 64))) return rc;
  if ((rc = dalloc(h, &h->d_npos, B * 2))) return rc;
  h->d_res = res;
  h->d_vals = vals;   // (last: the staging exists)
  return CNL_OK;
}

// One call on typed device pointers: the only place that fills cnl::LaunchArgs from them (its element arrays are untyped, in the
// handle's element type).  d_vals is written by newton_system alone.  params: np values (exact in double; a Float32 kernel narrows
// them back).
template <class T>
int run_typed(cnl_handle* h, int mode, const T* params, int np, const Results<T>& r, const T* d_vals, const T* d_rhs, T* d_d, hipStream_t stream,
              RunOpts o = {}) {
  cnl::LaunchArgs a{};
  a.mode = mode;
  a.rho_old = r.rho_old; a.rho = r.rho; a.nfact = r.nfact; a.success = r.success; a.npos = r.npos; a.nzero = r.nzero;
  for (int k = 0; k < np; k++) a.params[k] = params[k];
  return run(h, a, const_cast<T*>(d_vals), d_rhs, d_d, stream, o);
}
// where newton_system on the staged arrays leaves its results, for the problems from b0 on (no inertia counts: try_to_factorize's)
template <class T>
Results<T> newton_results(const Stage<T>& s, size_t b0 = 0) {
  Results<T> r;
  r.rho_old = s.rho_old + b0; r.rho = s.rho + b0; r.nfact = s.nfact + b0; r.success = s.success + b0;
  return r;
}

// Inside a host-pointer newton_system that goes on after a factorisation (its ladders): the factor on the device is that of the
// staged `vals` from here on, so a solve of the same call reads them.  (run() sets last_vals for try_to_factorize alone.)
void factor_is_of(cnl_handle* h, const void* d_vals) { h->last_vals = d_vals; }
// After a completed call, the only writer: this handle now holds a factor of `vals` (device array of its element type).  ok: the
// success flags of a host-pointer call, which cnl_solve consults; nullptr after a device-pointer call, whose flags the host has not seen
void holds_factor(cnl_handle* h, const void* d_vals, const int32_t* ok = nullptr) {
  h->factorized = true;
  h->factor_batch = h->batch;
  h->last_vals = d_vals;
  if (ok) h->last_ok.assign(ok, ok + h->batch);
  else h->last_ok.clear();
}

// ---- rows f1 / f2 / f4 and the trial point on device pointers: one implementation per row for both element types (the launchers
//      of kernels.h are overloaded on float / double); the entry points (extern "C" below) check the handle's element type first ----
template <class T>
int prepare_impl(cnl_handle* h, int64_t nnzhF, int64_t nnzhc, int64_t nnzjF, int64_t nnzjc, const T* d_hF, const T* d_hc, const T* d_Jx,
                 const T* d_Jcx, const T* d_delta, T* d_vals, void* stream) {
  const cnl::DevJt& J = h->djt;
  if (nnzhF < 0 || nnzhc < 0 || nnzjF < 0 || nnzjc < 0 || nnzhF + nnzhc + nnzjF + nnzjc + J.nequ + J.ncon + J.nvar != J.nnz)
    return fail(CNL_ERR_DIM, "segment sizes do not add up to nnz (7-segment layout of src/CaNNOLeS.jl:256-315)");
  if (J.ncon > 0 && (!d_hc || !d_Jcx || !d_delta)) return fail(CNL_ERR_ARG, "hc / Jcx / delta are required when ncon > 0");
  if (J.ncon == 0 && (nnzhc != 0 || nnzjc != 0)) return fail(CNL_ERR_DIM, "constraint segments must be empty when ncon == 0");
  HIPCHK(hipSetDevice(h->device));
  hipError_t e = cnl::launch_prepare((int)nnzhF, (int)nnzhc, (int)nnzjF, (int)nnzjc, J.nvar, J.nequ, J.ncon, d_hF, d_hc, d_Jx, d_Jcx,
                                     d_delta, d_vals, (int)h->batch, h->layout & 1, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CNL_ERR_HIP, std::string("prepare_newton_system: ") + hipGetErrorString(e));
  return CNL_OK;
}

template <class T>
int cgls_impl(cnl_handle* h, const cnl::JacSrcT<T>& S, const T* d_r, T* d_lambda, T* d_Jxtr, T atol, T rtol, int64_t itmax,
              int ones_if_zero, int32_t* d_iters, void* stream) {
  if (h->djt.ncon == 0) return CNL_OK;  // nothing to estimate
  if (!d_lambda) return fail(CNL_ERR_ARG, "null lambda");
  // the instance (tuning cgls_wide): the ncon-vectors in LDS, at most 1024 constraints; or in the workspace, any number
  const int mode = h->plan->opt.cgls_wide;
  const bool wide = mode == 2 || (mode == 1 && h->djt.ncon > 1024);
  if (!wide && h->djt.ncon > 1024)
    return fail(CNL_ERR_DIM, "cnl_cgls_multipliers_dev supports at most 1024 constraints (tuning cgls_wide = 1: the instance without that limit)");
  HIPCHK(hipSetDevice(h->device));
  T* ws = static_cast<T*>(h->cgls_ws);   // (the entry points have checked T against the handle's element type)
  if (!ws) {
    // (the created batch: cnl_set_active_batch may widen the handle again; which instance runs is fixed per handle)
    int rc = dalloc(h, &ws, (size_t)h->full_batch * (2 * (size_t)h->djt.nvar + (wide ? 3 * (size_t)h->djt.ncon : 0)));
    if (rc) return rc;
    h->cgls_ws = ws;
  }
  if (itmax <= 0) itmax = (int64_t)h->djt.nvar + h->djt.ncon;  // Krylov.jl's default: m + n
  if (itmax > INT_MAX) itmax = INT_MAX;  // the kernel counts in int: "no limit" (typemax(Int64)) must not wrap to a negative count
  hipError_t e = cnl::launch_cgls(h->djt, S, d_r, d_lambda, d_Jxtr, ws, d_iters, atol, rtol, (int)itmax, ones_if_zero,
                                  wide, (int)h->batch, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CNL_ERR_HIP, std::string("cgls: ") + hipGetErrorString(e));
  return CNL_OK;
}

// the Jacobian values from the model's arrays (problem-major [batch][nnz(J_F)], [batch][nnz(J_c)]: what cnl_prepare_newton_system_dev takes)
template <class T>
int jac_source(cnl_handle* h, int64_t nnzjF, int64_t nnzjc, const T* d_Jx, const T* d_Jcx, cnl::JacSrcT<T>* S) {
  if (!h->jac_segments) return fail(CNL_ERR_STATE, "the J_F / J_c entries of this pattern are not one run of slots each (7-segment layout of src/CaNNOLeS.jl:256-315)");
  if (nnzjF != h->jf_n || nnzjc != h->jc_n) return fail(CNL_ERR_DIM, "nnzjF / nnzjc do not match the pattern's Jacobian entries");
  if (h->jf_n == 0) return fail(CNL_ERR_STATE, "the pattern has no J_F entries");
  if (!d_Jx || (h->jc_n > 0 && !d_Jcx)) return fail(CNL_ERR_ARG, "null Jacobian values");
  // (no J_c entries: the J_c source aliases the J_F one, nothing is read through it but the gather kernel's loads of absent entries)
  if (h->jc_n > 0) *S = cnl::JacSrcT<T>{d_Jx - h->jf_lo, h->jf_n, d_Jcx - h->jc_lo, h->jc_n, (int)h->jf_lo, (int)h->jc_lo};
  else *S = cnl::JacSrcT<T>{d_Jx - h->jf_lo, h->jf_n, d_Jx - h->jf_lo, h->jf_n, (int)h->jf_lo, (int)h->jf_lo};
  return CNL_OK;
}

template <class T>
int residual_vectors_impl(cnl_handle* h, const cnl::JacSrcT<T>& S, const T* d_r, const T* d_lambda, const T* d_Fx,
                          const T* d_cx, T* d_rhs, T* d_norms, void* stream) {
  if (!d_r || !d_Fx || !d_rhs || !d_norms) return fail(CNL_ERR_ARG, "null argument");
  if (h->djt.ncon > 0 && (!d_lambda || !d_cx)) return fail(CNL_ERR_ARG, "lambda / c are required when ncon > 0");
  HIPCHK(hipSetDevice(h->device));
  hipError_t e = cnl::launch_residual_vectors(h->djt, S, d_r, d_lambda, d_Fx, d_cx, d_rhs, d_norms, (int)h->batch, (hipStream_t)stream);
  if (e != hipSuccess) return fail(CNL_ERR_HIP, std::string("residual_vectors: ") + hipGetErrorString(e));
  return CNL_OK;
}

template <class T>
int trial_point_impl(cnl_handle* h, const T* d_x, const T* d_r, const T* d_lambda, const T* d_d, T max_dlambda, T* d_xt, T* d_rt,
                     T* d_lambdat, T* d_dlambda, void* stream) {
  if (h->djt.ncon > 0 && (!d_lambda || !d_lambdat || !d_dlambda)) return fail(CNL_ERR_ARG, "lambda vectors are required when ncon > 0");
  HIPCHK(hipSetDevice(h->device));
  hipError_t e = cnl::launch_trial_point(h->djt, d_x, d_r, d_lambda, d_d, max_dlambda, d_xt, d_rt, d_lambdat, d_dlambda, (int)h->batch,
                                         (hipStream_t)stream);
  if (e != hipSuccess) return fail(CNL_ERR_HIP, std::string("trial_point: ") + hipGetErrorString(e));
  return CNL_OK;
}

// ---- factorize / solve / newton_system on device pointers ----
template <class T>
int factorize_dev_impl(cnl_handle* h, const T* d_vals, T eig_tol, int32_t* d_success, void* stream) {
  HIPCHK(hipSetDevice(h->device));
  Results<T> r;
  r.success = d_success;
  const int rc = run_typed<T>(h, cnl::MODE_FACTOR, &eig_tol, 1, r, d_vals, nullptr, nullptr, (hipStream_t)stream);
  if (rc == CNL_OK) holds_factor(h, d_vals);
  return rc;
}

// (band handles: the solve factorises the values of the last factorisation again, rho slots as the ladder left them — capi_run.cpp, run_band)
template <class T>
int solve_dev_impl(cnl_handle* h, const T* d_rhs, T* d_d, void* stream) {
  if (!h->factorized) return fail(CNL_ERR_STATE, "cnl_solve before cnl_factorize");
  if (h->factor_batch < h->batch)
    return fail(CNL_ERR_STATE, "cnl_solve_dev on " + std::to_string(h->batch) + " problems behind a factorisation of " + std::to_string(h->factor_batch) +
                                   " (cnl_set_active_batch widened the handle in between)");
  HIPCHK(hipSetDevice(h->device));
  return run_typed<T>(h, cnl::MODE_SOLVE, nullptr, 0, Results<T>(), nullptr, d_rhs, d_d, (hipStream_t)stream);
}

template <class T>
int newton_system_dev_impl(cnl_handle* h, T* d_vals, const T* d_rhs, T* d_d, T* d_rho_old, T* d_rho, int32_t* d_nfact, int32_t* d_success,
                           const T params[9], void* stream) {
  HIPCHK(hipSetDevice(h->device));
  Results<T> r;
  r.rho_old = d_rho_old; r.rho = d_rho; r.nfact = d_nfact; r.success = d_success;
  const int rc = run_typed(h, cnl::MODE_NEWTON, params, 9, r, d_vals, d_rhs, d_d, (hipStream_t)stream);
  if (rc == CNL_OK) holds_factor(h, d_vals);
  return rc;
}

// ---- the same on host pointers (what the Julia glue ccalls): the reference's problem-major arrays through the handle's staging ----
const char* const kSolveAfterFailure = "cnl_solve after a factorisation that failed (success = 0): there is no factor to solve with "
                                       "(the reference calls solve_ldl! only after a successful try_to_factorize, src/CaNNOLeS.jl:1049)";

template <class T>
int factorize_impl(cnl_handle* h, const T* vals, T eig_tol, int32_t* success, int64_t* npos, int64_t* nzero) {
  if (h->layout) return fail(CNL_ERR_STATE, kHostLayout);
  HIPCHK(hipSetDevice(h->device));
  if (int rc = ensure_staging(h)) return rc;
  const Stage<T> s = stage<T>(h);
  const size_t B = (size_t)h->batch;
  HIPCHK(hipMemcpyAsync(s.vals, vals, B * h->plan->nnz * sizeof(T), hipMemcpyHostToDevice, h->stream));
  Results<T> r;
  r.success = s.success; r.npos = s.npos; r.nzero = s.nzero;
  if (int rc = run_typed<T>(h, cnl::MODE_FACTOR, &eig_tol, 1, r, s.vals, nullptr, nullptr, h->stream)) return rc;
  // results through the handle's pinned block: asynchronous copies (a copy into pageable memory blocks, one after the other),
  // the inertia counts with one copy (npos | nzero are one block on the device), a single synchronisation
  const size_t o_su = 0, o_np = (B * 4 + 7) & ~(size_t)7, total = o_np + B * 16;
  if (int rc = ensure_pinned(h, total)) return rc;
  char* pb = static_cast<char*>(h->pin);
  HIPCHK(hipMemcpyAsync(pb + o_su, s.success, B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (npos || nzero) HIPCHK(hipMemcpyAsync(pb + o_np, s.npos, B * 16, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  std::memcpy(success, pb + o_su, B * sizeof(int32_t));
  if (npos) std::memcpy(npos, pb + o_np, B * sizeof(int64_t));
  if (nzero) std::memcpy(nzero, pb + o_np + B * 8, B * sizeof(int64_t));
  holds_factor(h, s.vals, success);
  return CNL_OK;
}

template <class T>
int solve_impl(cnl_handle* h, const T* rhs, T* d) {
  if (h->layout) return fail(CNL_ERR_STATE, kHostLayout);
  if (!h->factorized) return fail(CNL_ERR_STATE, "cnl_solve before cnl_factorize");
  const size_t B = (size_t)h->batch, N = (size_t)h->plan->N;
  const bool known = h->last_ok.size() == B;
  if (known && B == 1 && !h->last_ok[0]) return fail(CNL_ERR_STATE, kSolveAfterFailure);
  HIPCHK(hipSetDevice(h->device));
  if (int rc = ensure_staging(h)) return rc;
  const Stage<T> s = stage<T>(h);
  HIPCHK(hipMemcpyAsync(s.rhs, rhs, B * N * sizeof(T), hipMemcpyHostToDevice, h->stream));
  if (int rc = run_typed<T>(h, cnl::MODE_SOLVE, nullptr, 0, Results<T>(), nullptr, s.rhs, s.d, h->stream)) return rc;
  // rows of the problems that hold a factor (all of them after a device-pointer factorisation); the others stay as the caller passed them
  HIPCHK(copy_rows_where([&](size_t b) { return !known || h->last_ok[b]; }, d, s.d, B, N, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return CNL_OK;
}

// newton_system, the pieces every route shares, for problems [b0, b0 + nb) of the call (host arrays: the whole batch's).
// Up: vals, rhs and rho_old (nullptr: zeros) into the staging arrays.
template <class T>
hipError_t upload_inputs(const cnl_handle* h, const Stage<T>& s, size_t b0, size_t nb, const T* vals, const T* rhs, const T* rho_old, hipStream_t st) {
  const size_t nnz = (size_t)h->plan->nnz, N = (size_t)h->plan->N;
  hipError_t e = hipMemcpyAsync(s.vals + b0 * nnz, vals + b0 * nnz, nb * nnz * sizeof(T), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(s.rhs + b0 * N, rhs + b0 * N, nb * N * sizeof(T), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = rho_old ? hipMemcpyAsync(s.rho_old + b0, rho_old + b0, nb * sizeof(T), hipMemcpyHostToDevice, st)
                                   : hipMemsetAsync(s.rho_old + b0, 0, nb * sizeof(T), st);
  return e;
}
// Down, once the caller's `success` holds the flags: the rows of d where the factorisation succeeded — the reference leaves d untouched
// when it fails (src/CaNNOLeS.jl:1049) — and the rho tail of vals (it mutates get_vals(LDLT)[end-nvar+1:end], src/CaNNOLeS.jl:1031,1038)
template <class T>
hipError_t download_solution(const cnl_handle* h, const Stage<T>& s, size_t b0, size_t nb, T* vals, T* d, const int32_t* success, hipStream_t st) {
  const size_t nnz = (size_t)h->plan->nnz, N = (size_t)h->plan->N, nvar = (size_t)h->plan->nvar;
  hipError_t e = copy_rows_where([&](size_t q) { return success[b0 + q] != 0; }, d + b0 * N, s.d + b0 * N, nb, N, st);
  if (e == hipSuccess && nvar > 0)
    e = hipMemcpy2DAsync(vals + b0 * nnz + (nnz - nvar), nnz * sizeof(T), s.vals + b0 * nnz + (nnz - nvar), nnz * sizeof(T), nvar * sizeof(T), nb,
                         hipMemcpyDeviceToHost, st);
  return e;
}
// ... and rho, rho_old, nfact
template <class T>
hipError_t download_rho(const Stage<T>& s, size_t b0, size_t nb, T* rho, T* rho_old_out, int32_t* nfact, hipStream_t st) {
  hipError_t e = hipMemcpyAsync(rho + b0, s.rho + b0, nb * sizeof(T), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(rho_old_out + b0, s.rho_old + b0, nb * sizeof(T), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(nfact + b0, s.nfact + b0, nb * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  return e;
}

// The plain route of newton_system: the whole batch up, one call of run() (the rho ladder on the device), the results down.
// cnl_newton_system_f32 is this; cnl_newton_system comes here after deciding against its Float64-only routes (below).
template <class T>
int newton_system_impl(cnl_handle* h, T* vals, const T* rhs, T* d, const T* rho_old, const T params[9], T* rho, T* rho_old_out, int32_t* nfact,
                       int32_t* success) {
  const Stage<T> s = stage<T>(h);
  const size_t B = (size_t)h->batch;
  HIPCHK(upload_inputs(h, s, 0, B, vals, rhs, rho_old, h->stream));
  if (int rc = run_typed(h, cnl::MODE_NEWTON, params, 9, newton_results(s), s.vals, s.rhs, s.d, h->stream)) return rc;
  HIPCHK(hipMemcpyAsync(success, s.success, B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(download_solution(h, s, 0, B, vals, d, success, h->stream));
  HIPCHK(download_rho(s, 0, B, rho, rho_old_out, nfact, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  holds_factor(h, s.vals, success);
  return CNL_OK;
}

// ---- the routes of cnl_newton_system only Float64 handles take ----
// try_to_factorize of the staged vals / solve_ldl! of the staged rhs, as the host-driven ladders enqueue them
int factorize_staged_vals(cnl_handle* h, const Stage<double>& s, const double params[9]) {
  Results<double> r;
  r.success = s.success; r.npos = s.npos; r.nzero = s.nzero;
  return run_typed<double>(h, cnl::MODE_FACTOR, params, 9, r, s.vals, nullptr, nullptr, h->stream);
}
int solve_staged_rhs(cnl_handle* h, const Stage<double>& s, const double params[9]) {
  return run_typed<double>(h, cnl::MODE_SOLVE, params, 9, Results<double>(), nullptr, s.rhs, s.d, h->stream);
}

bool host_ladder_serves(const cnl_handle* h, bool any_device_ladder);   // (below, with newton_small_pinned)

// The rho ladder of src/CaNNOLeS.jl:1023-1047 driven from the host for the problems whose first (staged) factorisation failed:
// every rung is a staged try_to_factorize of the batch and a read-back of the success flags; the solve follows (cnl_newton_system).
// up: pinned staging of 12 bytes per problem; su_pin: pinned, batch ints.  On return rho / rho_old_out / nfact / success hold the
// reference's results and the device holds the factors and the solution of everything that succeeded.
// tail_redone: a dataflow wait of the remainder handle gave up in the first attempt — its redo launch has been through the whole
// device ladder for those problems, and the ladder here must leave them alone.
int host_ladder_run(cnl_handle* h, const double params[9], const double* rho_old, double* rho, double* rho_old_out, int32_t* nfact,
                    int32_t* success, char* up, int32_t* su_pin, bool tail_redone = false) {
  const cnl_plan& P = *h->plan;
  const Stage<double> s = stage<double>(h);
  const size_t B = (size_t)h->batch;
  int rc;
  const double rho0 = params[5], rhomax = params[6], rhomin = params[7], kdec = params[2], kinc = params[3], klarge = params[4];
  if (!h->d_act && (rc = dalloc(h, &h->d_act, B))) return rc;
  double* up_rho = reinterpret_cast<double*>(up);
  int32_t* up_act = reinterpret_cast<int32_t*>(up + B * 8);
  std::vector<char> act(B, 0);
  std::vector<double> ro_in(B);
  // split handles: only the chain part [0, split_staged) ran the first attempt alone; the single-stream part has been through the
  // whole device ladder already (a problem that exhausted it there must not climb again: nfact would count twice)
  const size_t first_only = (h->split_staged > 0 && (size_t)h->split_staged < B && !h->split_halves && (!h->tail || tail_redone)) ? (size_t)h->split_staged : B;
  bool any_act = false;
  for (size_t b = 0; b < B; b++) {
    ro_in[b] = rho_old ? rho_old[b] : 0.0;
    if (!success[b] && b < first_only) { act[b] = 1; any_act = true; rho[b] = ro_in[b] == 0.0 ? rho0 : std::max(rhomin, kdec * ro_in[b]); }
  }
  while (any_act) {
    for (size_t b = 0; b < B; b++) { up_rho[b] = rho[b]; up_act[b] = act[b]; }
    HIPCHK(hipMemcpyAsync(s.rho, up_rho, B * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_act, up_act, B * 4, hipMemcpyHostToDevice, h->stream));
    hipError_t e = cnl::launch_fill_rho(s.vals, P.nnz, (int)P.nvar, s.rho, h->d_act, (int)B, h->stream);
    if (e != hipSuccess) return fail(CNL_ERR_HIP, std::string("fill_rho: ") + hipGetErrorString(e));
    if ((rc = factorize_staged_vals(h, s, params))) return rc;
    HIPCHK(hipMemcpyAsync(su_pin, s.success, B * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    any_act = false;
    for (size_t b = 0; b < B; b++) {
      if (!act[b]) continue;
      nfact[b]++;
      if (su_pin[b]) { success[b] = 1; act[b] = 0; continue; }
      rho[b] = ro_in[b] == 0.0 ? klarge * rho[b] : kinc * rho[b];
      if (rho[b] > rhomax) act[b] = 0;   // the ladder ran out: rho keeps the value beyond rhomax, the slots the last one tried
      else any_act = true;
    }
  }
  for (size_t b = 0; b < first_only; b++)
    if (rho[b] != 0.0 && rho[b] <= rhomax) rho_old_out[b] = rho[b];   // (rho != 0: the problem entered the ladder)
  // solve_ldl! for everything that holds a valid factor now (the problems of the first attempt are solved again: same factor);
  // the rungs were try_to_factorize calls on s.vals, also where the first attempt was a newton_system the caller gave other arrays
  factor_is_of(h, s.vals);
  return solve_staged_rhs(h, s, params);
}

// Large host-pointer batches, chunk by chunk: the call is bound by the host link (1.1 MB per system go up, 0.25 MB come back),
// which is full duplex — while chunk c + 1 goes up (calling thread, alternating between two streams) chunk c is computed and the
// results of chunk c - 1 come down (a helper thread of the call, third stream).  Copies between pageable host memory and the
// device block their host thread, hence the second thread; the compute of a chunk hides behind the upload of the next.
int newton_system_pipelined(cnl_handle* h, double* vals, const double* rhs, double* d, const double* rho_old, const double params[9],
                     double* rho, double* rho_old_out, int32_t* nfact, int32_t* success, size_t chunk) {
  const cnl_plan& P = *h->plan;
  const Stage<double> s = stage<double>(h);
  const size_t B = (size_t)h->batch;
  const size_t nchunks = (B + chunk - 1) / chunk;
  for (hipStream_t& st : h->pipe_stream) if (!st) HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  while (h->pipe_ev.size() < nchunks) {
    hipEvent_t e;
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    h->pipe_ev.push_back(e);
  }
  // staged handles: the chunks run the first attempt only; the problems that failed it go through the host-driven ladder on the
  // whole (now device-resident) batch behind the last chunk (see newton_staged_ladder), whatever device ladder the handle has
  const bool host_ladder = host_ladder_serves(h, true);
  std::mutex mu;        // posted[], abort_, and the handle view (SubBatch mutates the handle: one enqueue at a time)
  std::condition_variable cv;
  std::vector<char> posted(nchunks, 0);
  bool abort_ = false;
  int wrc = CNL_OK;
  std::string wmsg;
  const int device = h->device;
  std::thread down([&]() {
    (void)hipSetDevice(device);
    hipStream_t st = h->pipe_stream[cnl_handle::kPipeUp];
    auto chk = [&](hipError_t e, const char* what) {
      if (e != hipSuccess && wrc == CNL_OK) { wrc = CNL_ERR_HIP; wmsg = std::string(what) + ": " + hipGetErrorString(e); }
      return e == hipSuccess;
    };
    for (size_t c = 0; c < nchunks; c++) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return posted[c] || abort_; });
        if (!posted[c]) return;
      }
      const size_t b0 = c * chunk, nb = std::min(chunk, B - b0);
      if (!chk(hipEventSynchronize(h->pipe_ev[c]), "hipEventSynchronize")) continue;
      if (!chk(hipMemcpyAsync(success + b0, s.success + b0, nb * sizeof(int32_t), hipMemcpyDeviceToHost, st), "copy success")) continue;
      if (!chk(hipStreamSynchronize(st), "hipStreamSynchronize")) continue;
      chk(download_solution(h, s, b0, nb, vals, d, success, st), "copy d / rho slots");
      chk(download_rho(s, b0, nb, rho, rho_old_out, nfact, st), "copy rho / rho_old / nfact");
      chk(hipStreamSynchronize(st), "hipStreamSynchronize");
    }
  });
  // two uploaders (the calling thread and a helper) take alternate chunks, each on a stream of its own: a copy out of pageable
  // memory keeps a host thread busy (the runtime pins or stages the pages), and one thread alone does not fill the link
  constexpr int NU = cnl_handle::kPipeUp;
  int urc[NU];
  for (int& r_ : urc) r_ = CNL_OK;
  std::string umsg[NU];
  auto uploader = [&](int u) {
    if (u) (void)hipSetDevice(device);
    hipStream_t st = h->pipe_stream[u];
    for (size_t c = (size_t)u; c < nchunks; c += NU) {
      {
        std::lock_guard<std::mutex> lk(mu);
        if (abort_) return;
      }
      const size_t b0 = c * chunk, nb = std::min(chunk, B - b0);
      const hipError_t e = upload_inputs(h, s, b0, nb, vals, rhs, rho_old, st);
      int r = CNL_OK;
      std::string m;
      if (e != hipSuccess) { r = CNL_ERR_HIP; m = std::string("upload: ") + hipGetErrorString(e); }
      std::lock_guard<std::mutex> lk(mu);
      if (r == CNL_OK) {
        SubBatch view(h, (int64_t)b0, (int64_t)nb);
        r = run_typed(h, cnl::MODE_NEWTON, params, 9, newton_results(s, b0), s.vals + b0 * P.nnz, s.rhs + b0 * P.N, s.d + b0 * P.N, st,
                      RunOpts{host_ladder, false});
        if (r) m = g_err;
        if (r == CNL_OK && hipEventRecord(h->pipe_ev[c], st) != hipSuccess) { r = CNL_ERR_HIP; m = "hipEventRecord failed"; }
      }
      if (r != CNL_OK) { urc[u] = r; umsg[u] = m; abort_ = true; cv.notify_all(); return; }
      posted[c] = 1;
      cv.notify_all();
    }
  };
  h->tail_fresh = false;   // the chunks factorise every problem in THIS handle's storage (views), the remainder's handle is not used
  {
    TimingOff untimed(h);   // (a chunked call is not timed: cnl_newton_system comes here on an untimed handle only)
    std::vector<std::thread> ups;
    for (int u = 1; u < NU; u++) ups.emplace_back(uploader, u);
    uploader(0);
    for (std::thread& th : ups) th.join();
  }
  down.join();
  for (int u = 0; u < NU; u++) (void)hipStreamSynchronize(h->pipe_stream[u]);
  for (int u = 0; u < NU; u++) if (urc[u] != CNL_OK) return fail(urc[u], umsg[u]);
  if (wrc != CNL_OK) return fail(wrc, "download: " + wmsg);
  factor_is_of(h, s.vals);   // (the chunks ran on views of the handle, which take their last_vals with them)
  if (host_ladder) {
    std::vector<char> failed(B, 0);
    bool any_failed = false;
    for (size_t b = 0; b < B; b++) { failed[b] = !success[b]; any_failed |= failed[b] != 0; }
    if (any_failed) {
      const size_t need = B * 16;
      if (int prc = ensure_pinned(h, need)) return prc;
      char* pb2 = static_cast<char*>(h->pin);
      int rc = host_ladder_run(h, params, rho_old, rho, rho_old_out, nfact, success, pb2, reinterpret_cast<int32_t*>(pb2 + B * 12));
      if (rc) return rc;
      for (size_t b = 0; b < B; b++) {
        if (!failed[b]) continue;
        if (success[b]) HIPCHK(hipMemcpyAsync(d + b * P.N, s.d + b * P.N, (size_t)P.N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (P.nvar > 0)
          HIPCHK(hipMemcpyAsync(vals + b * P.nnz + (P.nnz - P.nvar), s.vals + b * P.nnz + (P.nnz - P.nvar), (size_t)P.nvar * sizeof(double),
                                hipMemcpyDeviceToHost, h->stream));
      }
      HIPCHK(hipStreamSynchronize(h->stream));
    }
  }
  holds_factor(h, s.vals, success);
  return CNL_OK;
}

// Dense backend, host-pointer call: the reference's own sequence — try_to_factorize, the rho ladder on the host, solve_ldl! — with
// the library's multi-kernel factorisation for EVERY rung.  The fused device call decides its ladder on the device, where a
// problem that failed is refactorised by ONE workgroup walking all tiles (dn_ladder: 7.8 ms per rung at cfg2's size against
// 0.35 ms for the launch sequence): 48 ms for a cfg2 system that climbs to nfact = 7.  Costs one more synchronisation when
// nothing fails.
int newton_dense_host_ladder(cnl_handle* h, double* vals, const double* rhs, double* d, const double* rho_old, const double params[9],
                             double* rho, double* rho_old_out, int32_t* nfact, int32_t* success) {
  const cnl_plan& P = *h->plan;
  const Stage<double> s = stage<double>(h);
  const size_t B = (size_t)h->batch;
  int rc;
  HIPCHK(upload_inputs(h, s, 0, B, vals, rhs, rho_old, h->stream));
  if ((rc = factorize_staged_vals(h, s, params))) return rc;
  HIPCHK(hipMemcpyAsync(success, s.success, B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  bool any_failed = false;
  for (size_t b = 0; b < B; b++) {
    rho[b] = 0.0; nfact[b] = 1; rho_old_out[b] = rho_old ? rho_old[b] : 0.0;
    any_failed |= !success[b];
  }
  if (any_failed) {
    const size_t need = B * 16;
    if (int prc = ensure_pinned(h, need)) return prc;
    char* pb2 = static_cast<char*>(h->pin);
    if ((rc = host_ladder_run(h, params, rho_old, rho, rho_old_out, nfact, success, pb2, reinterpret_cast<int32_t*>(pb2 + B * 12)))) return rc;
  } else {
    if ((rc = solve_staged_rhs(h, s, params))) return rc;
  }
  for (size_t b = 0; b < B; b++) {
    if (success[b]) HIPCHK(hipMemcpyAsync(d + b * P.N, s.d + b * P.N, (size_t)P.N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (nfact[b] > 1 && P.nvar > 0)
      HIPCHK(hipMemcpyAsync(vals + b * P.nnz + (P.nnz - P.nvar), s.vals + b * P.nnz + (P.nnz - P.nvar), (size_t)P.nvar * sizeof(double),
                            hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  holds_factor(h, s.vals, success);
  return CNL_OK;
}

// Small batches on a staged handle: the rho ladder is driven from the HOST, like the reference's own newton_system!
// (src/CaNNOLeS.jl:1023-1047) — every rung is a staged try_to_factorize (all tasks of the elimination tree in parallel, ~0.1 ms)
// and a read-back of the success flags.  The sequential launch that takes failed problems through the ladder on the device
// walks the latency plan's fronts one after the other on ONE wavefront per four problems: 7.7 ms per rung for a system of
// cfg3's size (38 ms for nfact = 6, ten times one CPU core of the oracle); it stays the device-pointer calls' fallback.
// (handles whose in-kernel device ladder is available use that one: no round trip per rung — 0.67 against 0.9 ms for one system of
//  cfg3's size that climbs to nfact = 6)
// any_device_ladder: also where the in-kernel ladder is available (the chunked call: its chunks run on views, which have none)
bool host_ladder_serves(const cnl_handle* h, bool any_device_ladder) {
  const cnl::Plan& P = h->plan->P;
  // (a staged Float32 handle — tuning float32_staged — is never claimed: its host-pointer calls take the plain route over the float
  //  staging, and the routes below stage Float64 arrays)
  return !h->f32 && h->staged && !h->dense && !h->gdense && h->plan->opt.host_ladder != 0 && h->use_v2 && P.rec_direct && P.d_outer &&
         (any_device_ladder || h->lad_mode == 0 || h->split_staged > 0);
}
// The first attempt of the whole staged batch, as both routes below begin: inputs up, one call of run() — on a handle the host
// ladder serves the staged attempt alone.
int newton_first_attempt(cnl_handle* h, const Stage<double>& s, const double* vals, const double* rhs, const double* rho_old, const double params[9],
                         bool host_ladder) {
  HIPCHK(upload_inputs(h, s, 0, (size_t)h->batch, vals, rhs, rho_old, h->stream));
  const int rc = run_typed(h, cnl::MODE_NEWTON, params, 9, newton_results(s), s.vals, s.rhs, s.d, h->stream, RunOpts{host_ladder, false});
  if (rc == CNL_OK) factor_is_of(h, s.vals);   // (newton_system factorised them: what the caller does next on the device starts from here)
  return rc;
}

// Small batches (the reference's own call: one system): every result goes to ONE pinned block of the handle with asynchronous
// copies and a single synchronisation; the caller's arrays are then filled on the host by the reference's rules (d only
// where the factorisation succeeded, the rho slots of vals only where the ladder wrote them).  Copies into pageable memory
// block one by one, and the success flags would need a round trip of their own before d may be copied.
int newton_small_pinned(cnl_handle* h, double* vals, const double* rhs, double* d, const double* rho_old, const double params[9], double* rho,
                        double* rho_old_out, int32_t* nfact, int32_t* success, bool host_ladder) {
  const cnl_plan& P = *h->plan;
  const Stage<double> s = stage<double>(h);
  const size_t B = (size_t)h->batch;
  int rc;
  if ((rc = newton_first_attempt(h, s, vals, rhs, rho_old, params, host_ladder))) return rc;
  const size_t o_d = 0, o_tail = o_d + B * P.N * 8, o_rho = o_tail + B * P.nvar * 8, o_ro = o_rho + B * 8, o_nf = o_ro + B * 8,
               o_su = o_nf + B * 4, o_up = (o_su + B * 4 + 7) & ~(size_t)7, total = o_up + B * 12 + 8;
  if (int prc = ensure_pinned(h, total)) return prc;
  char* pb = static_cast<char*>(h->pin);
  HIPCHK(hipMemcpyAsync(pb + o_d, s.d, B * P.N * 8, hipMemcpyDeviceToHost, h->stream));
  // (with the host-driven ladder the first attempt never writes the rho slots: they come back only behind a ladder, or behind the
  //  sequential redo of a dataflow time-out)
  // (the rho slots come back only where a ladder wrote them: nfact > 1 — known after the first synchronisation; copying them
  //  on every call cost the common one-system call 40 us of its 0.24 ms)
  bool tail_valid = false;
  // rho, rho_old, nfact, success: one block on both sides (Stage), one copy
  static_assert(sizeof(double) == 8 && sizeof(int32_t) == 4, "layout of the result block");
  HIPCHK(hipMemcpyAsync(pb + o_rho, s.rho, B * 24, hipMemcpyDeviceToHost, h->stream));
  int32_t* up_status = reinterpret_cast<int32_t*>(pb + o_up + B * 12);
  *up_status = 0;
  // per-call status of the dataflow execution (kernels2.hip, spin_until): waits that gave up.  Only calls that ran in dataflow
  // fashion on the whole handle can set it (split handles run through views: one launch per stage, nothing waits)
  if (host_ladder && h->d_dep && h->d_stat && h->split_staged == 0)
    HIPCHK(hipMemcpyAsync(up_status, h->d_stat, 4, hipMemcpyDeviceToHost, h->stream));
  //  ... and of the remainder handle's call, which does run in dataflow fashion on a handle of its own
  int32_t tail_status = 0;
  if (host_ladder && h->tail && h->tail->d_dep && h->tail->d_stat)
    HIPCHK(hipMemcpyAsync(&tail_status, h->tail->d_stat, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  std::memcpy(rho, pb + o_rho, B * 8);
  std::memcpy(rho_old_out, pb + o_ro, B * 8);
  std::memcpy(nfact, pb + o_nf, B * 4);
  std::memcpy(success, pb + o_su, B * 4);
  bool any_failed = false;
  for (size_t b = 0; b < B; b++) any_failed |= !success[b];
  if (host_ladder && any_failed && *up_status == 0) {
    if ((rc = host_ladder_run(h, params, rho_old, rho, rho_old_out, nfact, success, pb + o_up, reinterpret_cast<int32_t*>(pb + o_su), tail_status != 0))) return rc;
    HIPCHK(hipMemcpyAsync(pb + o_d, s.d, B * P.N * 8, hipMemcpyDeviceToHost, h->stream));
    if (P.nvar > 0) {
      HIPCHK(hipMemcpy2DAsync(pb + o_tail, (size_t)P.nvar * 8, s.vals + (P.nnz - P.nvar), (size_t)P.nnz * 8, (size_t)P.nvar * 8, B,
                              hipMemcpyDeviceToHost, h->stream));
      tail_valid = true;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
  } else if (P.nvar > 0) {
    // the device climbed a ladder (in-kernel ladder, sequential launch, or the redo behind a dataflow time-out): rho slots back
    bool climbed = false;
    for (size_t b = 0; b < B; b++) climbed |= nfact[b] > 1;
    if (climbed) {
      HIPCHK(hipMemcpy2DAsync(pb + o_tail, (size_t)P.nvar * 8, s.vals + (P.nnz - P.nvar), (size_t)P.nnz * 8, (size_t)P.nvar * 8, B,
                              hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
      tail_valid = true;
    }
  }
  for (size_t b = 0; b < B; b++) {
    if (success[b]) std::memcpy(d + b * P.N, pb + o_d + b * P.N * 8, (size_t)P.N * 8);
    // rho tail of vals (the reference mutates get_vals(LDLT)[end-nvar+1:end] on retries only, src/CaNNOLeS.jl:1031,1038); the
    // device copy holds what the caller passed wherever the ladder did not write, so copying it back always is the same
    if (P.nvar > 0 && tail_valid) std::memcpy(vals + b * P.nnz + (P.nnz - P.nvar), pb + o_tail + b * P.nvar * 8, (size_t)P.nvar * 8);
  }
  holds_factor(h, s.vals, success);
  return CNL_OK;
}

// Larger batches on a handle the host ladder serves: the first attempt, then — if a problem failed it and no dataflow wait gave up —
// the ladder on top of the first attempt's per-problem results (rho = 0, rho_old as given, nfact = 1).
int newton_staged_ladder(cnl_handle* h, double* vals, const double* rhs, double* d, const double* rho_old, const double params[9], double* rho,
                         double* rho_old_out, int32_t* nfact, int32_t* success) {
  const Stage<double> s = stage<double>(h);
  const size_t B = (size_t)h->batch;
  int rc;
  if ((rc = newton_first_attempt(h, s, vals, rhs, rho_old, params, true))) return rc;
  HIPCHK(hipMemcpyAsync(success, s.success, B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  // per-call status of the dataflow execution, of this handle and of the remainder's (see newton_small_pinned)
  int32_t status_word = 0, tail_status = 0;
  if (h->d_dep && h->d_stat && h->split_staged == 0) HIPCHK(hipMemcpyAsync(&status_word, h->d_stat, 4, hipMemcpyDeviceToHost, h->stream));
  if (h->tail && h->tail->d_dep && h->tail->d_stat) HIPCHK(hipMemcpyAsync(&tail_status, h->tail->d_stat, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  bool any_failed = false;
  for (size_t b = 0; b < B; b++) any_failed |= !success[b];
  HIPCHK(download_rho(s, 0, B, rho, rho_old_out, nfact, h->stream));
  if (status_word == 0 && any_failed) {
    HIPCHK(hipStreamSynchronize(h->stream));
    if ((rc = ensure_pinned(h, B * 16))) return rc;
    char* pb = static_cast<char*>(h->pin);
    if ((rc = host_ladder_run(h, params, rho_old, rho, rho_old_out, nfact, success, pb, reinterpret_cast<int32_t*>(pb + B * 12), tail_status != 0))) return rc;
  }
  HIPCHK(download_solution(h, s, 0, B, vals, d, success, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  holds_factor(h, s.vals, success);
  return CNL_OK;
}

}  // namespace

extern "C" {

int cnl_prepare_newton_system_dev(cnl_handle* h, int64_t nnzhF, int64_t nnzhc, int64_t nnzjF, int64_t nnzjc, const double* d_hF,
                                  const double* d_hc, const double* d_Jx, const double* d_Jcx, const double* d_delta, double* d_vals,
                                  void* stream) {
  if (!h || !d_vals || !d_Jx) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F64(h);
  return prepare_impl(h, nnzhF, nnzhc, nnzjF, nnzjc, d_hF, d_hc, d_Jx, d_Jcx, d_delta, d_vals, stream);
}

int cnl_cgls_multipliers_dev(cnl_handle* h, const double* d_vals, const double* d_r, double* d_lambda, double* d_Jxtr, double atol,
                             double rtol, int64_t itmax, int ones_if_zero, int32_t* d_iters, void* stream) {
  if (!h || !d_vals || !d_r) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F64(h);
  if (h->layout & 1) return fail(CNL_ERR_STATE, "cnl_cgls_multipliers_dev reads problem-major vals: on a handle with batch_layout = CNL_LAYOUT_INTERLEAVED use cnl_cgls_multipliers_jac_dev");
  return cgls_impl(h, cnl::JacSrc{d_vals, h->djt.nnz, d_vals, h->djt.nnz, 0, 0}, d_r, d_lambda, d_Jxtr, atol, rtol, itmax, ones_if_zero, d_iters, stream);
}

int cnl_cgls_multipliers_jac_dev(cnl_handle* h, int64_t nnzjF, int64_t nnzjc, const double* d_Jx, const double* d_Jcx, const double* d_r,
                                 double* d_lambda, double* d_Jxtr, double atol, double rtol, int64_t itmax, int ones_if_zero, int32_t* d_iters,
                                 void* stream) {
  if (!h || !d_r) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F64(h);
  cnl::JacSrc S{};
  if (int rc = jac_source(h, nnzjF, nnzjc, d_Jx, d_Jcx, &S)) return rc;
  return cgls_impl(h, S, d_r, d_lambda, d_Jxtr, atol, rtol, itmax, ones_if_zero, d_iters, stream);
}

int cnl_residual_vectors_dev(cnl_handle* h, const double* d_vals, const double* d_r, const double* d_lambda, const double* d_Fx,
                             const double* d_cx, double* d_rhs, double* d_norms, void* stream) {
  if (!h || !d_vals) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F64(h);
  if (h->layout & 1) return fail(CNL_ERR_STATE, "cnl_residual_vectors_dev reads problem-major vals: on a handle with batch_layout = CNL_LAYOUT_INTERLEAVED use cnl_residual_vectors_jac_dev");
  return residual_vectors_impl(h, cnl::JacSrc{d_vals, h->djt.nnz, d_vals, h->djt.nnz, 0, 0}, d_r, d_lambda, d_Fx, d_cx, d_rhs, d_norms, stream);
}

int cnl_residual_vectors_jac_dev(cnl_handle* h, int64_t nnzjF, int64_t nnzjc, const double* d_Jx, const double* d_Jcx, const double* d_r,
                                 const double* d_lambda, const double* d_Fx, const double* d_cx, double* d_rhs, double* d_norms, void* stream) {
  if (!h) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F64(h);
  cnl::JacSrc S{};
  if (int rc = jac_source(h, nnzjF, nnzjc, d_Jx, d_Jcx, &S)) return rc;
  return residual_vectors_impl(h, S, d_r, d_lambda, d_Fx, d_cx, d_rhs, d_norms, stream);
}

int cnl_kkt_residual_dev(cnl_handle* h, const double* d_vals, const double* d_rhs, const double* d_d, double* d_g, double* d_norms, void* stream) {
  if (!h || !d_vals || !d_rhs || !d_d || !d_g) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F64(h);
  if (h->layout & 1) return fail(CNL_ERR_STATE, "cnl_kkt_residual_dev reads problem-major vals: this handle was created with batch_layout = CNL_LAYOUT_INTERLEAVED");
  return kkt_residual(h, d_vals, d_rhs, d_d, d_g, d_norms, (hipStream_t)stream);
}

int cnl_trial_point_dev(cnl_handle* h, const double* d_x, const double* d_r, const double* d_lambda, const double* d_d,
                        double max_dlambda, double* d_xt, double* d_rt, double* d_lambdat, double* d_dlambda, void* stream) {
  if (!h || !d_x || !d_r || !d_d || !d_xt || !d_rt) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F64(h);
  return trial_point_impl(h, d_x, d_r, d_lambda, d_d, max_dlambda, d_xt, d_rt, d_lambdat, d_dlambda, stream);
}

// Float32 twins (include/cannoles_hip.h): the same rows on a Float32 handle's float arrays
int cnl_prepare_newton_system_f32_dev(cnl_handle* h, int64_t nnzhF, int64_t nnzhc, int64_t nnzjF, int64_t nnzjc, const float* d_hF,
                                      const float* d_hc, const float* d_Jx, const float* d_Jcx, const float* d_delta, float* d_vals,
                                      void* stream) {
  if (!h || !d_vals || !d_Jx) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F32(h);
  return prepare_impl(h, nnzhF, nnzhc, nnzjF, nnzjc, d_hF, d_hc, d_Jx, d_Jcx, d_delta, d_vals, stream);
}

int cnl_residual_vectors_f32_dev(cnl_handle* h, const float* d_vals, const float* d_r, const float* d_lambda, const float* d_Fx,
                                 const float* d_cx, float* d_rhs, float* d_norms, void* stream) {
  if (!h || !d_vals) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F32(h);
  if (h->layout & 1) return fail(CNL_ERR_STATE, "cnl_residual_vectors_f32_dev reads problem-major vals: on a handle with batch_layout = CNL_LAYOUT_INTERLEAVED use cnl_residual_vectors_jac_f32_dev");
  return residual_vectors_impl(h, cnl::JacSrcF{d_vals, h->djt.nnz, d_vals, h->djt.nnz, 0, 0}, d_r, d_lambda, d_Fx, d_cx, d_rhs, d_norms, stream);
}

int cnl_residual_vectors_jac_f32_dev(cnl_handle* h, int64_t nnzjF, int64_t nnzjc, const float* d_Jx, const float* d_Jcx, const float* d_r,
                                     const float* d_lambda, const float* d_Fx, const float* d_cx, float* d_rhs, float* d_norms, void* stream) {
  if (!h) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F32(h);
  cnl::JacSrcF S{};
  if (int rc = jac_source(h, nnzjF, nnzjc, d_Jx, d_Jcx, &S)) return rc;
  return residual_vectors_impl(h, S, d_r, d_lambda, d_Fx, d_cx, d_rhs, d_norms, stream);
}

int cnl_cgls_multipliers_f32_dev(cnl_handle* h, const float* d_vals, const float* d_r, float* d_lambda, float* d_Jxtr, float atol,
                                 float rtol, int64_t itmax, int ones_if_zero, int32_t* d_iters, void* stream) {
  if (!h || !d_vals || !d_r) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F32(h);
  if (h->layout & 1) return fail(CNL_ERR_STATE, "cnl_cgls_multipliers_f32_dev reads problem-major vals: on a handle with batch_layout = CNL_LAYOUT_INTERLEAVED use cnl_cgls_multipliers_jac_f32_dev");
  return cgls_impl(h, cnl::JacSrcF{d_vals, h->djt.nnz, d_vals, h->djt.nnz, 0, 0}, d_r, d_lambda, d_Jxtr, atol, rtol, itmax, ones_if_zero, d_iters, stream);
}

int cnl_cgls_multipliers_jac_f32_dev(cnl_handle* h, int64_t nnzjF, int64_t nnzjc, const float* d_Jx, const float* d_Jcx, const float* d_r,
                                     float* d_lambda, float* d_Jxtr, float atol, float rtol, int64_t itmax, int ones_if_zero, int32_t* d_iters,
                                     void* stream) {
  if (!h || !d_r) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F32(h);
  cnl::JacSrcF S{};
  if (int rc = jac_source(h, nnzjF, nnzjc, d_Jx, d_Jcx, &S)) return rc;
  return cgls_impl(h, S, d_r, d_lambda, d_Jxtr, atol, rtol, itmax, ones_if_zero, d_iters, stream);
}

int cnl_trial_point_f32_dev(cnl_handle* h, const float* d_x, const float* d_r, const float* d_lambda, const float* d_d,
                            float max_dlambda, float* d_xt, float* d_rt, float* d_lambdat, float* d_dlambda, void* stream) {
  if (!h || !d_x || !d_r || !d_d || !d_xt || !d_rt) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F32(h);
  return trial_point_impl(h, d_x, d_r, d_lambda, d_d, max_dlambda, d_xt, d_rt, d_lambdat, d_dlambda, stream);
}

// ---- factorize / solve / newton_system: device pointers, host pointers, and their Float32 twins ----
int cnl_factorize_dev(cnl_handle* h, const double* d_vals, double eig_tol, int32_t* d_success, void* stream) {
  if (!h || !d_vals || !d_success) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F64(h);
  return factorize_dev_impl(h, d_vals, eig_tol, d_success, stream);
}
int cnl_factorize_f32_dev(cnl_handle* h, const float* d_vals, float eig_tol, int32_t* d_success, void* stream) {
  if (!h || !d_vals || !d_success) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F32(h);
  return factorize_dev_impl(h, d_vals, eig_tol, d_success, stream);
}

int cnl_solve_dev(cnl_handle* h, const double* d_rhs, double* d_d, void* stream) {
  if (!h || !d_rhs || !d_d) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F64(h);
  return solve_dev_impl(h, d_rhs, d_d, stream);
}
int cnl_solve_f32_dev(cnl_handle* h, const float* d_rhs, float* d_d, void* stream) {
  if (!h || !d_rhs || !d_d) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F32(h);
  return solve_dev_impl(h, d_rhs, d_d, stream);
}

int cnl_newton_system_dev(cnl_handle* h, double* d_vals, const double* d_rhs, double* d_d, double* d_rho_old, double* d_rho,
                          int32_t* d_nfact, int32_t* d_success, const double params[9], void* stream) {
  if (!h || !d_vals || !d_rhs || !d_d || !d_rho_old || !d_rho || !d_nfact || !d_success || !params)
    return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F64(h);
  return newton_system_dev_impl(h, d_vals, d_rhs, d_d, d_rho_old, d_rho, d_nfact, d_success, params, stream);
}
int cnl_newton_system_f32_dev(cnl_handle* h, float* d_vals, const float* d_rhs, float* d_d, float* d_rho_old, float* d_rho,
                              int32_t* d_nfact, int32_t* d_success, const float params[9], void* stream) {
  if (!h || !d_vals || !d_rhs || !d_d || !d_rho_old || !d_rho || !d_nfact || !d_success || !params)
    return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F32(h);
  return newton_system_dev_impl(h, d_vals, d_rhs, d_d, d_rho_old, d_rho, d_nfact, d_success, params, stream);
}

int cnl_factorize(cnl_handle* h, const double* vals, double eig_tol, int32_t* success, int64_t* npos, int64_t* nzero) {
  if (!h || !vals || !success) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F64(h);
  CNL_NEED_FULL_BATCH(h);
  return factorize_impl(h, vals, eig_tol, success, npos, nzero);
}
int cnl_factorize_f32(cnl_handle* h, const float* vals, float eig_tol, int32_t* success, int64_t* npos, int64_t* nzero) {
  if (!h || !vals || !success) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F32(h);
  CNL_NEED_FULL_BATCH(h);
  return factorize_impl(h, vals, eig_tol, success, npos, nzero);
}

int cnl_solve(cnl_handle* h, const double* rhs, double* d) {
  if (!h || !rhs || !d) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F64(h);
  CNL_NEED_FULL_BATCH(h);
  return solve_impl(h, rhs, d);
}
int cnl_solve_f32(cnl_handle* h, const float* rhs, float* d) {
  if (!h || !rhs || !d) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F32(h);
  CNL_NEED_FULL_BATCH(h);
  return solve_impl(h, rhs, d);
}

int cnl_newton_system(cnl_handle* h, double* vals, const double* rhs, double* d, const double* rho_old, const double params[9],
                      double* rho, double* rho_old_out, int32_t* nfact, int32_t* success) {
  if (!h || !vals || !rhs || !d || !params || !rho || !rho_old_out || !nfact || !success) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F64(h);
  CNL_NEED_FULL_BATCH(h);
  if (h->layout) return fail(CNL_ERR_STATE, kHostLayout);
  HIPCHK(hipSetDevice(h->device));
  if (int rc = ensure_staging(h)) return rc;
  // (a refined handle — tuning float32_refine — takes the plain route: the routes below are Float64 kernels' business)
  if (h->inner) return newton_system_impl(h, vals, rhs, d, rho_old, params, rho, rho_old_out, nfact, success);
  const cnl_plan& P = *h->plan;
  const size_t B = (size_t)h->batch;
  if (!h->dense && !h->gdense && !h->timing && B >= 32 && B * (size_t)(P.nnz + P.N) * sizeof(double) >= ((size_t)96 << 20)) {
    // eight chunks or more, each a multiple of four problems and at least 16 MB of upload
    size_t chunk = std::max<size_t>(16, ((B / 8) + 3) & ~(size_t)3);
    const size_t per = (size_t)(P.nnz + P.N) * sizeof(double);
    while (chunk * per < ((size_t)16 << 20) && chunk < B) chunk += 4;
    // band kernels: the factor records of a workgroup's problems (8, 16 or 32) are interleaved in ONE region of the factor storage;
    // chunks run concurrently on different streams, so their regions must not share a workgroup
    if (h->band) chunk = (chunk + 31) & ~(size_t)31;
    if (chunk < B) return newton_system_pipelined(h, vals, rhs, d, rho_old, params, rho, rho_old_out, nfact, success, chunk);
  }
  if (h->dense && !h->timing && P.opt.host_ladder != 0)
    return newton_dense_host_ladder(h, vals, rhs, d, rho_old, params, rho, rho_old_out, nfact, success);
  const bool host_ladder = host_ladder_serves(h, false);
  if (B * (size_t)P.N * sizeof(double) <= ((size_t)1 << 20))
    return newton_small_pinned(h, vals, rhs, d, rho_old, params, rho, rho_old_out, nfact, success, host_ladder);
  if (host_ladder) return newton_staged_ladder(h, vals, rhs, d, rho_old, params, rho, rho_old_out, nfact, success);
  return newton_system_impl(h, vals, rhs, d, rho_old, params, rho, rho_old_out, nfact, success);
}
int cnl_newton_system_f32(cnl_handle* h, float* vals, const float* rhs, float* d, const float* rho_old, const float params[9], float* rho,
                          float* rho_old_out, int32_t* nfact, int32_t* success) {
  if (!h || !vals || !rhs || !d || !params || !rho || !rho_old_out || !nfact || !success) return fail(CNL_ERR_ARG, "null argument");
  CNL_NEED_F32(h);
  CNL_NEED_FULL_BATCH(h);
  if (h->layout) return fail(CNL_ERR_STATE, kHostLayout);
  HIPCHK(hipSetDevice(h->device));
  if (int rc = ensure_staging(h)) return rc;
  return newton_system_impl(h, vals, rhs, d, rho_old, params, rho, rho_old_out, nfact, success);
}

}  // extern "C"
