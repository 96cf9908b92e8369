// kernels.hip — gfx950 (MI355X) kernels of the Newton-system path.
//
// One kernel executes the whole reference call
//   newton_system!(d, nvar, nequ, ncon, rhs, vals, LDLT, rho_old, params)
//   (/root/reference/src/CaNNOLeS.jl:1008-1052)
// for a batch of problems that share one sparsity pattern: KKT assembly with
// COO-order duplicate summation (set_vals!, src/solver_types.jl:53-59), LDL^T
// factorisation, inertia test (src/solver_types.jl:90-97), the per-problem rho
// ladder and the solve d = -K^-1 rhs (src/solver_types.jl:69-77).
//
// Mapping: a group of TPP threads (a wavefront, a fraction of one, or a whole
// workgroup) owns one problem and walks the static multifrontal plan built on
// the host (analysis.cpp).  Fronts are packed lower triangles addressed in
// REVERSED order: local index 0 is the right-hand-side row, 1..nupd the update
// rows, the pivots come last and are eliminated from the highest index down,
// so that after the pivots are gone the update matrix is the packed prefix of
// the front and the L panel is its packed suffix (one contiguous, coalesced
// store to HBM).  The update-matrix stack lives in LDS at offsets computed on
// the host; there is no inter-workgroup communication and no atomic.
//
// Every function is a template on the element type T: double for the Float64 handles, float for the Float32 handles that run on
// this kernel (tuning float32_general).  With T = float values, right-hand side, d, rho, the factor panels, the
// work area and the reduction scratch are float and every operation is a float operation; the parameters arrive widened in
// LaunchArgs::params and are narrowed back.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace cnl {

__device__ __forceinline__ int tri_i(int i) { return (int)(((unsigned)i * (unsigned)(i + 1)) >> 1); }

__device__ __forceinline__ void tri_decode(int t, int& a, int& b) {
  a = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while (tri_i(a + 1) <= t) a++;
  while (tri_i(a) > t) a--;
  b = t - tri_i(a);
}

// synchronise the TPP threads that own one problem
template <int TPP, bool LDSW>
__device__ __forceinline__ void psync() {
  if (TPP <= 64) {
    // one wavefront (or part of one): LDS operations of a wave execute in
    // order, so a compiler-level fence is all that is needed; work areas in
    // global memory additionally need the stores drained (workgroup scope).
    if (LDSW) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    else __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// orders the factor phase (L panel stores) before the solve phase (panel loads by other lanes)
template <int TPP>
__device__ __forceinline__ void phase_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  if (TPP <= 64) __builtin_amdgcn_wave_barrier();
  else __syncthreads();
}

__device__ __forceinline__ double abs_of(double v) { return fabs(v); }
__device__ __forceinline__ float abs_of(float v) { return fabsf(v); }
__device__ __forceinline__ double max_of(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float max_of(float a, float b) { return fmaxf(a, b); }

template <int TPP, class T>
__device__ __forceinline__ T psum(T v, T* red, int tid) {
  if (TPP <= 64) {
#pragma unroll
    for (int o = TPP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, TPP);
    return v;
  } else {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    T s = 0;
    for (int w = 0; w < TPP / 64; w++) s += red[w];
    return s;
  }
}

template <class T>
struct ProblemCtx {
  const T* vals;  // this problem's COO values
  const T* rhs;
  T* L;
  T* W;           // work area (LDS or global)
  T* red;         // cross-wave reduction scratch (TPP > 64)
};

// ---------------------------------------------------------------------------
// Blocked elimination (tuning general_blocked, and float32_blocked on a Float32 handle): the pivots of a front
// leave in PANELS of up to PANEL_W, and what a panel owes the rows below it is one product on the matrix cores instead of PANEL_W
// sweeps over the packed triangle.
constexpr int PANEL_W = 16;
typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

// The 16 x 16 x 4 matrix-core instruction of an element type.  The operand maps are the same for both — lane l holds
// A[row l & 15][k = l >> 4] and B[k = l >> 4][column l & 15] — and the result maps are NOT: register r of lane l is column l & 15 of
// row (l >> 4) + 4 r in double, of row 4 (l >> 4) + r in float (dense_f32.hip, update_block).
template <class T>
struct PanelMma;
template <>
struct PanelMma<double> {
  typedef d4 acc_t;
  static __device__ __forceinline__ int row(int lg, int r) { return lg + 4 * r; }
  static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
};
template <>
struct PanelMma<float> {
  typedef f4 acc_t;
  static __device__ __forceinline__ int row(int lg, int r) { return 4 * lg + r; }
  static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};

// F[a][b] -= sum_k L[k][a] W[k][b] for b <= a < lim, k < kp: L[k] is the scaled row of the panel's pivot p0 + k (in place in F),
// W[k] its unscaled copy (Wp, stride ws).  16 x 16 tiles of the packed triangle, dealt round-robin to the wavefronts of the
// workgroup; one tile is four v_mfma_f64_16x16x4_f64 (float: v_mfma_f32_16x16x4_f32) on two accumulator chains (dense.hip,
// update_block), the accumulator loaded from F and stored back by the result map of the instruction (PanelMma::row).
// Rows and columns beyond lim and panel slots beyond kp enter as zeros (selected, not multiplied: the slots may hold
// anything); a diagonal tile computes the whole tile and stores b <= a.  The trip count depends on the wavefront alone.
// LPAN (tuning subtree_lds_panels): the scaled rows are read from Lr, the copy of the piece F[tri_i(p0) ..) that eliminate_blocked keeps in
// LDS (Lr[0] is F[tri_i(p0)]), and Wp is in LDS too; the accumulator tiles are F's as ever.
template <int TPP, class T, bool LPAN = false>
__device__ __forceinline__ void panel_trailing_update(T* F, const T* Wp, int ws, int p0, int kp, int lim, int tid, const T* Lr = nullptr) {
  typedef PanelMma<T> M;
  const int lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int nt = (lim + PANEL_W - 1) / PANEL_W, ntiles = tri_i(nt);
  for (int t = wave; t < ntiles; t += TPP / 64) {
    int ta, tb;
    tri_decode(t, ta, tb);
    const int ar = PANEL_W * ta + li, bc = PANEL_W * tb + li;
    T aop[4], bop[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int k = 4 * s + lg;
      if constexpr (LPAN) aop[s] = (k < kp && ar < lim) ? -Lr[tri_i(p0 + k) - tri_i(p0) + ar] : T(0);
      else aop[s] = (k < kp && ar < lim) ? -F[tri_i(p0 + k) + ar] : T(0);
      bop[s] = (k < kp && bc < lim) ? Wp[k * ws + bc] : T(0);
    }
    typename M::acc_t acc, acc2 = typename M::acc_t{T(0), T(0), T(0), T(0)};
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int a = PANEL_W * ta + M::row(lg, r);
      acc[r] = (a < lim && bc <= a) ? F[tri_i(a) + bc] : T(0);
    }
    acc = M::mma(aop[0], bop[0], acc);
    acc2 = M::mma(aop[1], bop[1], acc2);
    acc = M::mma(aop[2], bop[2], acc);
    acc2 = M::mma(aop[3], bop[3], acc2);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int a = PANEL_W * ta + M::row(lg, r);
      if (a < lim && bc <= a) F[tri_i(a) + bc] = acc[r] + acc2[r];
    }
  }
}

// The blocked twin of the WITH_K elimination loop of front_forward, for a front with at least PANEL_W pivots: panels from the highest
// local index down, the last one of a kind as narrow as it comes.  The leading H.indep pivots (local index >= idep) do not touch
// each other: their panels need no step inside the panel and their trailing triangle ends at idep.  A dependent panel runs its
// pivots one by one — pivot read after every earlier pivot's update has reached it, counted against eig_tol, row kept unscaled in
// W, scaled in place, rank-1 update of the rows of the panel still to come (a contiguous piece of the packed triangle) — and then
// updates everything below it at once.
// LPAN (tuning subtree_lds_panels; the work area is global): a dependent panel [p0, p1) runs its pivot loop on a copy
// of its rows in LDS — the contiguous piece F[tri_i(p0) .. tri_i(p1)), at most PANEL_W rows of at most P.fmax elements, at lds; the
// unscaled rows at lds + PANEL_W * P.fmax, PANEL_W rows of stride P.fmax — with the statements of the loop below in their order, hands
// both areas to the trailing update and writes the piece back (the trailing update writes rows below p0 only).  The launch sized the
// areas for the stage's largest P.fmax.  Independent panels run as ever, on F and Wp.
template <int TPP, bool LDSW, class T, bool LPAN = false>
__device__ __forceinline__ void eliminate_blocked(const DevPlan& P, T* F, T* Wp, int f, int nupd, int idep, int tid, T eig_tol,
                                                  int& npos, int& nzer, T* lds = nullptr) {
  const int ws = P.fmax;
  int p1 = f;
  while (p1 > nupd + 1) {
    const bool indep = p1 > idep;
    const int floor_ = indep ? idep : nupd + 1;
    const int p0 = p1 - PANEL_W > floor_ ? p1 - PANEL_W : floor_;
    const int kp = p1 - p0;
    const int lim = indep ? idep : p0;
    if (indep) {
      for (int k = 0; k < kp; k++) {
        T* rowi = F + tri_i(p0 + k);
        T* wk = Wp + k * ws;
        const T dpiv = rowi[p0 + k];
        npos += dpiv > eig_tol;
        nzer += abs_of(dpiv) <= eig_tol;
        for (int j = tid; j < lim; j += TPP) {
          const T w = rowi[j];
          wk[j] = w;
          rowi[j] = w / dpiv;
        }
      }
      psync<TPP, LDSW>();
    } else if constexpr (LPAN) {
      T* const Ls = lds;
      T* const Wl = lds + PANEL_W * ws;
      const int t0 = tri_i(p0), tlen = tri_i(p1) - t0;
      for (int t = tid; t < tlen; t += TPP) Ls[t] = F[t0 + t];
      psync<TPP, LDSW>();
      for (int k = kp - 1; k >= 0; k--) {
        const int i = p0 + k;
        T* rowi = Ls + (tri_i(i) - t0);
        T* wk = Wl + k * ws;
        const T dpiv = rowi[i];
        npos += dpiv > eig_tol;
        nzer += abs_of(dpiv) <= eig_tol;
        for (int j = tid; j < i; j += TPP) {
          const T w = rowi[j];
          wk[j] = w;
          rowi[j] = w / dpiv;
        }
        psync<TPP, LDSW>();
        const int t1 = tri_i(i);   // rows p0 .. i - 1 of the packed triangle
        if (t0 + tid < t1) {
          int a, b;
          tri_decode(t0 + tid, a, b);
          for (int t = t0 + tid; t < t1; t += TPP) {
            Ls[t - t0] -= rowi[a] * wk[b];
            b += TPP;
            while (b > a) { b -= a + 1; a++; }
          }
        }
        psync<TPP, LDSW>();
      }
      for (int t = tid; t < tlen; t += TPP) F[t0 + t] = Ls[t];
      panel_trailing_update<TPP, T, true>(F, Wl, ws, p0, kp, lim, tid, Ls);
      psync<TPP, LDSW>();
      p1 = p0;
      continue;
    } else {
      for (int k = kp - 1; k >= 0; k--) {
        const int i = p0 + k;
        T* rowi = F + tri_i(i);
        T* wk = Wp + k * ws;
        const T dpiv = rowi[i];
        npos += dpiv > eig_tol;
        nzer += abs_of(dpiv) <= eig_tol;
        for (int j = tid; j < i; j += TPP) {
          const T w = rowi[j];
          wk[j] = w;
          rowi[j] = w / dpiv;
        }
        psync<TPP, LDSW>();
        const int t0 = tri_i(p0), t1 = tri_i(i);   // rows p0 .. i - 1 of the packed triangle
        if (t0 + tid < t1) {
          int a, b;
          tri_decode(t0 + tid, a, b);
          for (int t = t0 + tid; t < t1; t += TPP) {
            F[t] -= rowi[a] * wk[b];
            b += TPP;
            while (b > a) { b -= a + 1; a++; }
          }
        }
        psync<TPP, LDSW>();
      }
    }
    panel_trailing_update<TPP>(F, Wp, ws, p0, kp, lim, tid);
    psync<TPP, LDSW>();
    p1 = p0;
  }
}

// ---------------------------------------------------------------------------
// forward pass over one front: assemble, extend-add, eliminate the pivots,
// store the L panel, leave the update matrix for the parent.
// BLK (TPP a multiple of 64): fronts with at least PANEL_W pivots are eliminated by eliminate_blocked
// LPAN (only with BLK, work area global): ... whose dependent panels run in the LDS areas behind the 16 elements of c.red
template <int TPP, bool LDSW, bool WITH_K, class T, bool BLK = false, bool LPAN = false>
__device__ __forceinline__ void front_forward(const DevPlan& P, const FrontHdr& H, const ProblemCtx<T>& c, int tid,
                                              bool rho_override, T rho, T eig_tol, int& npos, int& nzer) {
  const int nupd = H.nupd, npiv = H.npiv;
  const int f = 1 + nupd + npiv;
  const int tf = tri_i(f);
  const int tu = tri_i(1 + nupd);
  T* F = c.W + H.foff;
  T* Lp = c.L + ((long long)H.lptr_lo | ((long long)H.lptr_hi << 31));

  if (WITH_K) {
    for (int t = tid; t < tf; t += TPP) F[t] = T(0);
    psync<TPP, LDSW>();
    // assembly rounds (round r holds the r-th duplicate of every slot: COO-order sums)
    for (int r = H.seg_begin; r < H.seg_end; r++) {
      const int e0 = P.seg_ptr[r], e1 = P.seg_ptr[r + 1];
      for (int e = e0 + tid; e < e1; e += TPP) {
        const int src = P.asm_src[e], pos = P.asm_pos[e];
        T v;
        if (src >= P.nnz) v = c.rhs ? c.rhs[src - P.nnz] : T(0);
        else if (rho_override && src >= P.rho_begin) v = rho;
        else v = c.vals[src];
        F[pos] += v;
      }
      psync<TPP, LDSW>();
    }
    // extend-add of the children's update matrices
    for (int ci = H.child_begin; ci < H.child_end; ci++) {
      const FrontHdr& C = P.fronts[P.child_idx[ci]];
      const int tuc = tri_i(1 + C.nupd);
      const T* U = c.W + C.ubase;
      const int* rel = P.rel_idx + C.rel_begin;
      if (tid < tuc) {
        int a, b;
        tri_decode(tid, a, b);
        for (int t = tid; t < tuc; t += TPP) {
          const int ra = rel[a], rb = rel[b];
          F[tri_i(ra) + rb] += U[t];
          b += TPP;
          while (b > a) { b -= a + 1; a++; }
        }
      }
      psync<TPP, LDSW>();
    }
  } else {
    // vector-only forward solve (cnl_solve): F is the front's right-hand side vector
    for (int t = tid; t < f; t += TPP) {
      T v = T(0);
      if (t > nupd) v = c.rhs[P.perm[H.first_piv + (f - 1 - t)]];
      F[t] = v;
    }
    psync<TPP, LDSW>();
    for (int ci = H.child_begin; ci < H.child_end; ci++) {
      const FrontHdr& C = P.fronts[P.child_idx[ci]];
      const T* U = c.W + C.ubase;
      const int* rel = P.rel_idx + C.rel_begin;
      for (int a = 1 + tid; a <= C.nupd; a += TPP) F[rel[a]] += U[a];
      psync<TPP, LDSW>();
    }
  }

  if (WITH_K) {
    T* wv0 = c.W + P.wv_off;
    const int idep = f - H.indep;  // pivots with local index >= idep are mutually independent
    bool blocked = false;
    if constexpr (BLK) {
      blocked = npiv >= PANEL_W;
      if constexpr (LPAN) {
        if (blocked) eliminate_blocked<TPP, LDSW, T, true>(P, F, wv0, f, nupd, idep, tid, eig_tol, npos, nzer, c.red + 16);
      } else {
        if (blocked) eliminate_blocked<TPP, LDSW>(P, F, wv0, f, nupd, idep, tid, eig_tol, npos, nzer);
      }
    }
    for (int i = blocked ? nupd : f - 1; i > nupd; i--) {
      const int ulim = i >= idep ? idep : i;
      T* rowi = F + tri_i(i);
      T* wv = wv0 + ((i & 1) ? P.fmax : 0);
      const T dpiv = rowi[i];
      npos += dpiv > eig_tol;
      nzer += abs_of(dpiv) <= eig_tol;
      for (int j = tid; j < ulim; j += TPP) {
        const T w = rowi[j];
        wv[j] = w;
        rowi[j] = w / dpiv;
      }
      psync<TPP, LDSW>();
      const int tul = tri_i(ulim);
      if (tid < tul) {
        int a, b;
        tri_decode(tid, a, b);
        for (int t = tid; t < tul; t += TPP) {
          F[t] -= rowi[a] * wv[b];
          b += TPP;
          while (b > a) { b -= a + 1; a++; }
        }
      }
      psync<TPP, LDSW>();
    }
    // L panel (packed suffix of the front) -> HBM, coalesced
    for (int t = tu + tid; t < tf; t += TPP) Lp[t - tu] = F[t];
  } else {
    // forward substitution with the stored panel: z_i = w_i / d_i, v_j -= l_ij w_i
    const int idep = f - H.indep;
    T* PB = c.W + P.pb_off;
    const int plen = tf - tu;
    for (int t = tid; t < plen; t += TPP) PB[t] = Lp[t];
    psync<TPP, LDSW>();
    for (int i = f - 1; i > nupd; i--) {
      const int ulim = i >= idep ? idep : i;
      const T* rowi = PB + (tri_i(i) - tu);
      const T w = F[i];
      psync<TPP, LDSW>();
      for (int j = 1 + tid; j < ulim; j += TPP) F[j] -= rowi[j] * w;
      if (tid == 0) Lp[tri_i(i) - tu] = w / rowi[i];
      psync<TPP, LDSW>();
    }
  }

  // hand the update matrix (or vector) to the parent: move it down the stack
  const int ulen = WITH_K ? tu : 1 + nupd;
  if (H.ubase != H.foff) {
    T* U = c.W + H.ubase;
    for (int t0 = 0; t0 < ulen; t0 += TPP) {
      const int t = t0 + tid;
      T v = T(0);
      if (t < ulen) v = F[t];
      psync<TPP, LDSW>();
      if (t < ulen) U[t] = v;
      psync<TPP, LDSW>();
    }
  } else {
    psync<TPP, LDSW>();
  }
}

// backward pass over one front: x_i = z_i - sum_j l_ij x_j ;  d = -x
template <int TPP, bool LDSW, class T>
__device__ __forceinline__ void front_backward(const DevPlan& P, const FrontHdr& H, const ProblemCtx<T>& c, int tid, T* dout) {
  const int nupd = H.nupd, npiv = H.npiv;
  const int f = 1 + nupd + npiv;
  const int tu = tri_i(1 + nupd);
  const int plen = tri_i(f) - tu;
  T* X = c.W + H.xoff;
  const T* Lp = c.L + ((long long)H.lptr_lo | ((long long)H.lptr_hi << 31));
  T* PB = c.W + P.pb_off;
  for (int t = tid; t < plen; t += TPP) PB[t] = Lp[t];
  if (H.parent >= 0) {
    const T* Xp = c.W + P.fronts[H.parent].xoff;
    const int* rel = P.rel_idx + H.rel_begin;
    for (int j0 = 1; j0 <= nupd; j0 += TPP) {
      const int j = j0 + tid;
      T v = T(0);
      if (j <= nupd) v = Xp[rel[j]];
      psync<TPP, LDSW>();
      if (j <= nupd) X[j] = v;
      psync<TPP, LDSW>();
    }
  }
  psync<TPP, LDSW>();
  for (int i = nupd + 1; i < f; i++) {
    const T* rowi = PB + (tri_i(i) - tu);
    T part = T(0);
    for (int j = 1 + tid; j < i; j += TPP) part += rowi[j] * X[j];
    const T acc = psum<TPP>(part, c.red, tid);
    const T xi = rowi[0] - acc;
    if (tid == 0) {
      X[i] = xi;
      dout[P.perm[H.first_piv + (f - 1 - i)]] = -xi;
    }
    psync<TPP, LDSW>();
  }
}

template <int TPP, bool LDSW, class T, bool BLK>
__device__ __forceinline__ bool factor_attempt(const DevPlan& P, const ProblemCtx<T>& c, int tid, bool rho_override, T rho,
                                               T eig_tol, int& npos_out, int& nzer_out, int xpos, int xzer) {
  int npos = xpos, nzer = xzer;
  for (int s = 0; s < P.nsuper; s++) front_forward<TPP, LDSW, true, T, BLK>(P, P.fronts[s], c, tid, rho_override, rho, eig_tol, npos, nzer);
  npos_out = npos; nzer_out = nzer;
  return npos == P.nvar && nzer == 0;  // src/solver_types.jl:96
}

template <class T>
__device__ __forceinline__ T* as_global(T* p) {  // struct members are generic pointers to the compiler: mark them global
  return (T*)(__attribute__((address_space(1))) T*)p;
}

// ---------------------------------------------------------------------------
// Subtree execution (tuning general_subtrees, and float32_subtrees on a Float32 handle; DESIGN sections 3.2 and 9.11; the SUB instances
// of newton_kernel: double or float, PPB = 1, work area in global scratch).  P.fronts is the plan's SECOND front table (plan.h:
// Plan::gfronts), whose offsets lie in the region of the front's task, and A.tasks the task records (plan.h: GTask, 8 words each).  A launch is one of
//   A.phase 0  forward of the tasks [A.task0, A.task0 + A.ntasks) of one stage, workgroup = (task, problem): MODE_NEWTON / MODE_FACTOR
//              assemble and eliminate the task's fronts at rho as given and leave the task's pivot counts in its own slot of
//              A.gcnt [tasks][batch][2] (no atomic, nothing to zero per call); MODE_SOLVE runs the vector sweep over the same fronts;
//   A.phase 1  backward sweep of the tasks of one stage, fronts from the task's last down; a problem without a factor
//              (A.success[b] == 0) is skipped by the whole workgroup;
//   A.phase 2  the climbers (MODE_NEWTON, A.skip_done = 1), workgroup = problem: a problem whose first attempt succeeded leaves at once,
//              a failed one runs the complete sequential newton_system — first attempt again, ladder, backward sweep, all outputs —
//              task by task over the same table (the subtree layout is a valid layout of a sequential walk too).
// Dependencies between tasks are the order of the launches on the stream: nothing here waits, and no two workgroups of a launch
// touch the same memory.  Control flow around every barrier is uniform per workgroup (one task of one problem).
enum { GT_STAGE = 0, GT_F0, GT_F1, GT_PARENT, GT_BASE, GT_PB_OFF, GT_WV_OFF, GT_FMAX, GT_WORDS = 8 };

// the plan as task k sees it: its own panel buffer and staging rows
__device__ __forceinline__ void sub_enter_task(DevPlan& P, const int32_t* tasks, int k, int& f0, int& f1) {
  const int32_t* t = tasks + (long long)k * GT_WORDS;
  f0 = t[GT_F0]; f1 = t[GT_F1];
  P.pb_off = t[GT_PB_OFF]; P.wv_off = t[GT_WV_OFF]; P.fmax = t[GT_FMAX];
}

template <int TPP, class T, bool BLK>
__device__ __forceinline__ bool sub_factor_attempt(DevPlan& P, const int32_t* tasks, int ntasks, const ProblemCtx<T>& c, int tid,
                                                   bool rho_override, T rho, T eig_tol, int xpos, int xzer) {
  int npos = xpos, nzer = xzer;
  for (int k = 0; k < ntasks; k++) {
    int f0, f1;
    sub_enter_task(P, tasks, k, f0, f1);
    for (int s = f0; s < f1; s++) front_forward<TPP, false, true, T, BLK>(P, P.fronts[s], c, tid, rho_override, rho, eig_tol, npos, nzer);
  }
  return npos == P.nvar && nzer == 0;
}

template <int TPP, class T>
__device__ __forceinline__ void sub_backward_all(DevPlan& P, const int32_t* tasks, int ntasks, const ProblemCtx<T>& c, int tid, T* dout) {
  for (int k = ntasks - 1; k >= 0; k--) {
    int f0, f1;
    sub_enter_task(P, tasks, k, f0, f1);
    for (int s = f1 - 1; s >= f0; s--) front_backward<TPP, false>(P, P.fronts[s], c, tid, dout);
  }
}

template <int TPP, class T, bool BLK, bool LPAN = false>
__device__ __forceinline__ void newton_subtrees(DevPlan& P, const LaunchArgs& A, T* smem) {
  T* const a_vals = static_cast<T*>(A.vals);
  const T* const a_rhs = static_cast<const T*>(A.rhs);
  T* const a_d = static_cast<T*>(A.d);
  const int32_t* const tasks = as_global(const_cast<int32_t*>(A.tasks));
  int* const gcnt = as_global(A.gcnt);
  const int tid = threadIdx.x;
  const bool climb = A.phase == 2;
  const int b = climb ? (int)blockIdx.x : (int)(blockIdx.x % (unsigned)A.batch);
  const int task = climb ? 0 : A.task0 + (int)(blockIdx.x / (unsigned)A.batch);
  if (b >= A.batch || task >= A.task0 + A.ntasks) return;
  ProblemCtx<T> c;
  c.vals = a_vals ? a_vals + (long long)b * P.vstride : nullptr;
  c.rhs = a_rhs ? a_rhs + (long long)b * P.rstride : nullptr;
  c.L = static_cast<T*>(A.L) + (long long)b * P.lsize;
  c.red = smem;
  c.W = static_cast<T*>(A.scratch) + (long long)b * P.work_doubles;
  T* dout = a_d ? a_d + (long long)b * P.dstride : nullptr;
  const T eig_tol = (T)A.params[0];

  if (!climb) {
    int f0, f1;
    sub_enter_task(P, tasks, task, f0, f1);
    if (A.phase == 1) {
      if (!A.success[b]) return;
      for (int s = f1 - 1; s >= f0; s--) front_backward<TPP, false>(P, P.fronts[s], c, tid, dout);
      return;
    }
    if (A.mode == MODE_SOLVE) {
      if (A.success && !A.success[b]) return;
      int np = 0, nz = 0;
      for (int s = f0; s < f1; s++) front_forward<TPP, false, false>(P, P.fronts[s], c, tid, false, T(0), eig_tol, np, nz);
      return;
    }
    if (A.mode == MODE_FACTOR) c.rhs = nullptr;
    int np = 0, nz = 0;
    for (int s = f0; s < f1; s++) front_forward<TPP, false, true, T, BLK, LPAN>(P, P.fronts[s], c, tid, false, T(0), eig_tol, np, nz);
    if (tid == 0) {
      int* slot = gcnt + 2 * ((long long)task * A.batch + b);
      slot[0] = np; slot[1] = nz;
    }
    return;
  }
  // ---- the climbers: newton_system! of one problem from the start (src/CaNNOLeS.jl:1019-1051), as newton_kernel runs it ----
  if (A.skip_done && A.success[b]) return;
  T* const a_rho_old = static_cast<T*>(A.rho_old);
  T* const a_rho = static_cast<T*>(A.rho);
  const int nt = A.ntasks_all;
  const int xpos = A.extra_pos ? A.extra_pos[b] : 0, xzer = A.extra_zer ? A.extra_zer[b] : 0;
  const T kdec = (T)A.params[2], kinc = (T)A.params[3], klarge = (T)A.params[4], rho0 = (T)A.params[5],
          rhomax = (T)A.params[6], rhomin = (T)A.params[7];
  T rho_old = a_rho_old[b];
  T rho = T(0), wrote = T(0);
  int nfact = 0;
  bool success = sub_factor_attempt<TPP, T, BLK>(P, tasks, nt, c, tid, false, T(0), eig_tol, xpos, xzer);
  nfact++;
  if (!success) {
    rho = rho_old == T(0) ? rho0 : max_of(rhomin, kdec * rho_old);
    wrote = rho;
    success = sub_factor_attempt<TPP, T, BLK>(P, tasks, nt, c, tid, true, rho, eig_tol, xpos, xzer);
    nfact++;
    while (!success && rho <= rhomax) {
      rho = rho_old == T(0) ? klarge * rho : kinc * rho;
      if (rho <= rhomax) {
        wrote = rho;
        success = sub_factor_attempt<TPP, T, BLK>(P, tasks, nt, c, tid, true, rho, eig_tol, xpos, xzer);
        nfact++;
      }
    }
    if (rho <= rhomax) rho_old = rho;
    T* vt = a_vals + (long long)b * P.vstride + P.rho_begin;
    for (int i = tid; i < P.nvar; i += TPP) vt[i] = wrote;
  }
  phase_fence<TPP>();
  if (success) sub_backward_all<TPP>(P, tasks, nt, c, tid, dout);
  if (tid == 0) {
    a_rho[b] = rho;
    a_rho_old[b] = rho_old;
    A.nfact[b] = nfact;
    A.success[b] = success ? 1 : 0;
  }
}

// Behind the last forward stage of a subtree call that factorises: one thread per problem sums the tasks' pivot counts with the
// condensed pivots' (extra_pos / extra_zer), applies the inertia test of src/solver_types.jl:96 and writes what newton_kernel writes
// for a first attempt — success, npos / nzero where the call asks for them (MODE_FACTOR), and for MODE_NEWTON rho = 0, nfact = 1 of the
// problems that succeeded, rho_old as it is (the climbers write everything of the others).  T: the element type of the handle's rho.
template <class T>
__global__ void __launch_bounds__(256) subtree_decide_kernel(const int* gcnt, int ntasks, int batch, int nvar, int mode, const int* extra_pos,
                                                            const int* extra_zer, int32_t* success, int64_t* npos, int64_t* nzero, T* rho,
                                                            int32_t* nfact) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  int np = extra_pos ? extra_pos[b] : 0, nz = extra_zer ? extra_zer[b] : 0;
  for (int k = 0; k < ntasks; k++) {
    const int* slot = gcnt + 2 * ((long long)k * batch + b);
    np += slot[0]; nz += slot[1];
  }
  const bool ok = np == nvar && nz == 0;
  success[b] = ok ? 1 : 0;
  if (npos) npos[b] = np;
  if (nzero) nzero[b] = nz;
  if (mode == MODE_NEWTON && ok) { rho[b] = T(0); nfact[b] = 1; }
}

// BLK: the blocked elimination of large fronts (PPB = 1; tuning general_blocked: double, TPP 256 or 1024, launch_newton; tuning
// float32_blocked: float, TPP 256, launch_newton_f32); MODE_SOLVE of such an instance reads A.success
// SUB: the subtree instances (PPB = 1, global work area, BLK either way; tuning general_subtrees: double, TPP 256 or 1024; tuning
// float32_subtrees: float, TPP 256; launch_newton_subtrees) — newton_subtrees above; they alone read A.tasks, A.task0, A.ntasks,
// A.ntasks_all, A.phase, A.gcnt and A.skip_done here.  Every other instance is the code it was.
// LPAN: the subtree instances whose factorising forward launch (A.phase 0, MODE_NEWTON / MODE_FACTOR) eliminates dependent pivot panels in
// LDS (tuning subtree_lds_panels; only with BLK and SUB, double or float, TPP 256 or 1024; launch_newton_subtrees, which sizes the dynamic
// LDS per stage); launched for such launches alone.  The default argument keeps every other instance the code it was.
template <int TPP, int PPB, bool LDSW, class T, bool BLK = false, bool SUB = false, bool LPAN = false>
__global__ void __launch_bounds__(TPP* PPB) newton_kernel(const DevPlan Pin, const LaunchArgs Ain) {
  static_assert(!LPAN || (BLK && SUB), "LDS pivot panels: blocked subtree instances only");
  if constexpr (SUB) {
    static_assert(PPB == 1 && !LDSW && TPP >= 256, "subtree instances: one problem per workgroup, work area in global scratch");
    DevPlan P = Pin;
    P.fronts = as_global(Pin.fronts); P.seg_ptr = as_global(Pin.seg_ptr); P.asm_pos = as_global(Pin.asm_pos);
    P.asm_src = as_global(Pin.asm_src); P.child_idx = as_global(Pin.child_idx); P.rel_idx = as_global(Pin.rel_idx);
    P.perm = as_global(Pin.perm);
    LaunchArgs A = Ain;
    A.vals = as_global(Ain.vals); A.rhs = as_global(Ain.rhs); A.d = as_global(Ain.d); A.L = as_global(Ain.L);
    A.scratch = as_global(Ain.scratch); A.rho_old = as_global(Ain.rho_old); A.rho = as_global(Ain.rho);
    A.nfact = as_global(Ain.nfact); A.success = as_global(Ain.success);
    A.extra_pos = as_global(Ain.extra_pos); A.extra_zer = as_global(Ain.extra_zer);
    extern __shared__ double smem_sub[];
    newton_subtrees<TPP, T, BLK, LPAN>(P, A, reinterpret_cast<T*>(smem_sub));
    return;
  }
  DevPlan P = Pin;
  P.fronts = as_global(Pin.fronts); P.seg_ptr = as_global(Pin.seg_ptr); P.asm_pos = as_global(Pin.asm_pos);
  P.asm_src = as_global(Pin.asm_src); P.child_idx = as_global(Pin.child_idx); P.rel_idx = as_global(Pin.rel_idx);
  P.perm = as_global(Pin.perm);
  LaunchArgs A = Ain;
  A.vals = as_global(Ain.vals); A.rhs = as_global(Ain.rhs); A.d = as_global(Ain.d); A.L = as_global(Ain.L);
  A.scratch = as_global(Ain.scratch); A.rho_old = as_global(Ain.rho_old); A.rho = as_global(Ain.rho);
  A.nfact = as_global(Ain.nfact); A.success = as_global(Ain.success); A.npos = as_global(Ain.npos); A.nzero = as_global(Ain.nzero);
  A.extra_pos = as_global(Ain.extra_pos); A.extra_zer = as_global(Ain.extra_zer);
  extern __shared__ double smem_raw[];
  T* smem = reinterpret_cast<T*>(smem_raw);
  // the element arrays of this launch, in the kernel's element type (LaunchArgs carries them untyped)
  T* const a_vals = static_cast<T*>(A.vals);
  const T* const a_rhs = static_cast<const T*>(A.rhs);
  T* const a_d = static_cast<T*>(A.d);
  T* const a_rho_old = static_cast<T*>(A.rho_old);
  T* const a_rho = static_cast<T*>(A.rho);
  const int gl = threadIdx.x / TPP;     // problem slot inside the workgroup
  const int tid = threadIdx.x % TPP;
  const int b = blockIdx.x * PPB + gl;
  if (b >= A.batch) return;             // whole owner group exits together (no block barrier when PPB > 1)
  ProblemCtx<T> c;
  c.vals = a_vals ? a_vals + (long long)b * P.vstride : nullptr;
  c.rhs = a_rhs ? a_rhs + (long long)b * P.rstride : nullptr;
  c.L = static_cast<T*>(A.L) + (long long)b * P.lsize;
  T* redbase = smem;                    // 16 elements for cross-wave sums (TPP > 64)
  c.red = redbase;
  c.W = LDSW ? (smem + 16 + (long long)gl * P.work_doubles) : (static_cast<T*>(A.scratch) + (long long)b * P.work_doubles);
  T* dout = a_d ? a_d + (long long)b * P.dstride : nullptr;
  const T eig_tol = (T)A.params[0];
  const int xpos = A.extra_pos ? A.extra_pos[b] : 0, xzer = A.extra_zer ? A.extra_zer[b] : 0;

  if (A.mode == MODE_SOLVE) {
    // a blocked handle keeps the success flags of its last factorisation (launch(), capi_run.cpp): a problem that holds no factor is
    // left alone, its rows of d untouched (one problem per workgroup: the whole workgroup leaves)
    if constexpr (BLK) {
      if (A.success && !A.success[b]) return;
    }
    int np = 0, nz = 0;
    for (int s = 0; s < P.nsuper; s++) front_forward<TPP, LDSW, false>(P, P.fronts[s], c, tid, false, T(0), eig_tol, np, nz);
    phase_fence<TPP>();
    for (int s = P.nsuper - 1; s >= 0; s--) front_backward<TPP, LDSW>(P, P.fronts[s], c, tid, dout);
    return;
  }
  if (A.mode == MODE_FACTOR) {
    int np, nz;
    ProblemCtx<T> cf = c; cf.rhs = nullptr;
    const bool ok = factor_attempt<TPP, LDSW, T, BLK>(P, cf, tid, false, T(0), eig_tol, np, nz, xpos, xzer);
    if (tid == 0) {
      A.success[b] = ok ? 1 : 0;
      if (A.npos) A.npos[b] = np;
      if (A.nzero) A.nzero[b] = nz;
    }
    return;
  }
  // ---- newton_system!: src/CaNNOLeS.jl:1019-1051 ----
  const T kdec = (T)A.params[2], kinc = (T)A.params[3], klarge = (T)A.params[4], rho0 = (T)A.params[5],
          rhomax = (T)A.params[6], rhomin = (T)A.params[7];
  T rho_old = a_rho_old[b];
  T rho = T(0), wrote = T(0);
  int nfact = 0, np, nz;
  bool success = factor_attempt<TPP, LDSW, T, BLK>(P, c, tid, false, T(0), eig_tol, np, nz, xpos, xzer);
  nfact++;
  if (!success) {
    rho = rho_old == T(0) ? rho0 : max_of(rhomin, kdec * rho_old);
    wrote = rho;
    success = factor_attempt<TPP, LDSW, T, BLK>(P, c, tid, true, rho, eig_tol, np, nz, xpos, xzer);
    nfact++;
    while (!success && rho <= rhomax) {
      rho = rho_old == T(0) ? klarge * rho : kinc * rho;
      if (rho <= rhomax) {
        wrote = rho;
        success = factor_attempt<TPP, LDSW, T, BLK>(P, c, tid, true, rho, eig_tol, np, nz, xpos, xzer);
        nfact++;
      }
    }
    if (rho <= rhomax) rho_old = rho;
    // the reference leaves the last rho tried in the rho slots of vals
    T* vt = a_vals + (long long)b * P.vstride + P.rho_begin;
    for (int i = tid; i < P.nvar; i += TPP) vt[i] = wrote;
  }
  phase_fence<TPP>();
  if (success)
    for (int s = P.nsuper - 1; s >= 0; s--) front_backward<TPP, LDSW>(P, P.fronts[s], c, tid, dout);
  if (tid == 0) {
    a_rho[b] = rho;
    a_rho_old[b] = rho_old;
    A.nfact[b] = nfact;
    A.success[b] = success ? 1 : 0;
  }
}

size_t max_lds_bytes() {
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) return 0;
  return (size_t)v;
}

template <int TPP, int PPB, bool LDSW, class T, bool BLK = false>
static hipError_t launch_t(const DevPlan& P, const KernelConfig& cfg, const LaunchArgs& a, hipStream_t stream) {
  auto kfn = newton_kernel<TPP, PPB, LDSW, T, BLK>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, lds_attr_cap((int)cfg.lds_bytes));
  if (e != hipSuccess) return e;
  const int grid = (a.batch + PPB - 1) / PPB;
  hipLaunchKernelGGL(kfn, dim3(grid), dim3(TPP * PPB), cfg.lds_bytes, stream, P, a);
  return hipGetLastError();
}

// the configurations with a blocked instance (tuning general_blocked; float32_blocked for f32): whole workgroups of several
// wavefronts on one problem; in float the 256-thread instances alone (the only 1024-thread float instances are subtree instances that
// tuning subtree_wide selects per stage, for factorising forward launches: no handle is configured with them)
bool newton_blocked_has(int tpp, int ppb, bool f32) { return ppb == 1 && (tpp == 256 || (tpp == 1024 && !f32)); }

hipError_t launch_newton(const DevPlan& P, const KernelConfig& cfg, const LaunchArgs& a, hipStream_t stream) {
  // (solve_ldl! runs the same sweeps on the factor a blocked launch left; given the flags of that factorisation in a.success it runs
  //  them in the blocked instance, which skips the problems that hold no factor)
  if (cfg.blocked && (a.mode != MODE_SOLVE || a.success)) {
#define CNL_CASE(T, W) \
  if (cfg.tpp == T && cfg.ppb == 1 && (cfg.lds_work != 0) == W) return launch_t<T, 1, W, double, true>(P, cfg, a, stream);
    CNL_CASE(256, true) CNL_CASE(1024, true) CNL_CASE(256, false) CNL_CASE(1024, false)
#undef CNL_CASE
    return hipErrorInvalidConfiguration;
  }
#define CNL_CASE(T, B, W) \
  if (cfg.tpp == T && cfg.ppb == B && (cfg.lds_work != 0) == W) return launch_t<T, B, W, double>(P, cfg, a, stream);
  CNL_CASE(64, 16, true) CNL_CASE(64, 8, true) CNL_CASE(64, 4, true) CNL_CASE(64, 2, true) CNL_CASE(64, 1, true)
  CNL_CASE(32, 32, true) CNL_CASE(32, 16, true) CNL_CASE(32, 8, true) CNL_CASE(32, 2, true)
  CNL_CASE(16, 64, true) CNL_CASE(16, 32, true) CNL_CASE(16, 16, true) CNL_CASE(16, 4, true)
  CNL_CASE(256, 1, true) CNL_CASE(1024, 1, true)
  CNL_CASE(64, 4, false) CNL_CASE(256, 1, false) CNL_CASE(1024, 1, false)
#undef CNL_CASE
  return hipErrorInvalidConfiguration;
}

// the configurations with subtree instances (tuning general_subtrees; float32_subtrees for f32): one problem per workgroup of 256 or
// 1024 threads, in float of 256 alone (1024-thread float subtree and ladder instances exist, but per stage only: tuning subtree_wide
// launches them for the factorising forward launch of a stage of a 256-thread handle, launch_newton_subtrees' `tpp` argument)
bool newton_subtrees_has(int tpp, int ppb, bool f32) { return ppb == 1 && (tpp == 256 || (tpp == 1024 && !f32)); }

// One launch of a subtree instance (newton_subtrees): a.phase 0 / 1 — the a.ntasks tasks of one stage from a.task0 on, one workgroup
// per (task, problem); a.phase 2 — the climbers, one workgroup per problem.  P.fronts is the task-region front table, P.work_doubles
// the elements of all regions of a problem, a.tasks the device task records; the work area is a.scratch whatever cfg.lds_work says.
// f32: the element arrays of a and the work area are float (a Float32 general handle, tuning float32_subtrees).
// shape (kernels.h: SubtreeStageShape), for a factorising forward launch alone (a.phase 0, not MODE_SOLVE): tpp 1024 on a
// 256-thread handle runs the stage on the 1024-thread instance (tuning subtree_wide: in float the only way to one), and lds_bytes above the
// 16 elements of psum runs the LPAN instance of a blocked handle with that much dynamic LDS (tuning subtree_lds_panels).
static bool subtree_shape_ok(const KernelConfig& cfg, const LaunchArgs& a, const SubtreeStageShape& shape, size_t red_bytes) {
  const bool plain = shape.tpp == cfg.tpp && shape.lds_bytes == (int)red_bytes;
  if (plain) return true;
  if (a.phase != 0 || a.mode == MODE_SOLVE) return false;
  if (shape.tpp != cfg.tpp && !(cfg.tpp == 256 && shape.tpp == 1024)) return false;
  if (shape.lds_bytes != (int)red_bytes && (!cfg.blocked || shape.lds_bytes < (int)red_bytes)) return false;
  return true;
}

template <class K, class... Args>
static hipError_t launch_subtree_instance(K kfn, long long grid, int tpp, size_t lds, hipStream_t stream, const Args&... args) {
  if (lds > 64 * 1024) {   // (LPAN areas of a large stage: the limit has to be raised, as launch_t does)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, lds_attr_cap((int)lds));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(tpp), lds, stream, args...);
  return hipGetLastError();
}

hipError_t launch_newton_subtrees(const DevPlan& P, const KernelConfig& cfg, const LaunchArgs& a, hipStream_t stream, bool f32,
                                  const SubtreeStageShape* shape) {
  if (!newton_subtrees_has(cfg.tpp, cfg.ppb, f32) || !a.tasks || !a.scratch || a.batch < 1) return hipErrorInvalidConfiguration;
  const long long grid = a.phase == 2 ? (long long)a.batch : (long long)a.batch * a.ntasks;
  if (grid < 1 || grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
  const size_t red = 16 * (f32 ? sizeof(float) : sizeof(double));   // the cross-wave sums of psum
  const SubtreeStageShape sh = shape ? *shape : SubtreeStageShape{cfg.tpp, (int32_t)red};
  if (!subtree_shape_ok(cfg, a, sh, red)) return hipErrorInvalidConfiguration;
  const size_t lds = (size_t)sh.lds_bytes;
  const bool lpan = lds > red;
#define CNL_CASE(T, E, B) \
  if (sh.tpp == T && (cfg.blocked != 0) == B && !lpan) return launch_subtree_instance(newton_kernel<T, 1, false, E, B, true>, grid, T, lds, stream, P, a);
#define CNL_LPAN(T, E) \
  if (sh.tpp == T && lpan) return launch_subtree_instance(newton_kernel<T, 1, false, E, true, true, true>, grid, T, lds, stream, P, a);
  if (f32) {
    CNL_CASE(256, float, false) CNL_CASE(256, float, true) CNL_CASE(1024, float, false) CNL_CASE(1024, float, true)
    CNL_LPAN(256, float) CNL_LPAN(1024, float)
    return hipErrorInvalidConfiguration;
  }
  CNL_CASE(256, double, false) CNL_CASE(256, double, true) CNL_CASE(1024, double, false) CNL_CASE(1024, double, true)
  CNL_LPAN(256, double) CNL_LPAN(1024, double)
#undef CNL_CASE
#undef CNL_LPAN
  return hipErrorInvalidConfiguration;
}

hipError_t launch_subtree_decide(const LaunchArgs& a, const int* gcnt, int ntasks, int nvar, hipStream_t stream, bool f32) {
  const dim3 grid((a.batch + 255) / 256), block(256);
  if (f32)
    hipLaunchKernelGGL(subtree_decide_kernel<float>, grid, block, 0, stream, gcnt, ntasks, a.batch, nvar, a.mode, a.extra_pos, a.extra_zer,
                       a.success, a.npos, a.nzero, static_cast<float*>(a.rho), a.nfact);
  else
    hipLaunchKernelGGL(subtree_decide_kernel<double>, grid, block, 0, stream, gcnt, ntasks, a.batch, nvar, a.mode, a.extra_pos, a.extra_zer,
                       a.success, a.npos, a.nzero, static_cast<double*>(a.rho), a.nfact);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The solve sweeps of a subtree handle in panels of PANEL_W pivots (tuning subtree_solve_panels).  Entries of their own,
// launched for the backward stages (A.phase 1) and the forward stages of solve_ldl! (A.phase 0, MODE_SOLVE) of handles with the key alone:
// front_forward, front_backward and every instance built from them are the code they were.  Grid, sub_enter_task and the early exit of a
// problem without a factor are newton_subtrees'.  The front's vector (X, resp. F) lives in dynamic LDS, the stored panel Lp is read in
// place (no copy to PB: the backward sweep only reads it, the forward one writes column 0 of a row and never reads it), and what other
// tasks read in later launches goes to the task region as ever: X of the front (backward), the 1 + nupd update entries at ubase (forward).
// LDS (kernels.h: subtree_solve_lds_elems): [vec: round4(F_s) | tri: PANEL_W rows of stride PANEL_W + 1 | pv: PANEL_W].
constexpr int SP_LD = PANEL_W + 1;
static_assert(PANEL_W * SP_LD == SOLVE_PANEL_TRI, "kernels.h sizes the triangle area");

__device__ __forceinline__ double fnma_of(double a, double b, double c) { return __builtin_fma(-a, b, c); }
__device__ __forceinline__ float fnma_of(float a, float b, float c) { return __builtin_fmaf(-a, b, c); }
// the value lane k of the wavefront holds, k uniform (a constant once the panel loops are unrolled): v_readlane, no LDS round trip
__device__ __forceinline__ float lane_value(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
__device__ __forceinline__ double lane_value(double v, int k) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

// Backward sweep of one front, x_i = z_i - sum_{1 <= j < i} l_ij x_j, panels [p0, p1) of pivot rows ascending, the last one short.
// Outer part: s_r = sum_{1 <= j < p0} l_rj x_j of the panel's rows at once, row r on the TPP / PANEL_W lanes tid / G, lanes striding over j
// (contiguous runs of Lp), reduced by shuffles inside the lane group; t_r = z_r - s_r into pv; the panel's triangle into tri meanwhile.
// Inner part: the first wavefront, lane r holding t_r: x_k is broadcast in steps k = 0 .. 14 and the lanes r > k subtract l_rk x_k.
// Two workgroup barriers per panel.  The order of summation is a function of (TPP, front) alone.
template <int TPP, class T>
__device__ __forceinline__ void front_backward_panels(const DevPlan& P, const FrontHdr& H, const ProblemCtx<T>& c, int tid, T* dout, T* Xs,
                                                      T* tri, T* pv) {
  constexpr int G = TPP / PANEL_W;   // lanes of a row: 16 or 64, never across a wavefront
  const int nupd = H.nupd, npiv = H.npiv;
  const int f = 1 + nupd + npiv;
  const int tu = tri_i(1 + nupd);
  T* X = c.W + H.xoff;
  const T* Lp = c.L + ((long long)H.lptr_lo | ((long long)H.lptr_hi << 31));
  if (H.parent >= 0) {
    // (the first child's X lies on its parent's: everything is read before anything is written)
    const T* Xp = c.W + P.fronts[H.parent].xoff;
    const int* rel = P.rel_idx + H.rel_begin;
    for (int j = 1 + tid; j <= nupd; j += TPP) Xs[j] = Xp[rel[j]];
    __syncthreads();
    for (int j = 1 + tid; j <= nupd; j += TPP) X[j] = Xs[j];
  }
  const int r = tid / G, l = tid % G;
  const int sr = (tid >> 4) & (PANEL_W - 1), sk = tid & (PANEL_W - 1);   // the triangle's element of this thread (tid < 256)
  for (int p0 = nupd + 1; p0 < f; p0 += PANEL_W) {
    const int kp = f - p0 < PANEL_W ? f - p0 : PANEL_W;
    const T* rowr = Lp + (tri_i(p0 + (r < kp ? r : 0)) - tu);
    T part = T(0);
    if (r < kp) {
#pragma unroll 4
      for (int j = 1 + l; j < p0; j += G) part += rowr[j] * Xs[j];
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, G);
    if (r < kp && l == 0) pv[r] = rowr[0] - part;
    if (tid < PANEL_W * PANEL_W && sr < kp && sk < sr) tri[sr * SP_LD + sk] = Lp[tri_i(p0 + sr) - tu + p0 + sk];
    __syncthreads();
    if (tid < 64) {
      T t = tid < kp ? pv[tid] : T(0);
#pragma unroll
      for (int k = 0; k < PANEL_W - 1; k++) {
        const T xk = lane_value(t, k);
        if (tid > k && tid < kp) t -= tri[tid * SP_LD + k] * xk;
      }
      if (tid < kp) {
        const int i = p0 + tid;
        Xs[i] = t;
        X[i] = t;
        dout[P.perm[H.first_piv + (f - 1 - i)]] = -t;
      }
    }
    __syncthreads();
  }
}

// Forward substitution of one front with the stored panel, panels [p0, p1) of pivot rows descending, the last one short.  Per pivot i
// descending the unpanelled loop (front_forward, WITH_K = false) does w = F[i]; F[j] -= l_ij w for 1 <= j < ulim; z_i = w / d_i.  Here the
// first wavefront runs the panel's pivots on F[p0 .. p1) (lane r holding F[p0 + r]), leaves the w_i in pv and stores the z_i; then every
// thread applies the panel's pivots, in the same order, to the elements j < p0 it owns.  Every element receives the operations of the
// unpanelled loop in their order, ulim honoured term by term, each one fused multiply-add as there: bit-equal.
template <int TPP, class T>
__device__ __forceinline__ void front_forward_solve_panels(const DevPlan& P, const FrontHdr& H, const ProblemCtx<T>& c, int tid, T* Fs, T* tri,
                                                           T* pv) {
  const int nupd = H.nupd, npiv = H.npiv;
  const int f = 1 + nupd + npiv;
  const int tu = tri_i(1 + nupd);
  T* Lp = c.L + ((long long)H.lptr_lo | ((long long)H.lptr_hi << 31));
  const int idep = f - H.indep;
  const int sk = (tid >> 4) & (PANEL_W - 1), sr = tid & (PANEL_W - 1);   // the triangle's element of this thread (tid < 256)
  // the triangle of panel [p0, p0 + kp), diagonal included: tri[k][r] = l_{p0 + k, p0 + r}, r <= k
  auto stage_tri = [&](int p0, int kp) {
    if (tid < PANEL_W * PANEL_W && sk < kp && sr <= sk) tri[sk * SP_LD + sr] = Lp[tri_i(p0 + sk) - tu + p0 + sr];
  };
  for (int t = tid; t < f; t += TPP) {
    T v = T(0);
    if (t > nupd) v = c.rhs[P.perm[H.first_piv + (f - 1 - t)]];
    Fs[t] = v;
  }
  {
    const int p0 = f - PANEL_W > nupd + 1 ? f - PANEL_W : nupd + 1;
    stage_tri(p0, f - p0);
  }
  __syncthreads();
  for (int ci = H.child_begin; ci < H.child_end; ci++) {
    const FrontHdr& C = P.fronts[P.child_idx[ci]];
    const T* U = c.W + C.ubase;
    const int* rel = P.rel_idx + C.rel_begin;
    for (int a = 1 + tid; a <= C.nupd; a += TPP) Fs[rel[a]] += U[a];
    __syncthreads();
  }
  for (int p1 = f; p1 > nupd + 1;) {
    const int p0 = p1 - PANEL_W > nupd + 1 ? p1 - PANEL_W : nupd + 1;
    const int kp = p1 - p0;
    if (tid < 64) {
      T v = tid < kp ? Fs[p0 + tid] : T(0);
#pragma unroll
      for (int k = PANEL_W - 1; k >= 0; k--) {
        if (k < kp) {   // (uniform)
          const int i = p0 + k;
          const int ulim = i >= idep ? idep : i;
          const T w = lane_value(v, k);
          if (tid < k && p0 + tid < ulim) v = fnma_of(tri[k * SP_LD + tid], w, v);
        }
      }
      // (lane k is not touched after step k: what it holds is w_k; the 16 quotients at once, off the chain)
      if (tid < kp) {
        pv[tid] = v;
        Lp[tri_i(p0 + tid) - tu] = v / tri[tid * SP_LD + tid];
      }
    }
    __syncthreads();
    p1 = p0;
    // the next panel's triangle is fetched while the outer part runs (stored behind it: the first wavefront is done with tri)
    const int q0 = p1 - PANEL_W > nupd + 1 ? p1 - PANEL_W : nupd + 1;
    const bool more = p1 > nupd + 1 && tid < PANEL_W * PANEL_W && sk < p1 - q0 && sr <= sk;
    T tnext = T(0);
    if (more) tnext = Lp[tri_i(q0 + sk) - tu + q0 + sr];
    for (int j = 1 + tid; j < p0; j += TPP) {
      // the panel's 16 rows at column j: independent loads, all in flight before the chain of multiply-adds starts
      T lv[PANEL_W];
#pragma unroll
      for (int k = 0; k < PANEL_W; k++) {
        const int i = p0 + k;
        lv[k] = (k < kp && (i < idep || j < idep)) ? Lp[tri_i(i) - tu + j] : T(0);
      }
      T v = Fs[j];
#pragma unroll
      for (int k = PANEL_W - 1; k >= 0; k--) {
        const int i = p0 + k;
        if (k < kp && (i < idep || j < idep)) v = fnma_of(lv[k], pv[k], v);   // (j < ulim, with j < p0 <= i)
      }
      Fs[j] = v;
    }
    if (more) tri[sk * SP_LD + sr] = tnext;
    __syncthreads();
  }
  // the update vector for the parent, in the task region where the unpanelled sweep leaves it
  T* U = c.W + H.ubase;
  for (int t = tid; t <= nupd; t += TPP) U[t] = Fs[t];
  __syncthreads();
}

template <int TPP, class T, bool BACKWARD>
__global__ void __launch_bounds__(TPP) subtree_solve_kernel(const DevPlan Pin, const LaunchArgs Ain, const int vec_elems) {
  static_assert(TPP >= 256 && TPP % 64 == 0, "subtree instances: one problem per workgroup of 256 or 1024 threads");
  DevPlan P = Pin;
  P.fronts = as_global(Pin.fronts); P.child_idx = as_global(Pin.child_idx); P.rel_idx = as_global(Pin.rel_idx);
  P.perm = as_global(Pin.perm);
  LaunchArgs A = Ain;
  A.rhs = as_global(Ain.rhs); A.d = as_global(Ain.d); A.L = as_global(Ain.L);
  A.scratch = as_global(Ain.scratch); A.success = as_global(Ain.success);
  const int32_t* const tasks = as_global(const_cast<int32_t*>(A.tasks));
  extern __shared__ __attribute__((aligned(16))) double smem_solve[];
  T* const vec = reinterpret_cast<T*>(smem_solve);
  T* const tri = vec + vec_elems;
  T* const pv = tri + SOLVE_PANEL_TRI;
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x % (unsigned)A.batch);
  const int task = A.task0 + (int)(blockIdx.x / (unsigned)A.batch);
  if (task >= A.task0 + A.ntasks) return;
  if (A.success && !A.success[b]) return;   // a problem without a factor: the whole workgroup leaves, before any barrier
  ProblemCtx<T> c;
  c.vals = nullptr;
  c.rhs = A.rhs ? static_cast<const T*>(A.rhs) + (long long)b * P.rstride : nullptr;
  c.L = static_cast<T*>(A.L) + (long long)b * P.lsize;
  c.red = nullptr;
  c.W = static_cast<T*>(A.scratch) + (long long)b * P.work_doubles;
  int f0, f1;
  sub_enter_task(P, tasks, task, f0, f1);
  if constexpr (BACKWARD) {
    T* const dout = static_cast<T*>(A.d) + (long long)b * P.dstride;
    for (int s = f1 - 1; s >= f0; s--) front_backward_panels<TPP>(P, P.fronts[s], c, tid, dout, vec, tri, pv);
  } else {
    for (int s = f0; s < f1; s++) front_forward_solve_panels<TPP>(P, P.fronts[s], c, tid, vec, tri, pv);
  }
}

// One launch of a stage's panelled sweep: a.phase 1 — backward; a.phase 0 with MODE_SOLVE — the forward substitution of solve_ldl!.
// fmax_s = F_s of the stage (every front of the stage has at most that many rows), lds_bytes = subtree_solve_lds_elems(F_s) elements.
hipError_t launch_subtree_solve(const DevPlan& P, const KernelConfig& cfg, const LaunchArgs& a, hipStream_t stream, bool f32, int fmax_s,
                                size_t lds_bytes) {
  if (!newton_subtrees_has(cfg.tpp, cfg.ppb, f32) || !a.tasks || !a.scratch || !a.L || a.batch < 1) return hipErrorInvalidConfiguration;
  if ((a.phase == 0 && !a.rhs) || (a.phase == 1 && !a.d)) return hipErrorInvalidConfiguration;
  const bool backward = a.phase == 1;
  if (!backward && !(a.phase == 0 && a.mode == MODE_SOLVE)) return hipErrorInvalidConfiguration;
  if (backward && !a.success) return hipErrorInvalidConfiguration;
  const long long grid = (long long)a.batch * a.ntasks;
  if (grid < 1 || grid > 0x7fffffffLL || fmax_s < 1) return hipErrorInvalidConfiguration;
  const int vec_elems = (int)subtree_solve_vec_elems(fmax_s);
  if (lds_bytes != (size_t)subtree_solve_lds_elems(fmax_s) * (f32 ? sizeof(float) : sizeof(double))) return hipErrorInvalidConfiguration;
#define CNL_CASE(T, E) \
  if (cfg.tpp == T) { \
    if (backward) return launch_subtree_instance(subtree_solve_kernel<T, E, true>, grid, T, lds_bytes, stream, P, a, vec_elems); \
    return launch_subtree_instance(subtree_solve_kernel<T, E, false>, grid, T, lds_bytes, stream, P, a, vec_elems); \
  }
  if (f32) {
    CNL_CASE(256, float)
    return hipErrorInvalidConfiguration;
  }
  CNL_CASE(256, double) CNL_CASE(1024, double)
#undef CNL_CASE
  return hipErrorInvalidConfiguration;
}

// ---------------------------------------------------------------------------
// The rho ladder of a subtree handle, stage by stage (tuning subtree_ladder = R > 0).  Entries of their own, launched
// by handles with R > 0 alone: newton_kernel's instances and subtree_decide_kernel are the code they were.  Per-problem state (kernels.h:
// LadderState): done[b] — 0 climbing, 1 succeeded on the first attempt, 2 finished inside the rungs (success, or the ladder exhausted) —
// and lrho[b][2] = {the rho of the problem's next rung, the last rho tried}.  The first decide writes done and rho_1 of every problem, so
// nothing is zeroed per call; every later kernel reads done before anything else.  As everywhere in the subtree execution the order of
// the launches on the stream is the only dependency: nothing waits, no counter, no atomic.
//
// subtree_ladder_kernel, CLIMB = false (A.phase 0): forward of the tasks of one stage at the problem's rho_k (rho_override), workgroup = (task, problem);
// a workgroup whose problem is done leaves before any barrier.  CLIMB = true (A.phase 2): the climbers, workgroup = problem, for a problem still
// climbing after R rungs: the reference's while loop (src/CaNNOLeS.jl:1033-1043) entered at rho_{R+1}, which the decide of rung R
// formed and found <= rhomax, with nfact = R + 1 behind it; the backward sweep on success; all outputs.
// LPAN (only with BLK, never with CLIMB): the rung instances with dependent pivot panels in LDS, as newton_kernel's.
template <int TPP, class T, bool BLK, bool CLIMB, bool LPAN = false>
__global__ void __launch_bounds__(TPP) subtree_ladder_kernel(const DevPlan Pin, const LaunchArgs Ain, const LadderState Sin) {
  static_assert(TPP >= 256, "subtree instances: one problem per workgroup of 256 or 1024 threads");
  static_assert(!LPAN || (BLK && !CLIMB), "LDS pivot panels: the blocked rung instances only");
  DevPlan P = Pin;
  P.fronts = as_global(Pin.fronts); P.seg_ptr = as_global(Pin.seg_ptr); P.asm_pos = as_global(Pin.asm_pos);
  P.asm_src = as_global(Pin.asm_src); P.child_idx = as_global(Pin.child_idx); P.rel_idx = as_global(Pin.rel_idx);
  P.perm = as_global(Pin.perm);
  LaunchArgs A = Ain;
  A.vals = as_global(Ain.vals); A.rhs = as_global(Ain.rhs); A.d = as_global(Ain.d); A.L = as_global(Ain.L);
  A.scratch = as_global(Ain.scratch); A.rho_old = as_global(Ain.rho_old); A.rho = as_global(Ain.rho);
  A.nfact = as_global(Ain.nfact); A.success = as_global(Ain.success);
  A.extra_pos = as_global(Ain.extra_pos); A.extra_zer = as_global(Ain.extra_zer);
  const int32_t* const done = as_global(Sin.done);
  const T* const lrho = as_global(static_cast<T*>(Sin.rho));
  extern __shared__ double smem_lad[];
  T* const a_vals = static_cast<T*>(A.vals);
  const T* const a_rhs = static_cast<const T*>(A.rhs);
  T* const a_d = static_cast<T*>(A.d);
  const int32_t* const tasks = as_global(const_cast<int32_t*>(A.tasks));
  const int tid = threadIdx.x;
  constexpr bool climb = CLIMB;   // (instances of their own: the rungs keep the registers of a forward pass)
  const int b = climb ? (int)blockIdx.x : (int)(blockIdx.x % (unsigned)A.batch);
  const int task = climb ? 0 : A.task0 + (int)(blockIdx.x / (unsigned)A.batch);
  if (b >= A.batch || task >= A.task0 + A.ntasks) return;
  if (done[b]) return;   // uniform per workgroup, before any barrier
  ProblemCtx<T> c;
  c.vals = a_vals + (long long)b * P.vstride;
  c.rhs = a_rhs ? a_rhs + (long long)b * P.rstride : nullptr;
  c.L = static_cast<T*>(A.L) + (long long)b * P.lsize;
  c.red = reinterpret_cast<T*>(smem_lad);
  c.W = static_cast<T*>(A.scratch) + (long long)b * P.work_doubles;
  const T eig_tol = (T)A.params[0];
  const T rho_next = lrho[2 * (long long)b];
  if constexpr (!climb) {
    int f0, f1;
    sub_enter_task(P, tasks, task, f0, f1);
    int np = 0, nz = 0;
    for (int s = f0; s < f1; s++) front_forward<TPP, false, true, T, BLK, LPAN>(P, P.fronts[s], c, tid, true, rho_next, eig_tol, np, nz);
    if (tid == 0) {
      int* slot = as_global(A.gcnt) + 2 * ((long long)task * A.batch + b);
      slot[0] = np; slot[1] = nz;
    }
  } else {
    T* dout = a_d ? a_d + (long long)b * P.dstride : nullptr;
    T* const a_rho_old = static_cast<T*>(A.rho_old);
    T* const a_rho = static_cast<T*>(A.rho);
    const int nt = A.ntasks_all;
    const int xpos = A.extra_pos ? A.extra_pos[b] : 0, xzer = A.extra_zer ? A.extra_zer[b] : 0;
    const T kinc = (T)A.params[3], klarge = (T)A.params[4], rhomax = (T)A.params[6];
    T rho_old = a_rho_old[b];
    T rho = rho_next, wrote = rho_next;
    int nfact = Sin.rungs + 1;
    bool success = sub_factor_attempt<TPP, T, BLK>(P, tasks, nt, c, tid, true, rho, eig_tol, xpos, xzer);
    nfact++;
    while (!success && rho <= rhomax) {
      rho = rho_old == T(0) ? klarge * rho : kinc * rho;
      if (rho <= rhomax) {
        wrote = rho;
        success = sub_factor_attempt<TPP, T, BLK>(P, tasks, nt, c, tid, true, rho, eig_tol, xpos, xzer);
        nfact++;
      }
    }
    if (rho <= rhomax) rho_old = rho;
    T* vt = a_vals + (long long)b * P.vstride + P.rho_begin;
    for (int i = tid; i < P.nvar; i += TPP) vt[i] = wrote;
    phase_fence<TPP>();
    if (success) sub_backward_all<TPP>(P, tasks, nt, c, tid, dout);
    if (tid == 0) {
      a_rho[b] = rho;
      a_rho_old[b] = rho_old;
      A.nfact[b] = nfact;
      A.success[b] = success ? 1 : 0;
    }
  }
}

// The first decide of a newton_system with R > 0, in the place of subtree_decide_kernel: what that kernel writes for MODE_NEWTON, and the
// ladder state of every problem — done = 1 for a success; for a failure done = 0 and rho_1 = rho_old == 0 ? rho0 : max(rhomin, kdec rho_old)
// (src/CaNNOLeS.jl:1029), tried whatever its relation to rhomax.
template <class T>
__global__ void __launch_bounds__(256) subtree_ladder_first_kernel(const int* gcnt, int ntasks, int batch, int nvar, const int* extra_pos,
                                                                  const int* extra_zer, int32_t* success, T* rho, const T* rho_old, int32_t* nfact,
                                                                  int32_t* done, T* lrho, T kdec, T rho0, T rhomin) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  int np = extra_pos ? extra_pos[b] : 0, nz = extra_zer ? extra_zer[b] : 0;
  for (int k = 0; k < ntasks; k++) {
    const int* slot = gcnt + 2 * ((long long)k * batch + b);
    np += slot[0]; nz += slot[1];
  }
  const bool ok = np == nvar && nz == 0;
  success[b] = ok ? 1 : 0;
  done[b] = ok ? 1 : 0;
  if (ok) { rho[b] = T(0); nfact[b] = 1; return; }
  const T ro = rho_old[b];
  lrho[2 * (long long)b] = ro == T(0) ? rho0 : max_of(rhomin, kdec * ro);
}

// Behind the stages of rung k: one thread per problem that is not done sums the slots, applies the inertia test and moves the problem
// along the ladder as the reference's loop does (src/CaNNOLeS.jl:1031-1047; rho_old[b] is still the call's incoming value, since only
// a problem that is done has had it written).  nfact = k + 1.  Success: rho = rho_k, rho_old = rho_k only if rho_k <= rhomax, done.
// Failure: rho_k > rhomax (rung 1 alone can be: the loop never runs) — done with rho = rho_k; else rho_{k+1} = klarge rho_k or kinc rho_k,
// and rho_{k+1} > rhomax — the ladder is exhausted — done with rho = rho_{k+1}, which is never tried; rho_old unchanged in both.
// The comparisons are written as the loop's own (rho <= rhomax), so that a NaN leaves the ladder where the sequential kernel leaves it.
template <class T>
__global__ void __launch_bounds__(256) subtree_rung_decide_kernel(const int* gcnt, int ntasks, int batch, int nvar, int k, const int* extra_pos,
                                                                 const int* extra_zer, int32_t* success, T* rho, T* rho_old, int32_t* nfact,
                                                                 int32_t* done, T* lrho, T kinc, T klarge, T rhomax) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  if (done[b]) return;
  int np = extra_pos ? extra_pos[b] : 0, nz = extra_zer ? extra_zer[b] : 0;
  for (int t = 0; t < ntasks; t++) {
    const int* slot = gcnt + 2 * ((long long)t * batch + b);
    np += slot[0]; nz += slot[1];
  }
  const bool ok = np == nvar && nz == 0;
  const T r = lrho[2 * (long long)b];
  nfact[b] = k + 1;
  lrho[2 * (long long)b + 1] = r;
  if (ok) {
    success[b] = 1;
    rho[b] = r;
    if (r <= rhomax) rho_old[b] = r;
    done[b] = 2;
    return;
  }
  if (!(r <= rhomax)) { rho[b] = r; done[b] = 2; return; }
  const T nx = rho_old[b] == T(0) ? klarge * r : kinc * r;
  if (!(nx <= rhomax)) { rho[b] = nx; done[b] = 2; return; }
  lrho[2 * (long long)b] = nx;
}

// The commit behind the backward stages: one workgroup per problem; a problem that failed the first attempt and finished inside the
// rungs (done == 2) gets the last rho tried in the nvar rho slots of its vals, as the reference leaves it; every other workgroup leaves.
template <class T>
__global__ void __launch_bounds__(256) subtree_ladder_commit_kernel(T* vals, long long vstride, int rho_begin, int nvar, int batch,
                                                                   const int32_t* done, const T* lrho) {
  const int b = blockIdx.x;
  if (b >= batch || done[b] != 2) return;
  const T wrote = lrho[2 * (long long)b + 1];
  T* vt = vals + (long long)b * vstride + rho_begin;
  for (int i = threadIdx.x; i < nvar; i += 256) vt[i] = wrote;
}

// shape: as launch_newton_subtrees' — the rungs (a.phase 0) are factorising forward launches, the climbers (a.phase 2) keep the handle's shape
hipError_t launch_subtree_ladder(const DevPlan& P, const KernelConfig& cfg, const LaunchArgs& a, const LadderState& st, hipStream_t stream, bool f32,
                                 const SubtreeStageShape* shape) {
  if (!newton_subtrees_has(cfg.tpp, cfg.ppb, f32) || !a.tasks || !a.scratch || !a.vals || !st.done || !st.rho || a.batch < 1 || a.mode != MODE_NEWTON ||
      (a.phase != 0 && a.phase != 2))
    return hipErrorInvalidConfiguration;
  const long long grid = a.phase == 2 ? (long long)a.batch : (long long)a.batch * a.ntasks;
  if (grid < 1 || grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
  const size_t red = 16 * (f32 ? sizeof(float) : sizeof(double));   // the cross-wave sums of psum
  const SubtreeStageShape sh = shape ? *shape : SubtreeStageShape{cfg.tpp, (int32_t)red};
  if (!subtree_shape_ok(cfg, a, sh, red)) return hipErrorInvalidConfiguration;
  const size_t lds = (size_t)sh.lds_bytes;
  const bool lpan = lds > red;
#define CNL_CASE(T, E, B) \
  if (sh.tpp == T && (cfg.blocked != 0) == B && !lpan) { \
    if (a.phase == 2) return launch_subtree_instance(subtree_ladder_kernel<T, E, B, true>, grid, T, lds, stream, P, a, st); \
    return launch_subtree_instance(subtree_ladder_kernel<T, E, B, false>, grid, T, lds, stream, P, a, st); \
  }
#define CNL_LPAN(T, E) \
  if (sh.tpp == T && lpan) return launch_subtree_instance(subtree_ladder_kernel<T, E, true, false, true>, grid, T, lds, stream, P, a, st);
  if (f32) {
    CNL_CASE(256, float, false) CNL_CASE(256, float, true)
    if (a.phase == 0) {   // (no 1024-thread float climbers: a stage alone is ever wide)
      if (sh.tpp == 1024 && !lpan) {
        if (cfg.blocked) return launch_subtree_instance(subtree_ladder_kernel<1024, float, true, false>, grid, 1024, lds, stream, P, a, st);
        return launch_subtree_instance(subtree_ladder_kernel<1024, float, false, false>, grid, 1024, lds, stream, P, a, st);
      }
      CNL_LPAN(256, float) CNL_LPAN(1024, float)
    }
    return hipErrorInvalidConfiguration;
  }
  CNL_CASE(256, double, false) CNL_CASE(256, double, true) CNL_CASE(1024, double, false) CNL_CASE(1024, double, true)
  CNL_LPAN(256, double) CNL_LPAN(1024, double)
#undef CNL_CASE
#undef CNL_LPAN
  return hipErrorInvalidConfiguration;
}

hipError_t launch_subtree_ladder_first(const LaunchArgs& a, const LadderState& st, const int* gcnt, int ntasks, int nvar, hipStream_t stream, bool f32) {
  const dim3 grid((a.batch + 255) / 256), block(256);
  if (f32)
    hipLaunchKernelGGL(subtree_ladder_first_kernel<float>, grid, block, 0, stream, gcnt, ntasks, a.batch, nvar, a.extra_pos, a.extra_zer, a.success,
                       static_cast<float*>(a.rho), static_cast<const float*>(a.rho_old), a.nfact, st.done, static_cast<float*>(st.rho),
                       (float)a.params[2], (float)a.params[5], (float)a.params[7]);
  else
    hipLaunchKernelGGL(subtree_ladder_first_kernel<double>, grid, block, 0, stream, gcnt, ntasks, a.batch, nvar, a.extra_pos, a.extra_zer, a.success,
                       static_cast<double*>(a.rho), static_cast<const double*>(a.rho_old), a.nfact, st.done, static_cast<double*>(st.rho),
                       a.params[2], a.params[5], a.params[7]);
  return hipGetLastError();
}

hipError_t launch_subtree_rung_decide(const LaunchArgs& a, const LadderState& st, int k, const int* gcnt, int ntasks, int nvar, hipStream_t stream, bool f32) {
  const dim3 grid((a.batch + 255) / 256), block(256);
  if (f32)
    hipLaunchKernelGGL(subtree_rung_decide_kernel<float>, grid, block, 0, stream, gcnt, ntasks, a.batch, nvar, k, a.extra_pos, a.extra_zer, a.success,
                       static_cast<float*>(a.rho), static_cast<float*>(a.rho_old), a.nfact, st.done, static_cast<float*>(st.rho),
                       (float)a.params[3], (float)a.params[4], (float)a.params[6]);
  else
    hipLaunchKernelGGL(subtree_rung_decide_kernel<double>, grid, block, 0, stream, gcnt, ntasks, a.batch, nvar, k, a.extra_pos, a.extra_zer, a.success,
                       static_cast<double*>(a.rho), static_cast<double*>(a.rho_old), a.nfact, st.done, static_cast<double*>(st.rho),
                       a.params[3], a.params[4], a.params[6]);
  return hipGetLastError();
}

hipError_t launch_subtree_ladder_commit(const DevPlan& P, const LaunchArgs& a, const LadderState& st, hipStream_t stream, bool f32) {
  if (!a.vals || a.batch < 1) return hipErrorInvalidConfiguration;
  const dim3 grid(a.batch), block(256);
  if (f32)
    hipLaunchKernelGGL(subtree_ladder_commit_kernel<float>, grid, block, 0, stream, static_cast<float*>(a.vals), (long long)P.vstride, (int)P.rho_begin,
                       (int)P.nvar, a.batch, st.done, static_cast<const float*>(st.rho));
  else
    hipLaunchKernelGGL(subtree_ladder_commit_kernel<double>, grid, block, 0, stream, static_cast<double*>(a.vals), (long long)P.vstride, (int)P.rho_begin,
                       (int)P.nvar, a.batch, st.done, static_cast<const double*>(st.rho));
  return hipGetLastError();
}

// The Float32 instances: the configurations choose_config picks for a Float32 handle (capi_handle.cpp) plus one per thread count and
// work-area placement, each launched by tests/test_float32_general_gpu.py.  Every other configuration of the list above is
// Float64-only.
#define CNL_F32_CASES(X) \
  X(64, 1, true) X(64, 4, true) X(32, 2, true) X(16, 4, true) X(256, 1, true) \
  X(64, 4, false) X(256, 1, false)

bool newton_f32_has(int tpp, int ppb, bool lds_work) {
#define CNL_CASE(T, B, W) if (tpp == T && ppb == B && lds_work == W) return true;
  CNL_F32_CASES(CNL_CASE)
#undef CNL_CASE
  return false;
}

hipError_t launch_newton_f32(const DevPlan& P, const KernelConfig& cfg, const LaunchArgs& a, hipStream_t stream) {
  // (tuning float32_blocked: the rule of launch_newton — Newton and factorise launches, and the solve sweeps where the flags of the
  //  last factorisation come with them)
  if (cfg.blocked && (a.mode != MODE_SOLVE || a.success)) {
    if (cfg.tpp == 256 && cfg.ppb == 1)
      return cfg.lds_work != 0 ? launch_t<256, 1, true, float, true>(P, cfg, a, stream) : launch_t<256, 1, false, float, true>(P, cfg, a, stream);
    return hipErrorInvalidConfiguration;
  }
#define CNL_CASE(T, B, W) \
  if (cfg.tpp == T && cfg.ppb == B && (cfg.lds_work != 0) == W) return launch_t<T, B, W, float>(P, cfg, a, stream);
  CNL_F32_CASES(CNL_CASE)
#undef CNL_CASE
  return hipErrorInvalidConfiguration;
}

}  // namespace cnl
