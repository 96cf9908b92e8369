// dense_f32.hip — the dense backend (dense.h, dense.hip) in float for gfx950: Float32 handles with tuning float32_dense.
//
// The float form of every kernel dense_run enqueues for the residual-block form, kept in a file of its own so that the Float64
// kernels of dense.hip compile to exactly the code they compiled to before.  Same launch sequence, same tile lists, same work
// partition (dense_impl.h builds them once for both element types), same producer / consumer protocol inside the panel kernels:
//
//   dnf_gather    J and w = -1/d_r out of the caller's COO values (+ inertia of the residual pivots, compared in float)
//   dnf_syrk2     J' W J by v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate), lower macro tiles, K split into slabs
//   dnf_assemble  S0 = slabs + H entries (COO order), S = S0 + rho slots
//   per tile column k:  dnf_panel2 / dnf_panel  +  dnf_update (rank-64 update on the f32 matrix cores)
//   dnf_decide / dnf_ladder   inertia rule and rho ladder, decided on the device
//   dnf_yrhs, dnf_gt_part, dnf_g_part, dnf_resid_part, dnf_xfinal, dnf_jx, dnf_out   d = -K^-1 rhs through S^-1 = G D G' and one
//                 step of iterative refinement against S0 (all in float)
//
// ... and of the kernels only the GENERAL form enqueues (dense_run_general: an arbitrary condensed system as one dense matrix,
// Float32 handles with tuning float32_general_dense; m == 0 in DnDevF marks it):
//   dnf_set_counts, dn_zero16, dnf_scatter_general, dnf_shift   in place of gather / J'WJ / assemble: the inertia counts of the
//                 condensed pivots handed in, S0 zeroed and scattered out of the float condensed buffer, S = S0 + the rho slots
//                 behind it.  (S0 is zeroed by a kernel, not by hipMemsetAsync: the call sequence is captured as a graph, and a
//                 replayed memset node was seen to fill S0 with something other than zeros — DESIGN section 9.6.)
//   dnf_yrhs_general, dnf_out_general                in place of yrhs / jx / out: y is the condensed right-hand side, d2 = -x
// Everything between them is the residual-block form's: none of the panel, update, ladder, decide and solve kernels reads n, m, p,
// J or w — they see S0, S, G, rsh, the counters and the tile lists, which the general form fills the same way.
//
// What differs from the double form, and what does not:
//   * Tile order stays 64, the macro tile of J'WJ stays 128, row chunks stay 16, dnf_yrhs stages 2048 rows at a time, the ladder
//     takes 7 row tiles per pass and dnf_panel 3 row tiles per workgroup: the float kernels have the edges of the double kernels.
//   * Wavefronts per tile are unchanged (dnf_panel2: 4 + 4 column blocks of 16, lane = row; dnf_panel: 1 + 3), so every published
//     count of the panel protocol (pub[0]: pivots of the diagonal tile, J + 1 after pivot J; pub[1]: J0 + 4 after four pivots of a
//     row block; consumers wait for J + 8 resp. J0 + 4) is the double form's.
//   * Matrix-core results: A / B lane maps of v_mfma_f32_16x16x4_f32 are those of the f64 instruction (lane l: row or column l & 15,
//     k = l >> 4), the C / D map is NOT: register `reg` of lane l is row 4 (l >> 4) + reg (f64: (l >> 4) + 4 reg), column l & 15.
//   * LDS, 64 banks of 4 bytes.  J'WJ operands: [column][row] with a stride of LDK = 20 floats.  The 16 x 4 operand fetch reads
//     (c0 + li) * 20 + 4 s + lg for li < 16, lg < 4: 20 li mod 64 runs through the 16 multiples of 4, lg fills the gaps, so the 64
//     lanes hit 64 different banks; rows of 80 bytes keep the 16-byte staging stores aligned.  (18, the double form's stride,
//     would give 18 li + lg: 2-way conflicts.)  Panel images W / Lr [pivot][row] stay as they are: a column store and the
//     per-pivot row fetch are 64 resp. 16 consecutive floats, the diagonal W[65 lane] walks through all banks.
//   * rho, rho_old and the rho slots are floats; the ladder itself is walked in double on the float inputs widened, and rounded once
//     where a value is stored, so that they equal the Float64 ladder's values rounded to float.
//   * v_rcp_f32 is good to 1 ulp; one Newton step brings a reciprocal to rounding level (relative error e^2 + 2^-24 for a start
//     error e), and a multiplier formed with the raw reciprocal and ONE residual correction (l0 = a r0; l = l0 + (a - d l0) r0) is
//     within an ulp of the quotient a / d.  That is the accuracy the panel steps rely on.
// Nothing here synchronises with the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "dense.h"
#include "dense_impl.h"

namespace cnl {

namespace {

constexpr int TS = dn::TS;   // tile order
constexpr int TT = dn::TT;   // floats per tile
typedef float f4 __attribute__((ext_vector_type(4)));

struct DnStateF {  // per problem, device
  float rho, rho_old, wrote;
  int nfact, success, done, pad;
};

struct DnDevF {  // dense.hip: DnDev, in floats (m == 0: the general form, one condensed system as a dense matrix)
  int ns, nv, T, nsp;
  int n, m, p, mp, npj, Tn;
  int nnz;
  int ks, ntl, nlt;
  int Tm, nml;
  int npos_ok;
  const int *jslot, *dslot;
  const int *lI, *lJ;
  const int *ht_ptr, *hu_loc, *hu_ptr, *hslot;
  const int* gpos;  // general form: position i + ns j of every slot
  int nslots;
  float *Jw;
  float *Jd, *w, *slab, *S0, *S, *G, *Wn, *dv, *rsh, *y, *x, *jxp;
  float *part1, *part2, *partA, *partB;
  const int *sy_wg, *sy_b, *sy_tl, *sy_ch0, *sy_ch1, *sy_tp;
  int* cnt;
  DnStateF* st;
};

__device__ __forceinline__ size_t tile_off(int T, int I, int J) { return ((size_t)J * T + I) * TT; }

// 1 / d to rounding level: v_rcp_f32 (1 ulp) and one Newton step
__device__ __forceinline__ float recip(float d) {
  float r = __builtin_amdgcn_rcpf(d);
  const float e = fmaf(-d, r, 1.0f);
  return fmaf(r, e, r);
}

// ---------------------------------------------------------------------------------------------------------------------
// J(i, j) = vals[jslot], zero-padded to mp x npj; w_i = -1 / d_r(i); inertia of the residual pivots (solver_types.jl:90-95)
__global__ void __launch_bounds__(256) dnf_gather(DnDevF D, const float* __restrict__ vals, float eig_tol) {
  const int b = blockIdx.y;
  const float* v = vals + (size_t)b * D.nnz;
  float* Jd = D.Jd + (size_t)b * D.mp * D.npj;
  float* Jw = D.Jw + (size_t)b * D.mp * D.npj;
  float* w = D.w + (size_t)b * D.mp;
  const long long tot = (long long)D.m * D.n;
  int np = 0, nz = 0;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < tot; t += (long long)gridDim.x * 256) {
    const int i = (int)(t % D.m), j = (int)(t / D.m);
    const float jv = v[D.jslot[t]], dvv = v[D.dslot[i]], wi = -1.0f / dvv;
    Jd[(size_t)i + (size_t)D.mp * j] = jv;
    Jw[(size_t)i + (size_t)D.mp * j] = jv * wi;
    if (j == 0) {
      w[i] = wi;
      np += dvv > eig_tol;
      nz += fabsf(dvv) <= eig_tol;
    }
  }
  if (np) atomicAdd(&D.cnt[b * 4 + 2], np);
  if (nz) atomicAdd(&D.cnt[b * 4 + 3], nz);
}

// ---------------------------------------------------------------------------------------------------------------------
// slab[piece] = sum over the rows of the piece of  J(:, I)' diag(w) J(:, J)   (lower tiles I >= J), as dn_syrk2 of dense.hip:
// 128 x 128 macro tile per workgroup, 4 waves with a 64 x 64 quadrant each (4 x 4 accumulators = 16 independent chains: the
// 40-cycle dependent latency of the f32 instruction never shows), chunks of 16 rows staged through LDS, the next chunk
// prefetched into registers.  The core produces C' (D'[c][r]); register reg of lane (lg, li) is c = 4 lg + reg, r = li.
constexpr int MT = 128, KT = dn::KT, LDK = 20;
__global__ void __launch_bounds__(256, 2) dnf_syrk2(DnDevF D) {
  __shared__ __attribute__((aligned(16))) float tA[MT * LDK];
  __shared__ __attribute__((aligned(16))) float tB[MT * LDK];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 15, lg = lane >> 4;
  const int col = t >> 1, part = t & 1;          // staging: thread = (column of the macro tile, 8-row half of the chunk)
  const int wc = (wave >> 1) * 64, wr = (wave & 1) * 64;  // this wave's quadrant: A-side columns wc.., B-side columns wr..
  for (int pc = D.sy_wg[blockIdx.x]; pc < D.sy_wg[blockIdx.x + 1]; pc++) {
    const int b = D.sy_b[pc], ml = D.sy_tl[pc], ch0 = D.sy_ch0[pc], ch1 = D.sy_ch1[pc];
    int MJ = 0, rem = ml;  // lower macro tile, column by column
    while (rem >= D.Tm - MJ) { rem -= D.Tm - MJ; MJ++; }
    const int MI = MJ + rem;
    const float* Jb = D.Jd + (size_t)b * D.mp * D.npj;
    const float* Jwb = D.Jw + (size_t)b * D.mp * D.npj;
    f4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) acc[i][j] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* pa = Jwb + (size_t)D.mp * min(MT * MJ + col, D.npj - 1) + 8 * part;
    const float* pb = Jb + (size_t)D.mp * min(MT * MI + col, D.npj - 1) + 8 * part;
    float4 ra0, ra1, rb0, rb1;
#define DNF_GLOAD2(CH)                                                              \
  {                                                                                 \
    const float4* qa_ = reinterpret_cast<const float4*>(pa + (CH) * KT);            \
    const float4* qb_ = reinterpret_cast<const float4*>(pb + (CH) * KT);            \
    ra0 = qa_[0]; ra1 = qa_[1];                                                     \
    rb0 = qb_[0]; rb1 = qb_[1];                                                     \
  }
    DNF_GLOAD2(ch0)
    for (int ch = ch0; ch < ch1; ch++) {
      __syncthreads();
      {
        float4* wa_ = reinterpret_cast<float4*>(&tA[col * LDK + 8 * part]);
        float4* wb_ = reinterpret_cast<float4*>(&tB[col * LDK + 8 * part]);
        wa_[0] = ra0; wa_[1] = ra1;
        wb_[0] = rb0; wb_[1] = rb1;
      }
      __syncthreads();
      if (ch + 1 < ch1) DNF_GLOAD2(ch + 1)
#pragma unroll 2
      for (int s = 0; s < KT / 4; s++) {
        float a[4], bb[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          a[i] = tA[(wc + 16 * i + li) * LDK + 4 * s + lg];
          bb[i] = tB[(wr + 16 * i + li) * LDK + 4 * s + lg];
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bb[j], acc[i][j], 0, 0, 0);
      }
    }
#undef DNF_GLOAD2
    // quadrant (wr, wc) of the macro tile = 64 x 64 tile (2 MI + (wave & 1), 2 MJ + (wave >> 1)); the upper one of a diagonal
    // macro tile is not needed
    if (!(MI == MJ && (wave & 1) == 0 && (wave >> 1) == 1)) {
      float* out = D.slab + ((size_t)pc * 4 + (size_t)((wave & 1) * 2 + (wave >> 1))) * TT;
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
          for (int reg = 0; reg < 4; reg++) out[(16 * j + li) + 64 * (16 * i + 4 * lg + reg)] = acc[i][j][reg];
    }
  }
}

// S = S0 + shift on the diagonal of one lower tile (pad rows: unit diagonal)
__device__ __forceinline__ void shift_tile(const DnDevF& D, const float* S0t, float* St, int I, int J, const float* rsh, int tid, int nthr) {
  for (int e = tid; e < TT; e += nthr) {
    float v = S0t[e];
    if (I == J) {
      const int r = e & 63, c = e >> 6;
      if (r == c) { const int gi = 64 * I + r; v = gi < D.ns ? v + rsh[gi] : 1.0f; }
    }
    St[e] = v;
  }
}

// S0 = sum of the pieces of J'WJ (fixed order) + H entries in COO order; S = S0 + rho slots as given (first attempt)
__global__ void __launch_bounds__(256) dnf_assemble(DnDevF D, const float* __restrict__ vals) {
  __shared__ __attribute__((aligned(16))) float tile[TT];
  __shared__ float sh64[64];
  const int b = blockIdx.y, lt = blockIdx.x, t = threadIdx.x;
  const int I = D.lI[lt], J = D.lJ[lt];
  const float* v = vals + (size_t)b * D.nnz;
  float* rsh = D.rsh + (size_t)b * D.nsp;
  const bool has_slab = D.m > 0 && I < D.Tn;
  const int MI = I >> 1, MJ = J >> 1, sub = (I & 1) * 2 + (J & 1);   // pieces come per 128 x 128 macro tile, four tiles each
  const int ml = MJ * D.Tm - (MJ * (MJ - 1)) / 2 + (MI - MJ);
  int p0 = 0, p1 = 0;
  if (has_slab) { p0 = D.sy_tp[b * D.nml + ml]; p1 = D.sy_tp[b * D.nml + ml + 1]; }
  float4 s4[4];
#pragma unroll
  for (int q = 0; q < 4; q++) s4[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int pc = p0; pc < p1; pc++) {
    const float4* sp = reinterpret_cast<const float4*>(D.slab + ((size_t)pc * 4 + sub) * TT) + t;
    float4 g[4];
#pragma unroll
    for (int q = 0; q < 4; q++) g[q] = sp[256 * q];
#pragma unroll
    for (int q = 0; q < 4; q++) { s4[q].x += g[q].x; s4[q].y += g[q].y; s4[q].z += g[q].z; s4[q].w += g[q].w; }
  }
#pragma unroll
  for (int q = 0; q < 4; q++) reinterpret_cast<float4*>(tile)[t + 256 * q] = s4[q];
  if (I == J && t < 64) {
    const int gi = 64 * I + t;
    const float sv = gi < D.nv ? v[D.nnz - D.nv + gi] : 0.0f;
    rsh[gi] = sv;
    sh64[t] = sv;
  }
  __syncthreads();
  for (int e = D.ht_ptr[lt] + t; e < D.ht_ptr[lt + 1]; e += 256) {
    float s = tile[D.hu_loc[e]];
    for (int q = D.hu_ptr[e]; q < D.hu_ptr[e + 1]; q++) s += v[D.hslot[q]];
    tile[D.hu_loc[e]] = s;
  }
  __syncthreads();
  const size_t off = (size_t)b * D.T * D.T * TT + tile_off(D.T, I, J);
#pragma unroll
  for (int q = 0; q < 4; q++) reinterpret_cast<float4*>(D.S0 + off)[t + 256 * q] = reinterpret_cast<const float4*>(tile)[t + 256 * q];
  shift_tile(D, tile, D.S + off, I, J, sh64 - 64 * I, t, 256);
}

// general condensed system (dense.hip: dn_scatter_general, dn_shift): S0 from the slots of the float condensed buffer (unique
// positions; dn_zero16 zeroes S0 in front: n4 groups of 16 bytes, a whole number of tiles of either element type — the double form
// of dense.hip zeroes its S0 through it too, dn::zero_async —), the rho slots behind them become
// the shifts; then S = S0 + shift, tile by tile
__global__ void __launch_bounds__(256) dn_zero16(float4* __restrict__ p, long long n4) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) p[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
__global__ void __launch_bounds__(256) dnf_scatter_general(DnDevF D, const float* __restrict__ cbuf, long long cstride) {
  const int b = blockIdx.y;
  const float* cb = cbuf + (size_t)b * cstride;
  float* S0 = D.S0 + (size_t)b * D.T * D.T * TT;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < D.nslots; e += gridDim.x * 256) {
    const int pos = D.gpos[e], i = pos % D.ns, j = pos / D.ns;
    S0[tile_off(D.T, i >> 6, j >> 6) + (i & 63) + 64 * (j & 63)] = cb[e];
  }
  float* rsh = D.rsh + (size_t)b * D.nsp;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < D.nsp; i += gridDim.x * 256) rsh[i] = i < D.nv ? cb[D.nslots + i] : 0.0f;
}
__global__ void __launch_bounds__(256) dnf_shift(DnDevF D) {
  const int b = blockIdx.y, lt = blockIdx.x;
  const int I = D.lI[lt], J = D.lJ[lt];
  const size_t off = (size_t)b * D.T * D.T * TT + tile_off(D.T, I, J);
  shift_tile(D, D.S0 + off, D.S + off, I, J, D.rsh + (size_t)b * D.nsp, threadIdx.x, 256);
}

// ---------------------------------------------------------------------------------------------------------------------
// Panel step, one wavefront per tile (dense.hip: dn_panel).  Row-per-lane: lane r holds row r of a 64 x 64 tile in registers.  The
// wave that owns the diagonal tile publishes, per pivot j, the column below the pivot BEFORE it is divided in LDS row j and the
// reciprocal pivot; every row x of the tile column then becomes  l = x[j] / d_j,  x[c] -= l w_c (c > j).  The other waves consume
// the published rows eight pivots at a time.
struct PanelLds {
  float W[TS * TS];
  float inv[TS + 8];  // [TS ..]: dump slots, so that "lane 0 stores" needs no branch
  int pub[12];        // [0]: pivots published; [1 ..]: dump slots
};
#define DNF_PIN(v) asm volatile("" : "+v"(v))  // the value is computed here, not sunk to its next use

__device__ __forceinline__ void lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// The rank-1 update x[c] -= l w_c takes its wave-uniform operand through the DPP row broadcast of the f32 FMA, as the double form
// does: the published column is read ONCE per pivot as four registers (lane i of every 16-lane row holds w[16 k + i]) and
//   x[c] += W_{c / 16}[row_newbcast: c % 16] * (-l)
// is one instruction without LDS traffic.  (hipcc does not pad hazards inside asm: the DPP source comes from an LDS read, not from a
// VALU write.)
#define DNF_FMAC_BCAST(X, WK, NL, I) \
  asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:" #I " row_mask:0xf bank_mask:0xf" : "+v"(X) : "v"(WK), "v"(NL))
template <int C>
__device__ __forceinline__ void fmac_bcast(float& x, const float (&W)[4], float nl) {
  constexpr int K = C >> 4, I = C & 15;
  if constexpr (I == 0) DNF_FMAC_BCAST(x, W[K], nl, 0);
  else if constexpr (I == 1) DNF_FMAC_BCAST(x, W[K], nl, 1);
  else if constexpr (I == 2) DNF_FMAC_BCAST(x, W[K], nl, 2);
  else if constexpr (I == 3) DNF_FMAC_BCAST(x, W[K], nl, 3);
  else if constexpr (I == 4) DNF_FMAC_BCAST(x, W[K], nl, 4);
  else if constexpr (I == 5) DNF_FMAC_BCAST(x, W[K], nl, 5);
  else if constexpr (I == 6) DNF_FMAC_BCAST(x, W[K], nl, 6);
  else if constexpr (I == 7) DNF_FMAC_BCAST(x, W[K], nl, 7);
  else if constexpr (I == 8) DNF_FMAC_BCAST(x, W[K], nl, 8);
  else if constexpr (I == 9) DNF_FMAC_BCAST(x, W[K], nl, 9);
  else if constexpr (I == 10) DNF_FMAC_BCAST(x, W[K], nl, 10);
  else if constexpr (I == 11) DNF_FMAC_BCAST(x, W[K], nl, 11);
  else if constexpr (I == 12) DNF_FMAC_BCAST(x, W[K], nl, 12);
  else if constexpr (I == 13) DNF_FMAC_BCAST(x, W[K], nl, 13);
  else if constexpr (I == 14) DNF_FMAC_BCAST(x, W[K], nl, 14);
  else DNF_FMAC_BCAST(x, W[K], nl, 15);
}
// x[c] += W[c] * nl for c = C0 .. 63
template <int C0>
__device__ __forceinline__ void bulk_from(float (&x)[TS], const float (&W)[4], float nl) {
  if constexpr (C0 < TS) {
    fmac_bcast<C0>(x[C0], W, nl);
    bulk_from<C0 + 1>(x, W, nl);
  }
}
// registers k >= K0 of row j of the published columns: lane i of every row of 16 lanes takes w[16 k + i]
template <int K0>
__device__ __forceinline__ void load_wrow(const PanelLds& P, int j, int li, float (&W)[4]) {
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (k >= K0) W[k] = P.W[j * 64 + 16 * k + li];
}

// returns the pivot counts through np / nz (same value in every lane); the pivots stay in P.W[j][j].  Software pipeline as in the
// double form: the region of pivot J holds the CHAIN of pivot J + 1 next to the BULK of pivot J.
template <int J>
__device__ __forceinline__ void diag_step(PanelLds& P, float (&a)[TS], float& l, float& rinv, float& d, float (&W)[4], int lane,
                                          int nreal, float eig_tol, int& np, int& nz) {
  // here: l = multiplier of pivot J (a[J] / d_J), rinv ~ 1 / d_J, d = d_J, W = row J of the published columns
  if (J < nreal) { np += d > eig_tol; nz += fabsf(d) <= eig_tol; }
  const float nl = -l;
  float ln = 0.0f, rn = 0.0f, dn = 0.0f;
  float Wn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (J + 1 < TS) {
    fmac_bcast<J + 1>(a[J + 1], W, nl);
    P.W[(J + 1) * 64 + lane] = a[J + 1];
  }
  // the reciprocal the other waves use: rinv is v_rcp_f32 + one Newton step already; a second one off the critical chain
  {
    const float e = fmaf(-d, rinv, 1.0f);
    const float r2 = fmaf(rinv, e, rinv);
    P.inv[lane == 0 ? J : TS + (lane & 7)] = r2;  // branch-free "lane 0 stores": no control flow inside the pipeline
  }
  // LDS executes one wave's operations in order: the counter becomes visible after the column and the reciprocal
  // without waiting for them here (a release store would stall the chain for an LDS round trip)
  asm volatile("" ::: "memory");
  __hip_atomic_store(&P.pub[lane == 0 ? 0 : 1 + (lane & 7)], J + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  asm volatile("" ::: "memory");
  if constexpr (J + 1 < TS) {
    dn = P.W[(J + 1) * 64 + J + 1];
    load_wrow<((J + 2) >> 4)>(P, J + 1, lane & 15, Wn);
    // multiplier through the raw reciprocal (1 ulp) and one residual correction: within an ulp of the quotient
    const float r0 = __builtin_amdgcn_rcpf(dn);
    const float l0 = a[J + 1] * r0;
    const float res = fmaf(-dn, l0, a[J + 1]);
    ln = fmaf(res, r0, l0);
    const float e0 = fmaf(-dn, r0, 1.0f);
    rn = fmaf(r0, e0, r0);
  }
  bulk_from<J + 2>(a, W, nl);
  DNF_PIN(ln);
  __builtin_amdgcn_sched_barrier(0);
  l = ln; rinv = rn; d = dn;
#pragma unroll
  for (int k = 0; k < 4; k++) W[k] = Wn[k];
  if constexpr (J + 1 < TS) diag_step<J + 1>(P, a, l, rinv, d, W, lane, nreal, eig_tol, np, nz);
}
__device__ void panel_diag(PanelLds& P, const float* __restrict__ tile, int nreal, float eig_tol, int& np_out, int& nz_out) {
  const int lane = threadIdx.x & 63;
  float a[TS];
#pragma unroll
  for (int c = 0; c < TS; c++) a[c] = tile[lane + 64 * c];
  P.W[lane] = a[0];
  int np = 0, nz = 0;
  float W[4];
  float d = P.W[0];
  load_wrow<0>(P, 0, lane & 15, W);
  float rinv = recip(d);
  float l = a[0] * rinv;
  diag_step<0>(P, a, l, rinv, d, W, lane, nreal, eig_tol, np, nz);
  np_out = np; nz_out = nz;
}

// one 64-row tile of the column: in = tile (or the identity when `ident`), out = L form
template <int J>
__device__ __forceinline__ void rows_step(PanelLds& P, float (&x)[TS], float (&W)[4], int li, float* __restrict__ wout, int lane) {
  if constexpr (J % 8 == 0) {  // eight pivots per wait on the publisher
    while (__hip_atomic_load(&P.pub[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < J + 8) __builtin_amdgcn_s_sleep(1);
    load_wrow<((J + 1) >> 4)>(P, J, li, W);
  }
  if (wout) wout[lane + 64 * J] = -x[J];  // -l d: the B operand of this column's trailing update (wave-uniform branch)
  const float l = x[J] * P.inv[J];
  x[J] = l;
  const float nl = -l;
  float Wn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (J % 8 != 7 && J + 1 < TS) load_wrow<((J + 2) >> 4)>(P, J + 1, li, Wn);
  bulk_from<J + 1>(x, W, nl);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (J % 8 != 7) {
#pragma unroll
    for (int k = 0; k < 4; k++) W[k] = Wn[k];
  }
  if constexpr (J + 1 < TS) rows_step<J + 1>(P, x, W, li, wout, lane);
}
__device__ void panel_rows(PanelLds& P, const float* __restrict__ in, float* __restrict__ out, float* __restrict__ wout, bool ident) {
  const int lane = threadIdx.x & 63;
  float x[TS];
  if (ident) {
#pragma unroll
    for (int c = 0; c < TS; c++) x[c] = c == lane ? 1.0f : 0.0f;
  } else {
#pragma unroll
    for (int c = 0; c < TS; c++) x[c] = in[lane + 64 * c];
  }
  float W[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  rows_step<0>(P, x, W, lane & 15, wout, lane);
#pragma unroll
  for (int c = 0; c < TS; c++) out[lane + 64 * c] = x[c];
}

// row tile rt of tile column k: the T - 1 - k tiles below the diagonal of S first, then the k + 1 tiles of the G block
__device__ __forceinline__ void row_tile_ptrs(const DnDevF& D, int b, int k, int rt, const float*& in, float*& out, float*& wout, bool& ident) {
  const size_t pb = (size_t)b * D.T * D.T * TT;
  const int ntop = D.T - 1 - k;
  if (rt < ntop) {
    float* p = D.S + pb + tile_off(D.T, k + 1 + rt, k);
    in = p; out = p; ident = false;
    wout = D.Wn + ((size_t)b * D.T + (k + 1 + rt)) * TT;
  } else {
    const int I = rt - ntop;
    float* p = D.G + pb + tile_off(D.T, I, k);
    in = p; out = p; ident = I == k;
    wout = nullptr;
  }
}

__global__ void __launch_bounds__(256) dnf_panel(DnDevF D, int k, float eig_tol, int b0) {
  __shared__ PanelLds P;
  const int b = b0 + blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x == 0) P.pub[0] = 0;
  __syncthreads();
  if (wave == 0) {
    int np, nz;
    panel_diag(P, D.S + (size_t)b * D.T * D.T * TT + tile_off(D.T, k, k), min(64, D.ns - 64 * k), eig_tol, np, nz);
    if (blockIdx.x == 0) {
      lds_fence();
      D.dv[(size_t)b * D.nsp + 64 * k + lane] = P.W[lane * 64 + lane];
      if (lane == 0) {
        if (np) atomicAdd(&D.cnt[b * 4 + 0], np);
        if (nz) atomicAdd(&D.cnt[b * 4 + 1], nz);
      }
    }
  } else {
    const int rt = blockIdx.x * 3 + wave - 1;
    if (rt < D.T) {
      const float* in; float* out; float* wout; bool ident;
      row_tile_ptrs(D, b, k, rt, in, out, wout, ident);
      panel_rows(P, in, out, wout, ident);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Panel step in column blocks (dense.hip: dn_panel2): the diagonal tile and every row tile are cut into four blocks of 16 COLUMNS,
// one wavefront each (lane = row, 16 registers).  Workgroup = row tile rt of the tile column: waves 0 .. 3 the diagonal tile's
// blocks (recomputed by every workgroup), waves 4 .. 7 the row tile's.  A wavefront applies the pivots of the blocks to its left
// as they are published, then runs its own 16 pivots; the pivot and the operands inside the block come from v_readlane.
// Protocol (unchanged from the double form): the owner of pivot J stores column J, the reciprocal, then pub[0] = J + 1; consumers
// wait for pub[0] >= J0 + 4 before they read pivots J0 .. J0 + 3.  A row block stores its multipliers of pivots J0 .. J0 + 3 in Lr,
// then pub[1] = J0 + 4; the row blocks to its right wait for pub[1] >= J0 + 4.
struct Panel2Lds {
  float W[TS * TS];   // [J][r]: column J of the diagonal tile at the moment pivot J is taken (undivided)
  float Lr[TS * TS];  // [J][r]: multiplier of pivot J for row r of the row tile
  float inv[TS + 8];  // [TS ..]: dump slots ("lane 0 stores" without a branch)
  int pub[12];        // [0]: pivots of the diagonal tile published so far, [1]: pivots whose row-tile multipliers are in Lr; dump slots
};
__device__ __forceinline__ void lds_wait_ge(const int* c, int v) {
  while (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < v) __builtin_amdgcn_s_sleep(1);
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ float readlane_f32(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
// x[c] += W[row_newbcast: c] * nl for the 16 columns of a block (c >= C0)
template <int C0>
__device__ __forceinline__ void blk_update(float (&x)[16], float w, float nl) {
#define DNF_B(I) if constexpr (C0 <= I) DNF_FMAC_BCAST(x[I], w, nl, I);
  DNF_B(0) DNF_B(1) DNF_B(2) DNF_B(3) DNF_B(4) DNF_B(5) DNF_B(6) DNF_B(7) DNF_B(8) DNF_B(9) DNF_B(10) DNF_B(11) DNF_B(12) DNF_B(13) DNF_B(14) DNF_B(15)
#undef DNF_B
}

// own pivot JJ (compile-time position inside the block) of a diagonal block.  Chain of a pivot: the column is final -> pivot and
// the operand of the NEXT column's update through v_readlane (scalar operands) -> reciprocal, multiplier -> next column.  The
// other columns of the block take their operands from the published column (one LDS read, DPP broadcast): they are needed a
// pivot later at the earliest.  No branch inside (lane-0 stores go to dump slots otherwise).
template <int JJ>
__device__ __forceinline__ void diag_own(Panel2Lds& P, float (&a)[16], int q, int lane, int li, int nreal, float eig_tol, int& np, int& nz,
                                         float rr, float wprev, float nlprev) {
  // here: a[JJ] is final; rr = v_rcp_f32 of an APPROXIMATION of its pivot, started a pivot ago; wprev / nlprev: operand register
  // and multiplier of the PREVIOUS pivot, whose updates of the columns >= JJ + 2 are still due.
  const int J = 16 * q + JJ;
  const float col = a[JJ];
  P.W[J * 64 + lane] = col;
  const float d = readlane_f32(col, J);
  np += (J < nreal) & (d > eig_tol); nz += (J < nreal) & (fabsf(d) <= eig_tol);
  float rrn = 1.0f;
  float w1 = 0.0f;
  if constexpr (JJ + 1 < 16) {
    w1 = readlane_f32(col, J + 1);
    const float a11 = readlane_f32(a[JJ + 1], J + 1);
    const float dapp = fmaf(-w1, w1 * rr, a11);
    rrn = __builtin_amdgcn_rcpf(dapp);
    DNF_PIN(rrn);  // issued here, ahead of the deferred updates below
  }
  const float e = fmaf(-d, rr, 1.0f);
  float r1 = fmaf(rr, e, rr);
  // The speculative reciprocal is checked against the exact pivot, as in the double form: e is its residual, and one Newton step
  // leaves a relative error of e^2.  The approximation a11 - w1 (w1 rr) loses what the subtraction cancels, so e is small only
  // where the pivot is well separated from its two terms; beyond |e| = 2^-13 (e^2 = 2^-26, a quarter of the float rounding) the
  // reciprocal is formed from the exact pivot (wave-uniform branch, rare).  Tested on the bits: NaN and Inf take the exact path too.
  if ((__float_as_int(e) & 0x7fffffff) > 0x39000000) r1 = recip(d);
  const float l = col * r1;
  const float nl = -l;
  if constexpr (JJ + 1 < 16) a[JJ + 1] = fmaf(w1, nl, a[JJ + 1]);
  // the column after that feeds the next region's a11: scalar operand as well, no LDS round trip on the chain
  if constexpr (JJ + 2 < 16) a[JJ + 2] = fmaf(readlane_f32(col, J + 2), nl, a[JJ + 2]);
  {  // the reciprocal the other wavefronts use: one more Newton step, off the chain
    const float e1 = fmaf(-d, r1, 1.0f);
    P.inv[lane == 0 ? J : TS + (lane & 7)] = fmaf(r1, e1, r1);
  }
  asm volatile("" ::: "memory");
  __hip_atomic_store(&P.pub[lane == 0 ? 0 : 2 + (lane & 7)], J + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // LDS keeps a wave's operations in order
  asm volatile("" ::: "memory");
  // operand register of THIS pivot's remaining updates (columns >= JJ + 3): read back now, used a pivot later
  float w = 0.0f;
  if constexpr (JJ + 3 < 16) w = P.W[J * 64 + 16 * q + li];
  if constexpr (JJ >= 1 && JJ + 2 < 16) blk_update<JJ + 2>(a, wprev, nlprev);
  if constexpr (JJ + 1 < 16) diag_own<JJ + 1>(P, a, q, lane, li, nreal, eig_tol, np, nz, rrn, w, nl);
}

__device__ __forceinline__ void panel2_diag_block(Panel2Lds& P, const float* __restrict__ tile, int q, int lane, int nreal, float eig_tol,
                                                  int& np, int& nz) {
  float a[16];
#pragma unroll
  for (int c = 0; c < 16; c++) a[c] = tile[lane + 64 * (16 * q + c)];
  const int li = lane & 15;
  // four pivots per wait: their operands are in flight together
  for (int J0 = 0; J0 < 16 * q; J0 += 4) {
    lds_wait_ge(&P.pub[0], J0 + 4);
    float l[4], w[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { l[u] = P.W[(J0 + u) * 64 + lane] * P.inv[J0 + u]; w[u] = P.W[(J0 + u) * 64 + 16 * q + li]; }
#pragma unroll
    for (int u = 0; u < 4; u++) blk_update<0>(a, w[u], -l[u]);
  }
  np = 0; nz = 0;
  diag_own<0>(P, a, q, lane, li, nreal, eig_tol, np, nz, __builtin_amdgcn_rcpf(readlane_f32(a[0], 16 * q)), 0.0f, 0.0f);
}

// own pivots JJ .. JJ + 3 of a row block: the four reciprocals and operand registers are read from LDS TOGETHER behind one wait
// on the publisher, so that the chain from pivot to pivot is one update and one multiplication
template <int JJ>
__device__ __forceinline__ void rows_own(Panel2Lds& P, float (&x)[16], int q, int lane, int li, float* __restrict__ wout) {
  const int J0 = 16 * q + JJ;
  lds_wait_ge(&P.pub[0], J0 + 4);
  float iv[4], w[4];
#pragma unroll
  for (int u = 0; u < 4; u++) { iv[u] = P.inv[J0 + u]; w[u] = P.W[(J0 + u) * 64 + 16 * q + li]; }
#define DNF_ROWS_PIVOT(U)                                                                      \
  {                                                                                            \
    constexpr int C = JJ + U;                                                                  \
    if (wout) wout[lane + 64 * (J0 + U)] = -x[C];  /* -l d: the B operand of this column's trailing update */ \
    const float l = x[C] * iv[U];                                                              \
    P.Lr[(J0 + U) * 64 + lane] = l;                                                            \
    x[C] = l;                                                                                  \
    if constexpr (C + 1 < 16) blk_update<C + 1>(x, w[U], -l);                                  \
  }
  DNF_ROWS_PIVOT(0) DNF_ROWS_PIVOT(1) DNF_ROWS_PIVOT(2) DNF_ROWS_PIVOT(3)
#undef DNF_ROWS_PIVOT
  asm volatile("" ::: "memory");
  __hip_atomic_store(&P.pub[lane == 0 ? 1 : 2 + (lane & 7)], J0 + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  asm volatile("" ::: "memory");
  if constexpr (JJ + 4 < 16) rows_own<JJ + 4>(P, x, q, lane, li, wout);
}

__device__ __forceinline__ void panel2_rows_block(Panel2Lds& P, const float* __restrict__ in, float* __restrict__ out, float* __restrict__ wout,
                                                  bool ident, int q, int lane) {
  float x[16];
#pragma unroll
  for (int c = 0; c < 16; c++) x[c] = ident ? ((16 * q + c) == lane ? 1.0f : 0.0f) : in[lane + 64 * (16 * q + c)];
  const int li = lane & 15;
  for (int J0 = 0; J0 < 16 * q; J0 += 4) {
    lds_wait_ge(&P.pub[1], J0 + 4);
    float l[4], w[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { l[u] = P.Lr[(J0 + u) * 64 + lane]; w[u] = P.W[(J0 + u) * 64 + 16 * q + li]; }
#pragma unroll
    for (int u = 0; u < 4; u++) blk_update<0>(x, w[u], -l[u]);
  }
  rows_own<0>(P, x, q, lane, li, wout);
#pragma unroll
  for (int c = 0; c < 16; c++) out[lane + 64 * (16 * q + c)] = x[c];
}

__global__ void __launch_bounds__(512) dnf_panel2(DnDevF D, int k, float eig_tol) {
  __shared__ Panel2Lds P;  // 33 KB: static (the double form's 66 KB need the dynamic opt-in)
  const int b = blockIdx.y, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (threadIdx.x == 0) { P.pub[0] = 0; P.pub[1] = 0; }
  __syncthreads();
  if (wave < 4) {
    int np, nz;
    panel2_diag_block(P, D.S + (size_t)b * D.T * D.T * TT + tile_off(D.T, k, k), wave, lane, min(64, D.ns - 64 * k), eig_tol, np, nz);
    if (blockIdx.x == 0) {
      if (lane >= 16 * wave && lane < 16 * wave + 16) D.dv[(size_t)b * D.nsp + 64 * k + lane] = P.W[lane * 64 + lane];  // own column: written by this wave
      if (lane == 0) {
        if (np) atomicAdd(&D.cnt[b * 4 + 0], np);
        if (nz) atomicAdd(&D.cnt[b * 4 + 1], nz);
      }
    }
  } else {
    const int rt = blockIdx.x;
    const float* in; float* out; float* wout; bool ident;
    row_tile_ptrs(D, b, k, rt, in, out, wout, ident);
    panel2_rows_block(P, in, out, wout, ident, wave - 4, lane);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// C(I, J) -= L(I, k) diag(d) L(J, k)'  (tiles of S, or of the G block with G(I, k) in place of L(I, k)): rank-64 update of one tile
// on the f32 matrix cores.  The core produces C'; its A operand is the tile -L(J, k) d that the panel step left in Wn, its B
// operand the L form of the row tile.  One wave per 16 x 16 block, operands straight from L2 in the operand layout, two
// accumulators (even / odd k-steps) so that two independent chains cover the 40-cycle dependent latency of the instruction.
// Register reg of lane (lg, li) is row 4 lg + reg of the product (the double form: lg + 4 reg).
__device__ __forceinline__ void update_block(const float* __restrict__ At, const float* __restrict__ Wt, float* __restrict__ Ct, bool czero,
                                             int blk, int lane) {
  const int li = lane & 15, lg = lane >> 4, bc = blk >> 2, br = blk & 3;
  float aop[16], bop[16];
#pragma unroll
  for (int s = 0; s < 16; s++) {
    aop[s] = Wt[(16 * bc + li) + 64 * (4 * s + lg)];
    bop[s] = At[(16 * br + li) + 64 * (4 * s + lg)];
  }
  f4 acc, acc2 = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int reg = 0; reg < 4; reg++) acc[reg] = czero ? 0.0f : Ct[(16 * br + li) + 64 * (16 * bc + 4 * lg + reg)];
#pragma unroll
  for (int s = 0; s < 16; s += 2) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aop[s], bop[s], acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(aop[s + 1], bop[s + 1], acc2, 0, 0, 0);
  }
#pragma unroll
  for (int reg = 0; reg < 4; reg++) Ct[(16 * br + li) + 64 * (16 * bc + 4 * lg + reg)] = acc[reg] + acc2[reg];
}

// trailing tile idx of step k: lower tiles (I >= J > k) of S first, then the tiles (I <= k, J > k) of the G block
__device__ __forceinline__ void trailing_tile(const DnDevF& D, int b, int k, int idx, const float*& At, const float*& Bt, float*& Ct, bool& czero) {
  const size_t pb = (size_t)b * D.T * D.T * TT;
  const int nt = D.T - 1 - k, ntop = nt * (nt + 1) / 2;
  int I, J;
  if (idx < ntop) {
    int c = 0, rem = idx;
    while (rem >= nt - c) { rem -= nt - c; c++; }
    J = k + 1 + c; I = J + rem;
    At = D.S + pb + tile_off(D.T, I, k);
    Ct = D.S + pb + tile_off(D.T, I, J);
    czero = false;
  } else {
    const int q = idx - ntop;
    I = q / nt; J = k + 1 + q % nt;
    At = D.G + pb + tile_off(D.T, I, k);
    Ct = D.G + pb + tile_off(D.T, I, J);
    czero = I == k;  // first touch of this tile of the G block
  }
  Bt = D.Wn + ((size_t)b * D.T + J) * TT;
}

// one workgroup = one 32 x 32 quadrant of a trailing tile (4 waves, a 16 x 16 block each)
__global__ void __launch_bounds__(256) dnf_update(DnDevF D, int k, int b0) {
  const int b = b0 + blockIdx.y;
  const float *At, *Bt; float* Ct; bool czero;
  trailing_tile(D, b, k, blockIdx.x >> 2, At, Bt, Ct, czero);
  const int q = blockIdx.x & 3, wave = threadIdx.x >> 6;
  const int blk = ((q >> 1) * 2 + (wave >> 1)) * 4 + (q & 1) * 2 + (wave & 1);
  update_block(At, Bt, Ct, czero, blk, threadIdx.x & 63);
}

// ---------------------------------------------------------------------------------------------------------------------
// inertia rule + first rung of the ladder state.  mode 0: newton, 1: factorize
__global__ void __launch_bounds__(256) dnf_decide(DnDevF D, int batch, int mode, const float* __restrict__ rho_old, int32_t* success,
                                                  int64_t* npos, int64_t* nzero) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  const int tp = D.cnt[b * 4 + 0] + D.cnt[b * 4 + 2], tz = D.cnt[b * 4 + 1] + D.cnt[b * 4 + 3];
  const bool ok = tp == D.npos_ok && tz == 0;
  D.cnt[b * 4 + 0] = 0; D.cnt[b * 4 + 1] = 0; D.cnt[b * 4 + 2] = 0; D.cnt[b * 4 + 3] = 0;  // clean for the next call
  DnStateF s;
  s.rho = 0.0f; s.wrote = 0.0f; s.rho_old = rho_old ? rho_old[b] : 0.0f;
  s.nfact = 1; s.success = ok ? 1 : 0; s.done = (ok || mode == 1) ? 1 : 0; s.pad = 0;
  D.st[b] = s;
  if (mode == 1) {
    success[b] = ok ? 1 : 0;
    if (npos) npos[b] = tp;
    if (nzero) nzero[b] = tz;
  }
}

// rho ladder for the problems whose first factorisation failed: one workgroup per problem repeats the factorisation with
// S = S0 + rho I (src/CaNNOLeS.jl:1029-1047).  Same device code as the per-step kernels, walked tile by tile.  The rungs are
// computed in double from the float inputs widened (the Float64 ladder on those inputs) and rounded where they are stored: the
// shift of an attempt is (float)rho, and so are rho, rho_old and the rho slots handed back.
constexpr int LNW = 8;
__global__ void __launch_bounds__(LNW * 64) dnf_ladder(DnDevF D, float* vals, const float* __restrict__ rho_old_in, float eig_tol, double kdec,
                                                       double kinc, double klarge, double rho0, double rhomax, double rhomin) {
  __shared__ PanelLds P;
  __shared__ int scnt[2];
  __shared__ int s_first[3];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // inertia rule on the first factorisation (src/solver_types.jl:90-97); the counters are left clean for the next call
  if (tid == 0) {
    const int c0 = D.cnt[b * 4 + 0], c1 = D.cnt[b * 4 + 1], c2 = D.cnt[b * 4 + 2], c3 = D.cnt[b * 4 + 3];
    s_first[0] = (c0 + c2 == D.npos_ok && c1 + c3 == 0) ? 1 : 0; s_first[1] = c2; s_first[2] = c3;
    D.cnt[b * 4 + 0] = 0; D.cnt[b * 4 + 1] = 0; D.cnt[b * 4 + 2] = 0; D.cnt[b * 4 + 3] = 0;
  }
  __syncthreads();
  DnStateF s;
  s.rho = 0.0f; s.wrote = 0.0f; s.rho_old = rho_old_in[b]; s.nfact = 1; s.success = 1; s.done = 1; s.pad = 0;
  if (s_first[0]) {
    if (tid == 0) D.st[b] = s;
    return;
  }
  const size_t pb = (size_t)b * D.T * D.T * TT;
  float* rsh = D.rsh + (size_t)b * D.nsp;
  const int rp = s_first[1], rz = s_first[2];
  const double ro_in = (double)s.rho_old;
  double rho = ro_in == 0.0 ? rho0 : fmax(rhomin, kdec * ro_in);
  double wrote = rho;
  int nfact = 1;
  bool success = false;
  while (true) {
    // ---- one attempt at `rho`
    const float rho_f = (float)rho;
    for (int i = tid; i < D.nsp; i += LNW * 64) rsh[i] = i < D.nv ? rho_f : 0.0f;
    if (tid == 0) { scnt[0] = 0; scnt[1] = 0; }
    __threadfence();
    __syncthreads();
    for (int lt = 0; lt < D.nlt; lt++) {
      const int I = D.lI[lt], J = D.lJ[lt];
      const size_t off = pb + tile_off(D.T, I, J);
      shift_tile(D, D.S0 + off, D.S + off, I, J, rsh, tid, LNW * 64);
    }
    __threadfence();
    __syncthreads();
    for (int k = 0; k < D.T; k++) {
      if (tid == 0) P.pub[0] = 0;
      __syncthreads();
      for (int pass = 0; pass * (LNW - 1) < D.T; pass++) {
        if (wave == 0) {
          if (pass == 0) {
            int np, nz;
            panel_diag(P, D.S + pb + tile_off(D.T, k, k), min(64, D.ns - 64 * k), eig_tol, np, nz);
            lds_fence();
            D.dv[(size_t)b * D.nsp + 64 * k + lane] = P.W[lane * 64 + lane];
            if (lane == 0) { scnt[0] += np; scnt[1] += nz; }
          }
        } else {
          const int rt = pass * (LNW - 1) + wave - 1;
          if (rt < D.T) {
            const float* in; float* out; float* wout; bool ident;
            row_tile_ptrs(D, b, k, rt, in, out, wout, ident);
            panel_rows(P, in, out, wout, ident);
          }
        }
      }
      __threadfence();
      __syncthreads();
      const int nt = D.T - 1 - k, ntr = nt * (nt + 1) / 2 + (k + 1) * nt;
      for (int idx = 0; idx < ntr; idx++) {
        const float *At, *Bt; float* Ct; bool czero;
        trailing_tile(D, b, k, idx, At, Bt, Ct, czero);
        update_block(At, Bt, Ct, czero, 2 * wave, lane);
        update_block(At, Bt, Ct, czero, 2 * wave + 1, lane);
      }
      __threadfence();
      __syncthreads();
    }
    nfact++;
    success = scnt[0] + rp == D.npos_ok && scnt[1] + rz == 0;
    __syncthreads();
    if (success || rho > rhomax) break;
    rho = ro_in == 0.0 ? klarge * rho : kinc * rho;
    if (rho > rhomax) break;
    wrote = rho;
  }
  if (rho <= rhomax) s.rho_old = (float)rho;
  s.rho = (float)rho; s.wrote = (float)wrote; s.nfact = nfact; s.success = success ? 1 : 0; s.done = 1;
  if (tid == 0) D.st[b] = s;
  float* vt = vals + (size_t)b * D.nnz + (D.nnz - D.nv);
  for (int i = tid; i < D.nv; i += LNW * 64) vt[i] = s.wrote;
}

// ---------------------------------------------------------------------------------------------------------------------
// solve: y = [rhs_x - J' (rhs_r / d_r); rhs_c]  ->  x = G D G' y  (+ one refinement step with S)  ->  d
__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wave per variable column: y_c = rhs_x[c] + sum_i J(i, c) w_i rhs_r[i]; the constraint part and the pad behind it.
// t = w .* rhs_r is staged in LDS once per workgroup (2048 rows at a time), the column of J streams through 8-byte loads.
__global__ void __launch_bounds__(256) dnf_yrhs(DnDevF D, const float* __restrict__ rhs, int gate) {
  __shared__ float ts[2048];
  const int b = blockIdx.y;
  if (gate && !D.st[b].success) return;
  const int N = D.n + D.m + D.p;
  const float* rb = rhs + (size_t)b * N;
  float* y = D.y + (size_t)b * D.nsp;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const float* w = D.w + (size_t)b * D.mp;
  const float* Jc = D.Jd + (size_t)b * D.mp * D.npj + (size_t)D.mp * min(c, D.npj - 1);
  float s = 0.0f;
  for (int i0 = 0; i0 < D.mp; i0 += 2048) {
    __syncthreads();
    for (int i = threadIdx.x; i < 2048; i += 256) { const int gi = i0 + i; ts[i] = gi < D.m ? w[gi] * rb[D.n + gi] : 0.0f; }
    __syncthreads();
    const int lim = min(2048, D.mp - i0);  // mp is a multiple of 64
#pragma unroll 4
    for (int i = 2 * lane; i < lim; i += 128) {
      const float2 j2 = *reinterpret_cast<const float2*>(Jc + i0 + i);
      s = fmaf(j2.x, ts[i], s);
      s = fmaf(j2.y, ts[i + 1], s);
    }
  }
  s = wave_sum(s);
  if (lane == 0) {
    if (c < D.n) y[c] = rb[c] + s;
    else if (c < D.nsp) y[c] = c < D.ns ? rb[D.n + D.m + (c - D.n)] : 0.0f;
  }
}
// general form: y = the condensed right-hand side, behind the matrix and rho slots of the condensed buffer
__global__ void __launch_bounds__(256) dnf_yrhs_general(DnDevF D, const float* __restrict__ cbuf, long long cstride, int gate) {
  const int b = blockIdx.y;
  if (gate && !D.st[b].success) return;
  const float* crhs = cbuf + (size_t)b * cstride + D.nslots + D.nv;
  float* y = D.y + (size_t)b * D.nsp;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < D.nsp; i += gridDim.x * 256) y[i] = i < D.ns ? crhs[i] : 0.0f;
}

// ---- tile GEMVs of the solve.  Every tile of G (upper, J >= I) resp. S (lower) is one workgroup; a tile product is 64
// partial sums, and the vector a later kernel needs is summed from the partials in a fixed order by the workgroup that
// needs it, so the results are deterministic and no reduction launches are needed.
__device__ __forceinline__ size_t part_off(const DnDevF& D, int b, int I, int J) { return (((size_t)b * D.T + J) * D.T + I) * 64; }

// sum_{q = q0}^{q1 - 1} base[q * stride] in index order; the loads of eight terms are in flight together
__device__ __forceinline__ float sum_strided(const float* __restrict__ base, size_t stride, int q0, int q1) {
  float s = 0.0f;
  for (int c0 = q0; c0 < q1; c0 += 8) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; q++) v[q] = c0 + q < q1 ? base[(size_t)(c0 + q) * stride] : 0.0f;
#pragma unroll
    for (int q = 0; q < 8; q++) s += v[q];
  }
  return s;
}

// row sums out[r] = sum_c tile[r + 64 c] v[c] over the columns with mask(r, c); 256 threads, v in LDS, red = [4][64] LDS
template <class M>
__device__ __forceinline__ void tile_rowsum(const float* __restrict__ tile, const float* v, float (*red)[64], float* __restrict__ out, M mask) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float tv[16];
#pragma unroll
  for (int q = 0; q < 16; q++) tv[q] = tile[lane + 64 * (16 * wave + q)];
  float acc = 0.0f;
#pragma unroll
  for (int q = 0; q < 16; q++) if (mask(lane, 16 * wave + q)) acc = fmaf(tv[q], v[16 * wave + q], acc);
  red[wave][lane] = acc;
  __syncthreads();
  if (wave == 0) out[lane] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
  __syncthreads();
}
// column sums out[c] = sum_r tile[r + 64 c] v[r] over the rows with mask(r, c)
template <class M>
__device__ __forceinline__ void tile_colsum(const float* __restrict__ tile, const float* v, float* __restrict__ out, M mask) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float tv[16];
#pragma unroll
  for (int q = 0; q < 16; q++) tv[q] = tile[lane + 64 * (16 * wave + q)];
  const float vr = v[lane];
  float mine = 0.0f;
#pragma unroll
  for (int q = 0; q < 16; q++) {
    const float s = wave_sum(mask(lane, 16 * wave + q) ? tv[q] * vr : 0.0f);
    if (lane == q) mine = s;
  }
  if (lane < 16) out[16 * wave + lane] = mine;
}
struct MaskAll { __device__ bool operator()(int, int) const { return true; } };
struct MaskLowerEq { __device__ bool operator()(int r, int c) const { return c <= r; } };
struct MaskStrictLower { __device__ bool operator()(int r, int c) const { return r > c; } };

// residual of the first solve, block I, entry i:  y - shift x - (S x)  from the partial products of dnf_resid_part
__device__ __forceinline__ float resid_entry(const DnDevF& D, int b, int I, int i) {
  const int gi = 64 * I + i;
  const size_t vb = (size_t)b * D.nsp;
  const float sh = gi < D.ns ? D.rsh[vb + gi] : 1.0f;
  float s = sh * D.x[vb + gi];
  s += sum_strided(D.partA + part_off(D, b, I, 0) + i, (size_t)D.T * 64, 0, I + 1);   // J = 0 .. I: part_off advances by T * 64 per J
  s += sum_strided(D.partB + part_off(D, b, 0, I) + i, 64, I, D.T);                     // K = I .. T - 1: by 64 per K
  return D.y[vb + gi] - s;
}

// part1(I, J) = G(I, J)' v_I for the upper tiles; v = y (pass 0) or the residual of the first solve (pass 1)
__global__ void __launch_bounds__(256) dnf_gt_part(DnDevF D, int pass, int gate) {
  __shared__ float vs[64];
  const int b = blockIdx.y, I = D.lJ[blockIdx.x], J = D.lI[blockIdx.x];  // lower-tile list read transposed: J >= I
  if (gate && !D.st[b].success) return;
  if (threadIdx.x < 64) vs[threadIdx.x] = pass == 0 ? D.y[(size_t)b * D.nsp + 64 * I + threadIdx.x] : resid_entry(D, b, I, threadIdx.x);
  __syncthreads();
  tile_colsum(D.G + (size_t)b * D.T * D.T * TT + tile_off(D.T, I, J), vs, D.part1 + part_off(D, b, I, J), MaskAll());
}

// part2(I, J) = G(I, J) u_J with u_J = dv_J .* sum_{I' <= J} part1(I', J)
__global__ void __launch_bounds__(256) dnf_g_part(DnDevF D, int gate) {
  __shared__ float us[64], red[4][64];
  const int b = blockIdx.y, I = D.lJ[blockIdx.x], J = D.lI[blockIdx.x];
  if (gate && !D.st[b].success) return;
  if (threadIdx.x < 64) {
    const float s = sum_strided(D.part1 + part_off(D, b, 0, J) + threadIdx.x, 64, 0, J + 1);
    us[threadIdx.x] = D.dv[(size_t)b * D.nsp + 64 * J + threadIdx.x] * s;
  }
  __syncthreads();
  tile_rowsum(D.G + (size_t)b * D.T * D.T * TT + tile_off(D.T, I, J), us, red, D.part2 + part_off(D, b, I, J), MaskAll());
}

// x = sum of part2 (first solve); partA(I, J) = S(I, J) x_J, partB(I, J) = S(I, J)' x_I over the lower tiles of S0
// (the diagonal tiles hold the lower triangle: A takes c <= r, B the strictly lower part transposed)
__global__ void __launch_bounds__(256) dnf_resid_part(DnDevF D, int gate) {
  __shared__ float xJ[64], xI[64], red[4][64];
  const int b = blockIdx.y, I = D.lI[blockIdx.x], J = D.lJ[blockIdx.x];
  if (gate && !D.st[b].success) return;
  if (threadIdx.x < 128) {
    const int B0 = threadIdx.x < 64 ? J : I, i = threadIdx.x & 63;
    const float s = sum_strided(D.part2 + part_off(D, b, B0, 0) + i, (size_t)D.T * 64, B0, D.T);
    (threadIdx.x < 64 ? xJ : xI)[i] = s;
    if (I == J && threadIdx.x < 64) D.x[(size_t)b * D.nsp + 64 * I + i] = s;
  }
  __syncthreads();
  const float* tile = D.S0 + (size_t)b * D.T * D.T * TT + tile_off(D.T, I, J);
  if (I == J) {
    tile_rowsum(tile, xJ, red, D.partA + part_off(D, b, I, J), MaskLowerEq());
    tile_colsum(tile, xI, D.partB + part_off(D, b, I, J), MaskStrictLower());
  } else {
    tile_rowsum(tile, xJ, red, D.partA + part_off(D, b, I, J), MaskAll());
    tile_colsum(tile, xI, D.partB + part_off(D, b, I, J), MaskAll());
  }
}

// x += correction of the refinement step (sum of its part2)
__global__ void __launch_bounds__(64) dnf_xfinal(DnDevF D, int gate) {
  const int b = blockIdx.y, I = blockIdx.x, i = threadIdx.x;
  if (gate && !D.st[b].success) return;
  const float s = D.x[(size_t)b * D.nsp + 64 * I + i] + sum_strided(D.part2 + part_off(D, b, I, 0) + i, (size_t)D.T * 64, I, D.T);
  D.x[(size_t)b * D.nsp + 64 * I + i] = s;
}

// partial products of J x: rows in blocks of 256, columns in chunks of 32
__global__ void __launch_bounds__(256) dnf_jx(DnDevF D, int gate) {
  const int b = blockIdx.z;
  if (gate && !D.st[b].success) return;
  const int i = blockIdx.x * 256 + threadIdx.x, ch = blockIdx.y;
  const float* Jb = D.Jd + (size_t)b * D.mp * D.npj;
  const float* x = D.x + (size_t)b * D.nsp;
  float acc = 0.0f;
  if (i < D.mp) {
#pragma unroll 8
    for (int c = 32 * ch; c < 32 * ch + 32; c++) acc = fmaf(Jb[(size_t)i + (size_t)D.mp * c], x[c], acc);
    D.jxp[((size_t)b * (D.npj / 32) + ch) * D.mp + i] = acc;
  }
}

// d = [-x; -(rhs_r - J x) / d_r; -x_c] and the scalars of newton_system!'s return tuple
__global__ void __launch_bounds__(256) dnf_out(DnDevF D, const float* __restrict__ rhs, float* __restrict__ d, int mode, float* rho_old,
                                               float* rho, int32_t* nfact, int32_t* success) {
  const int b = blockIdx.y;
  const DnStateF s = D.st[b];
  if (mode == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    rho[b] = s.rho; rho_old[b] = s.rho_old; nfact[b] = s.nfact; success[b] = s.success;
  }
  if (mode == 0 && !s.success) return;
  const int N = D.n + D.m + D.p;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float* x = D.x + (size_t)b * D.nsp;
  float* db = d + (size_t)b * N;
  if (i < D.n) db[i] = -x[i];
  else if (i < D.n + D.m) {
    const int q = i - D.n;
    const float jx = sum_strided(D.jxp + (size_t)b * (D.npj / 32) * D.mp + q, (size_t)D.mp, 0, D.npj / 32);
    db[i] = D.w[(size_t)b * D.mp + q] * (rhs[(size_t)b * N + i] - jx);
  } else db[i] = -x[D.n + (i - D.n - D.m)];
}
// general form: d2 = -x in the reduced numbering (the expand pass makes d of it); a problem no rho repairs leaves d2 as it was
__global__ void __launch_bounds__(256) dnf_out_general(DnDevF D, float* __restrict__ d2, int mode, float* rho_old, float* rho, int32_t* nfact,
                                                       int32_t* success) {
  const int b = blockIdx.y;
  const DnStateF s = D.st[b];
  if (mode == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    rho[b] = s.rho; rho_old[b] = s.rho_old; nfact[b] = s.nfact; success[b] = s.success;
  }
  if (mode == 0 && !s.success) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < D.ns) d2[(size_t)b * D.ns + i] = -D.x[(size_t)b * D.nsp + i];
}
// general form: the residual pivots are counted outside (the inertia pass of the condensation, compared in float)
__global__ void __launch_bounds__(256) dnf_set_counts(DnDevF D, int batch, const int* __restrict__ xpos, const int* __restrict__ xzer) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  D.cnt[b * 4 + 0] = 0; D.cnt[b * 4 + 1] = 0;
  D.cnt[b * 4 + 2] = xpos ? xpos[b] : 0; D.cnt[b * 4 + 3] = xzer ? xzer[b] : 0;
}

struct DenseStateF32 : DenseState { DnDevF d{}; };
inline DnDevF& dev32(DenseState* st) { return static_cast<DenseStateF32*>(st)->d; }

// the per-column steps of one factorisation of S (all problems)
int enqueue_factor(DenseState* st, float eig_tol, hipStream_t stream, std::string& err) {
  const DnDevF& d = dev32(st);
  const int B = (int)st->batch;
  for (int k = 0; k < d.T; k++) {
    if (st->panel2) hipLaunchKernelGGL(dnf_panel2, dim3(d.T, B), dim3(512), 0, stream, d, k, eig_tol);
    else hipLaunchKernelGGL(dnf_panel, dim3((d.T + 2) / 3, B), dim3(256), 0, stream, d, k, eig_tol, 0);
    const int nt = d.T - 1 - k, ntr = nt * (nt + 1) / 2 + (k + 1) * nt;
    if (ntr > 0) hipLaunchKernelGGL(dnf_update, dim3(4 * ntr, B), dim3(256), 0, stream, d, k, 0);
  }
  DCHK(hipGetLastError());
  return 0;
}

int enqueue_solve_core(DenseState* st, int gate, hipStream_t stream, std::string& err) {
  const DnDevF& d = dev32(st);
  const int B = (int)st->batch;
  hipLaunchKernelGGL(dnf_gt_part, dim3(d.nlt, B), dim3(256), 0, stream, d, 0, gate);
  hipLaunchKernelGGL(dnf_g_part, dim3(d.nlt, B), dim3(256), 0, stream, d, gate);
  hipLaunchKernelGGL(dnf_resid_part, dim3(d.nlt, B), dim3(256), 0, stream, d, gate);
  hipLaunchKernelGGL(dnf_gt_part, dim3(d.nlt, B), dim3(256), 0, stream, d, 1, gate);
  hipLaunchKernelGGL(dnf_g_part, dim3(d.nlt, B), dim3(256), 0, stream, d, gate);
  hipLaunchKernelGGL(dnf_xfinal, dim3(d.T, B), dim3(64), 0, stream, d, gate);
  DCHK(hipGetLastError());
  return 0;
}

// the launch sequence of dense.hip: dense_enqueue, kernel by kernel
int dense_enqueue_f32(DenseState* st, int mode, float* vals, const float* rhs, float* dout, float* rho_old, float* rho, int32_t* nfact,
                      int32_t* success, int64_t* npos, int64_t* nzero, const double params[9], hipStream_t stream, std::string& err) {
  const DnDevF& d = dev32(st);
  const int B = (int)st->batch;
  const int N = d.n + d.m + d.p;
  const float eig_tol = (float)params[0];  // the inertia rule compares in float
  int rc;
  if (mode != 2) {
    hipLaunchKernelGGL(dnf_gather, dim3(std::min(2048, dn::blocks((long long)d.m * d.n)), B), dim3(256), 0, stream, d, vals, eig_tol);
    hipLaunchKernelGGL(dnf_syrk2, dim3(d.ks), dim3(256), 0, stream, d);
    hipLaunchKernelGGL(dnf_assemble, dim3(d.nlt, B), dim3(256), 0, stream, d, vals);
    if ((rc = enqueue_factor(st, eig_tol, stream, err))) return rc;
    if (mode == 0)
      hipLaunchKernelGGL(dnf_ladder, dim3(B), dim3(LNW * 64), 0, stream, d, vals, rho_old, eig_tol, params[2], params[3], params[4], params[5],
                         params[6], params[7]);
    else
      hipLaunchKernelGGL(dnf_decide, dim3(dn::blocks(B)), dim3(256), 0, stream, d, B, mode, nullptr, success, npos, nzero);
    DCHK(hipGetLastError());
    if (mode == 1) return 0;
  }
  const int gate = mode == 0 ? 1 : 0;
  hipLaunchKernelGGL(dnf_yrhs, dim3((d.nsp + 3) / 4, B), dim3(256), 0, stream, d, rhs, gate);
  if ((rc = enqueue_solve_core(st, gate, stream, err))) return rc;
  hipLaunchKernelGGL(dnf_jx, dim3(d.mp / 256 + (d.mp % 256 ? 1 : 0), d.npj / 32, B), dim3(256), 0, stream, d, gate);
  hipLaunchKernelGGL(dnf_out, dim3(dn::blocks(N), B), dim3(256), 0, stream, d, rhs, dout, mode, rho_old, rho, nfact, success);
  DCHK(hipGetLastError());
  return 0;
}

// the launch sequence of dense.hip: dense_enqueue_general, kernel by kernel (its hipMemsetAsync of S0 is a kernel here: no memset node
// in the captured graph; the double form zeroes through the same kernel, dn::zero_async)
int dense_enqueue_general_f32(DenseState* st, const GeneralOps& G, int mode, const float* cbuf, const int* xpos, const int* xzer, float* d2,
                              float* vals_rho0, int64_t vals_stride, float* rho_old, float* rho, int32_t* nfact, int32_t* success,
                              int64_t* npos, int64_t* nzero, const double params[9], hipStream_t stream, std::string& err) {
  const DnDevF& d = dev32(st);
  const int B = (int)st->batch;
  const float eig_tol = (float)params[0];  // the inertia rule compares in float
  int rc;
  if (mode != 2) {
    hipLaunchKernelGGL(dnf_set_counts, dim3(dn::blocks(B)), dim3(256), 0, stream, d, B, xpos, xzer);
    dn::zero_async(d.S0, (size_t)B * d.T * d.T * TT * sizeof(float), stream);   // S0 of the batch (setup_common allocates exactly this)
    hipLaunchKernelGGL(dnf_scatter_general, dim3(std::min(1024, dn::blocks(std::max(d.nslots, d.nsp))), B), dim3(256), 0, stream, d, cbuf, (long long)G.cstride);
    hipLaunchKernelGGL(dnf_shift, dim3(d.nlt, B), dim3(256), 0, stream, d);
    if ((rc = enqueue_factor(st, eig_tol, stream, err))) return rc;
    if (mode == 0) {
      // the ladder writes the last rho tried into the caller's rho slots: vals_rho0 + b * vals_stride, nv entries
      DnDevF dl = d;
      dl.nnz = (int)vals_stride;  // dnf_ladder addresses vals + b * nnz + (nnz - nv)
      hipLaunchKernelGGL(dnf_ladder, dim3(B), dim3(LNW * 64), 0, stream, dl, vals_rho0 - (vals_stride - d.nv), rho_old, eig_tol, params[2], params[3],
                         params[4], params[5], params[6], params[7]);
    } else
      hipLaunchKernelGGL(dnf_decide, dim3(dn::blocks(B)), dim3(256), 0, stream, d, B, mode, nullptr, success, npos, nzero);
    DCHK(hipGetLastError());
    if (mode == 1) return 0;
  }
  const int gate = mode == 0 ? 1 : 0;
  hipLaunchKernelGGL(dnf_yrhs_general, dim3(std::min(256, dn::blocks(d.nsp)), B), dim3(256), 0, stream, d, cbuf, (long long)G.cstride, gate);
  if ((rc = enqueue_solve_core(st, gate, stream, err))) return rc;
  hipLaunchKernelGGL(dnf_out_general, dim3(dn::blocks(d.ns), B), dim3(256), 0, stream, d, d2, mode, rho_old, rho, nfact, success);
  DCHK(hipGetLastError());
  return 0;
}

}  // namespace

// (the launch is not checked here: both callers end their sequence with hipGetLastError)
void dn::zero_async(void* p, size_t bytes, hipStream_t stream) {
  const long long n4 = (long long)(bytes / 16);
  hipLaunchKernelGGL(dn_zero16, dim3((unsigned)std::min<long long>(8192, (n4 + 255) / 256)), dim3(256), 0, stream, static_cast<float4*>(p), n4);
}

int dense_create_general_f32(DenseState** out, int32_t ns, int32_t nv, int32_t nslots, const int32_t* d_pos, int64_t batch, std::string& err,
                             bool use_graph, int panel_blocks) {
  DenseStateF32* st = new DenseStateF32();
  st->batch = batch;
  st->f32 = true;
  st->use_graph = use_graph;
  st->panel2 = panel_blocks != 0; st->panel2_auto = panel_blocks == 1;
  st->general = true;
  *out = st;
  DnDevF& d = st->d;
  d.n = ns; d.m = 0; d.p = 0; d.nnz = 0; d.mp = 0; d.npj = 0; d.Tn = 0; d.ntl = 0; d.ks = 1;
  d.npos_ok = nv;
  d.nslots = nslots; d.gpos = d_pos;
  return dn::setup_common(st, d, ns, nv, batch, nullptr, 0, err);
}

int dense_run_general_f32(DenseState* st, const GeneralOps& G, int mode, const void* cbuf, const int* xpos, const int* xzer, void* d2,
                          void* vals_rho0, int64_t vals_stride, void* rho_old, void* rho, int32_t* nfact, int32_t* success, int64_t* npos,
                          int64_t* nzero, const double params[9], hipStream_t stream, std::string& err) {
  if (!st->f32 || !st->general) { err = "dense_run_general_f32 needs a Float32 state of the general form (dense_create_general_f32)"; return 4; }
  if (mode == 2 && !st->factored) { err = "cnl_solve before cnl_factorize"; return 5; }
  GraphKey key;
  key.mode = 16 + mode;
  const void* ps[10] = {cbuf, xpos, xzer, d2, vals_rho0, rho_old, rho, nfact, success, npos};
  for (int i = 0; i < 10; i++) key.p[i] = ps[i];
  for (int i = 0; i < 9; i++) key.params[i] = params[i];
  key.extra = (long long)vals_stride ^ ((long long)(uintptr_t)nzero << 1);
  const int rc = dn::run_cached(st, key, stream, err, [&](hipStream_t s2) {
    return dense_enqueue_general_f32(st, G, mode, static_cast<const float*>(cbuf), xpos, xzer, static_cast<float*>(d2), static_cast<float*>(vals_rho0),
                                     vals_stride, static_cast<float*>(rho_old), static_cast<float*>(rho), nfact, success, npos, nzero, params, s2, err);
  });
  if (!rc && mode != 2) st->factored = true;
  return rc;
}

int dense_create_f32(DenseState** out, const DensePlan& P, int64_t batch, std::string& err, bool use_graph, int syrk_wgs, int panel_blocks) {
  DenseStateF32* st = new DenseStateF32();
  st->batch = batch;
  st->f32 = true;
  st->use_graph = use_graph;
  st->panel2 = panel_blocks != 0; st->panel2_auto = panel_blocks == 1;
  *out = st;
  // sizes, work partition, lists and buffers as for the double form (dense_impl.h); every LDS block of the float kernels is static
  return dn::setup_blocks(st, st->d, P, batch, syrk_wgs, nullptr, 0, err);
}

int dense_run_f32(DenseState* st, int mode, void* vals, const void* rhs, void* dout, void* rho_old, void* rho, int32_t* nfact,
                  int32_t* success, int64_t* npos, int64_t* nzero, const double params[9], hipStream_t stream, std::string& err) {
  if (!st->f32) { err = "dense_run_f32 on a Float64 state (dense_run serves it)"; return 4; }
  if (mode == 2 && !st->factored) { err = "cnl_solve before cnl_factorize"; return 5; }
  GraphKey key;
  key.mode = 32 + mode;
  const void* ps[10] = {vals, rhs, dout, rho_old, rho, nfact, success, npos, nzero, nullptr};
  for (int i = 0; i < 10; i++) key.p[i] = ps[i];
  for (int i = 0; i < 9; i++) key.params[i] = params[i];
  const int rc = dn::run_cached(st, key, stream, err, [&](hipStream_t s2) {
    return dense_enqueue_f32(st, mode, static_cast<float*>(vals), static_cast<const float*>(rhs), static_cast<float*>(dout),
                             static_cast<float*>(rho_old), static_cast<float*>(rho), nfact, success, npos, nzero, params, s2, err);
  });
  if (!rc && mode != 2) st->factored = true;
  return rc;
}

}  // namespace cnl
