// band.hip — newton_system! (/root/reference/src/CaNNOLeS.jl:1008-1052) of a batch of band-structured problems as a
// sliding-window elimination with ONE LANE per (problem, part): executes the band program of band.h / band.cpp.
//
// Mapping.  A workgroup serves NL problems with one wavefront per part of the chain (two parts: the first eliminates upwards
// from variable 0, the second downwards from variable n-1, the four variables between them are the junction).  A wavefront
// has two roles that alternate:
//  * mover — all 64 lanes: lane (lq, le) = (lane / 8, lane % 8) moves element le of the 64-byte pieces of problems lq, lq + 8, ...
//    between HBM and the problems' LDS blocks: the operand pieces of the NEXT epoch are loaded into registers while the current
//    epoch computes (the registers are the look-ahead buffer), written to LDS at the next epoch's start, and the solution
//    components an epoch produced (with 8 or 16 problems per workgroup its factor records too) go out the same way.  Every
//    vector-memory instruction moves eight 64-byte runs.
//  * compute — lanes 0 .. NL-1, lane = problem: the window (5 band slots x 5, one border row, the right-hand side: 27 doubles) lives
//    in registers, every operand is one ds_read_b64 at an offset the generator fixed, every update a plain v_fma_f64; with 32
//    problems per workgroup every factor record goes to global memory from the lane that computed it (frec_index).  No
//    cross-lane operation, no LDS atomics, no index decode: the step blocks are wave-uniform and come through the scalar cache.
// Summation order (documented deviation, within the fp64 bar of DESIGN section 5): entering position = plain entries in COO
// order (src/solver_types.jl:53-59: duplicates summed in COO order), then the condensed rows' products in row order, then the
// pivots' updates as they happen.
// Element type T (LDLFactorization{T}): double, or float for Float32 handles (cnl_create_f32).  The program is the same — steps,
// epochs, pieces of EIGHT elements, the lane block of band_lane_elems(NPC) elements — with its LDS byte offsets written for
// sizeof(T) (build_band_plan's element size), so a float operand is one ds_read_b32 at an offset the generator fixed.  All
// arithmetic is in T (fmaf, float compares, v_rcp_f32); only the control block of the two wavefronts stays double (a float
// widens to double exactly).
#include <hip/hip_runtime.h>

#include "band.h"
#include "kernels.h"

namespace cnl {

namespace {

template <class T>
__device__ __forceinline__ T* as_global(T* p) {
  return (T*)(__attribute__((address_space(1))) T*)p;
}

typedef const __attribute__((address_space(4))) int* cptr;   // program blocks: wave-uniform, read through the scalar cache
__device__ __forceinline__ cptr as_const(const int* p) { return (cptr)(const __attribute__((address_space(1))) int*)p; }

constexpr int EXCH_OFF = BAND_IN_OFF;   // junction exchange (46 doubles) in a lane block: over the operand pieces, idle between the sweeps
static_assert(48 <= BAND_NPIECE * 8, "exchange area inside the operand pieces");

__device__ __forceinline__ constexpr int sidx(int a, int b) { return a >= b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; }

// refined reciprocal (v_rcp_f64 is good to 2^-25 on gfx950: one Newton step) and a quotient with a residual correction: the same
// division the register-front kernel uses (kernels2.hip, fast_div), the reciprocal shared by the multipliers of one pivot
// (float: v_rcp_f32 is good to 1 ulp; the same Newton step and residual correction in float)
template <class T>
__device__ __forceinline__ T rrcp(T d) {
  T r;
  if constexpr (sizeof(T) == 8) r = __builtin_amdgcn_rcp(d);
  else r = __builtin_amdgcn_rcpf(d);
  const T e = fma(-d, r, T(1));
  return fma(r, e, r);
}
template <class T>
__device__ __forceinline__ T rdiv(T w, T d, T r) {
  const T q = w * r;
  const T res = fma(-d, q, w);
  return fma(res, r, q);
}


// The window: BAND_NS slots, of which the five that hold the variables entered last are live (the allocator sees that: every
// index below is a compile-time constant, so the dead slots' registers are free).
constexpr int NS = BAND_NS;
template <class T>
struct Win {
  T S[NS * (NS + 1) / 2];   // band slots, packed lower triangle
  T X[NS];                  // border row
  T S55;
  T c[NS];                  // right-hand side
  T c5;
};
// live slot k of step phase PH: 0 = the step's pivot .. BAND_HW = the entering variable
__device__ __forceinline__ constexpr int lslot(int PH, int k) { return (PH - BAND_HW + k + NS) % NS; }

#define LDSD(off) (*reinterpret_cast<const T*>(myb + (off)))
#define LDSW(off) (*reinterpret_cast<T*>(myb + (off)))

// Step and row blocks of the current epoch sit in the wavefront's LDS record buffer (copied there by the mover with the operand
// pieces): every compute lane reads the same address (one broadcast read), the operand offsets stay in VGPRs — they are only ever
// added to the lane's LDS base — and the flags word goes to an SGPR for the wave-uniform branches.
struct Rec { int v[BAND_SW]; };
struct RowRec { int v[BAND_RW]; };
// AL (mover-table instance): the block starts on a 16-byte boundary of LDS — the record buffers lie behind whole lane blocks of 32
// problems, BAND_REC_MAX, BAND_SW and BAND_RW are multiples of four ints — which the compiler cannot see: told so, it reads a block
// with one ds_read_b128 per four words (of the words the sweep uses) where it otherwise reads it in 4- and 8-byte pieces
static_assert(BAND_SW % 4 == 0 && BAND_RW % 4 == 0 && BAND_REC_MAX % 4 == 0, "step and row blocks start on 16-byte boundaries");
template <bool AL = false>
__device__ __forceinline__ const int4* rec_ptr(const char* recb, int o) {
  if constexpr (AL) return static_cast<const int4*>(__builtin_assume_aligned(recb + 4 * o, 16));
  else return reinterpret_cast<const int4*>(recb + 4 * o);
}
typedef unsigned __int128 __attribute__((may_alias)) rec_u128;
template <bool AL = false>
__device__ __forceinline__ void load_rec(Rec& R, const char* recb, int o) {
  const int4* q = rec_ptr<AL>(recb, o);
  if constexpr (AL) {
#pragma unroll
    for (int k = 0; k < BAND_SW / 4; k++) {
      const rec_u128 t = reinterpret_cast<const rec_u128*>(q)[k];
      R.v[4 * k] = (int)t; R.v[4 * k + 1] = (int)(t >> 32); R.v[4 * k + 2] = (int)(t >> 64); R.v[4 * k + 3] = (int)(t >> 96);
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < BAND_SW / 4; k++) { const int4 t = q[k]; R.v[4 * k] = t.x; R.v[4 * k + 1] = t.y; R.v[4 * k + 2] = t.z; R.v[4 * k + 3] = t.w; }
}
template <bool AL = false>
__device__ __forceinline__ void load_row(RowRec& R, const char* recb, int o) {
  const int4* q = rec_ptr<AL>(recb, o);
  if constexpr (AL) {
#pragma unroll
    for (int k = 0; k < BAND_RW / 4; k++) {
      const rec_u128 t = reinterpret_cast<const rec_u128*>(q)[k];
      R.v[4 * k] = (int)t; R.v[4 * k + 1] = (int)(t >> 32); R.v[4 * k + 2] = (int)(t >> 64); R.v[4 * k + 3] = (int)(t >> 96);
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < BAND_RW / 4; k++) { const int4 t = q[k]; R.v[4 * k] = t.x; R.v[4 * k + 1] = t.y; R.v[4 * k + 2] = t.z; R.v[4 * k + 3] = t.w; }
}

// operands of one forward step: the entering variable's fifteen entries and the first residual row
template <class T>
struct FOps { T eo[15]; T rj[BAND_NB]; T rdr, rrr; };
template <class T>
__device__ __forceinline__ void fload(FOps<T>& P, const Rec& st, const RowRec& row0, const int fl, char* myb) {
#pragma unroll
  for (int q = 0; q < 15; q++) P.eo[q] = LDSD(st.v[BS_DG0 + q]);
  static_assert(BS_RX == BS_DG0 + 14, "the fifteen operands of an entering variable are consecutive words of the step block");
  P.rdr = T(1); P.rrr = T(0);
#pragma unroll
  for (int k = 0; k < BAND_NB; k++) P.rj[k] = T(0);
  if ((fl >> 8) & 255) {
#pragma unroll
    for (int k = 0; k < BAND_NB; k++) P.rj[k] = LDSD(row0.v[BR_J0 + k]);
    P.rdr = LDSD(row0.v[BR_DI]);
    P.rrr = LDSD(row0.v[BR_RR]);
  }
}

// offset of element e of a problem from the problem's first element: e for the ABI's problem-major arrays (stride 0); for arrays
// interleaved over the NL problems of a workgroup in blocks of eight doubles (stride = NL * 8) block e / 8 is NL * 8 doubles further
__device__ __forceinline__ long long band_il_offset(int e, int stride) { return stride ? (long long)(e >> 3) * stride + (e & 7) : (long long)e; }

// Factor records of the 32-problem instantiations go from the compute lanes straight to global memory (direct_records).  Their
// layout is private to the launch (written by the forward sweep, read by the backward sweep of the SAME workgroup): ELEMENT-major,
// problem-minor over the NL problems of the workgroup — element e of problem p at (loff + e) * NL + p of the workgroup's region —
// so that one store of the compute lanes writes NL contiguous elements (256 bytes, two whole lines, for 32 doubles) and a
// backward piece of eight elements reads eight such rows (2 KB).  The program's forward BS_LB / BS_LX hold the record's LDS byte offset in the half-epoch out ring the
// generator still lays out (band.cpp: BAND_LOUT_OFF + event * BAND_LREC - BE_LBASE / BE_LBASE2 of the step's half); recb0 = that
// half's BE_LBASE* - BAND_LOUT_OFF turns it back into the record's first element (tests/test_band_records_cpu.py).
// The 8- and 16-problem instantiations keep the records in the LDS out ring at those offsets and the mover flushes them behind
// steps 3 and 7, problem-major: at 8 192 problems and below the chain of one wavefront per SIMD bounds the time, and the compute
// lanes' stores and their address arithmetic cost Float32 with 16 problems per workgroup 4 % (tools/time_band_f32.py) while the
// 32-problem instantiations gain 4 ... 5 %.
__host__ __device__ constexpr bool direct_records(int nl) { return nl >= 32; }
template <class T>
__device__ __forceinline__ int frec_index(int lds_off, int recb0) {
  return (lds_off >> (sizeof(T) == 8 ? 3 : 2)) + recb0;
}

// CACHE POLICY of the mover-table instance (tuning band_cache_policy): a compile-time mask POL over the streams the
// kernel touches ONCE per sweep, so that they leave the XCD's L2 to the lines it touches twice, an epoch apart (the two 64-byte halves
// of a line of the problem-major rhs and d, the program blocks every workgroup reads).  Builtins only; POL = 0 is the plain code.
constexpr int BAND_POL_VALS_NT = 1;     // typed BAND_MK_VALS loads are non-temporal
constexpr int BAND_POL_FACTOR_NT = 2;   // typed BAND_MK_FACTOR loads (backward sweep) are non-temporal
constexpr int BAND_POL_REC_NT = 4;      // record stores of the compute lanes are non-temporal
constexpr int BAND_POL_REC_WT = 8;      // ... or written through and dropped from L2 (a relaxed agent-scope atomic store: sc1); not with 4
constexpr int BAND_POL_D_NT = 16;       // d stores (backward mover, border and junction components) are non-temporal
template <int POL, class T>
__device__ __forceinline__ void rec_store(T* p, T v) {
  static_assert((POL & BAND_POL_REC_NT) == 0 || (POL & BAND_POL_REC_WT) == 0, "a record store is non-temporal or written through, not both");
  if constexpr ((POL & BAND_POL_REC_NT) != 0) __builtin_nontemporal_store(v, p);
  else if constexpr ((POL & BAND_POL_REC_WT) != 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
template <int POL, class T>
__device__ __forceinline__ void d_store(T* p, T v) {
  if constexpr ((POL & BAND_POL_D_NT) != 0) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// one forward step of phase PH = step number % 8: enter slot PH, pivot slot PH - 4; fl = flags word (wave-uniform), o = int
// offset of the step block in the record buffer.  The operands were read (fload) while the previous step computed.  The step's
// factor records go to recp (the lane's first record element, RNL = problems per workgroup) when recst, or to the out ring.
// POL: the cache policy of the record stores (rec_store).
template <int PH, int RNL, int POL, class T>
__device__ __forceinline__ void fstep(Win<T>& W, const FOps<T>& OP, const Rec& st, const int fl, const char* recb, const int o, char* myb,
                                      const T* __restrict__ gvals, const T* __restrict__ grhs, cptr borders, long long pv, long long pr,
                                      bool has_rhs, T rho, bool ovr, T tol, int& npos, int& nzer, const int vstride, const int rstride,
                                      T* recp, const int recb0, const bool recst) {
  constexpr int es = PH, ps = lslot(PH, 0);
  const int nrows = (fl >> 8) & 255;
  const T (&eo)[15] = OP.eo;
  const T (&rj)[BAND_NB] = OP.rj;
  const T rdr = OP.rdr, rrr = OP.rrr;
  // ---- enter ----
  {
    const T dg = (eo[0] + eo[1]) + eo[2];
    T rv = eo[BS_RHO - BS_DG0];
    if (!(fl & (1 << 16))) rv = ovr ? rho : rv;
    W.S[sidx(es, es)] = dg + rv;
#pragma unroll
    for (int k = 1; k <= BAND_HW; k++) W.S[sidx(es, lslot(PH, BAND_HW - k))] = eo[BS_OD - BS_DG0 + 2 * (k - 1)] + eo[BS_OD - BS_DG0 + 2 * (k - 1) + 1];
    W.X[es] = eo[BS_BC0 - BS_DG0] + eo[BS_BC1 - BS_DG0];
    W.c[es] = eo[BS_RX - BS_DG0];
  }
  // ---- residual rows completed by the entering variable: products -J_a J_b / d_r, counted in the inertia ----
  for (int i = 0; i < nrows; i++) {
    T J[BAND_NB], dr, rr;
    if (i == 0) {
#pragma unroll
      for (int k = 0; k < BAND_NB; k++) J[k] = rj[k];
      dr = rdr; rr = rrr;
    } else {
      RowRec rb;
      load_row(rb, recb, o + BAND_SW + BAND_RW * i);
#pragma unroll
      for (int k = 0; k < BAND_NB; k++) J[k] = LDSD(rb.v[BR_J0 + k]);
      dr = LDSD(rb.v[BR_DI]);
      rr = LDSD(rb.v[BR_RR]);
    }
    npos += dr > tol;
    nzer += fabs(dr) <= tol;
    const T r = rrcp(dr);
    const T w = rdiv(T(-1), dr, r);
    const T tr = rr * w;
#pragma unroll
    for (int ka = 0; ka < BAND_NB; ka++) {
      const T ta = J[ka] * w;
#pragma unroll
      for (int kb = 0; kb <= ka; kb++) W.S[sidx(lslot(PH, ka), lslot(PH, kb))] = fma(ta, J[kb], W.S[sidx(lslot(PH, ka), lslot(PH, kb))]);
      W.c[lslot(PH, ka)] = fma(tr, J[ka], W.c[lslot(PH, ka)]);
    }
  }
  // ---- border pivot ----
  if (fl & BF_PIVOT_B) {
    cptr bt = borders + BAND_BW * __builtin_amdgcn_readfirstlane(st.v[BS_BORDER]);
    // (vstride / rstride != 0: the array is interleaved over the workgroup's problems in blocks of eight doubles, see band_il_offset)
    W.S55 += gvals[pv + band_il_offset(bt[BB_DSRC], vstride)];
    W.c5 += has_rhs ? grhs[pr + band_il_offset(bt[BB_RHS], rstride)] : T(0);
    const T d = W.S55;
    npos += d > tol;
    nzer += fabs(d) <= tol;
    const T r = rrcp(d);
    T l[BAND_NB], w[BAND_NB];
#pragma unroll
    for (int k = 0; k < BAND_NB; k++) { w[k] = W.X[lslot(PH, k)]; l[k] = rdiv(w[k], d, r); }
    const T z = rdiv(W.c5, d, r);
#pragma unroll
    for (int ka = 0; ka < BAND_NB; ka++) {
#pragma unroll
      for (int kb = 0; kb <= ka; kb++) W.S[sidx(lslot(PH, ka), lslot(PH, kb))] = fma(w[ka], -l[kb], W.S[sidx(lslot(PH, ka), lslot(PH, kb))]);
      W.c[lslot(PH, ka)] = fma(w[ka], -z, W.c[lslot(PH, ka)]);
    }
    if constexpr (direct_records(RNL)) {
      if (recst) {
        T* lo = recp + frec_index<T>(st.v[BS_LB], recb0) * RNL;
#pragma unroll
        for (int k = 0; k < BAND_NB; k++) rec_store<POL>(lo + k * RNL, l[k]);
        rec_store<POL>(lo + BAND_NB * RNL, z);
      }
    } else {
      T* lo = reinterpret_cast<T*>(myb + st.v[BS_LB]);
#pragma unroll
      for (int k = 0; k < BAND_NB; k++) lo[k] = l[k];
      lo[BAND_NB] = z;
    }
#pragma unroll
    for (int k = 0; k < BAND_NB; k++) W.X[lslot(PH, k)] = T(0);
    W.S55 = T(0); W.c5 = T(0);
  }
  // ---- band pivot ----
  if (fl & BF_PIVOT_X) {
    const T d = W.S[sidx(ps, ps)];
    npos += d > tol;
    nzer += fabs(d) <= tol;
    const T r = rrcp(d);
    T l[BAND_NB], w[BAND_NB];
#pragma unroll
    for (int k = 1; k < BAND_NB; k++) { w[k] = W.S[sidx(lslot(PH, k), ps)]; l[k] = rdiv(w[k], d, r); }
    const T w5 = W.X[ps], l5 = rdiv(w5, d, r), z = rdiv(W.c[ps], d, r);
#pragma unroll
    for (int ka = 1; ka < BAND_NB; ka++) {
#pragma unroll
      for (int kb = 1; kb <= ka; kb++) W.S[sidx(lslot(PH, ka), lslot(PH, kb))] = fma(w[ka], -l[kb], W.S[sidx(lslot(PH, ka), lslot(PH, kb))]);
      W.X[lslot(PH, ka)] = fma(w5, -l[ka], W.X[lslot(PH, ka)]);
      W.c[lslot(PH, ka)] = fma(w[ka], -z, W.c[lslot(PH, ka)]);
    }
    W.S55 = fma(w5, -l5, W.S55);
    W.c5 = fma(w5, -z, W.c5);
    if constexpr (direct_records(RNL)) {
      if (recst) {
        T* lo = recp + frec_index<T>(st.v[BS_LX], recb0) * RNL;
#pragma unroll
        for (int k = 1; k < BAND_NB; k++) rec_store<POL>(lo + (k - 1) * RNL, l[k]);
        rec_store<POL>(lo + 4 * RNL, l5);
        rec_store<POL>(lo + 5 * RNL, z);
      }
    } else {
      T* lo = reinterpret_cast<T*>(myb + st.v[BS_LX]);
#pragma unroll
      for (int k = 1; k < BAND_NB; k++) lo[k - 1] = l[k];
      lo[4] = l5;
      lo[5] = z;
    }
  }
}

// one backward step of phase PH: x of the band pivot, then of the border pivot, then the residual components
template <class T>
struct BOps { T lx[BAND_LREC], lb[BAND_LREC], rj[BAND_NB]; T rdr, rrr; };
template <class T>
__device__ __forceinline__ void bload(BOps<T>& P, const Rec& st, const RowRec& row0, const int fl, char* myb) {
#pragma unroll
  for (int q = 0; q < BAND_LREC; q++) { P.lx[q] = T(0); P.lb[q] = T(0); }
#pragma unroll
  for (int k = 0; k < BAND_NB; k++) P.rj[k] = T(0);
  P.rdr = T(1); P.rrr = T(0);
  if (fl & BF_PIVOT_X) {
    const T* lo = reinterpret_cast<const T*>(myb + st.v[BS_LX]);
#pragma unroll
    for (int q = 0; q < BAND_LREC; q++) P.lx[q] = lo[q];
  }
  if (fl & BF_PIVOT_B) {
    const T* lo = reinterpret_cast<const T*>(myb + st.v[BS_LB]);
#pragma unroll
    for (int q = 0; q < BAND_LREC; q++) P.lb[q] = lo[q];
  }
  if ((fl >> 8) & 255) {
#pragma unroll
    for (int k = 0; k < BAND_NB; k++) P.rj[k] = LDSD(row0.v[BR_J0 + k]);
    P.rdr = LDSD(row0.v[BR_DI]);
    P.rrr = LDSD(row0.v[BR_RR]);
  }
}
template <int PH, int POL, class T>
__device__ __forceinline__ void bstep(T (&xs)[NS + 1], const BOps<T>& OP, const Rec& st, const RowRec& row0, const int fl, const char* recb,
                                      const int o, char* myb, cptr borders, T* __restrict__ gd, long long pd, bool okme) {
  constexpr int ps = lslot(PH, 0);
  const int nrows = (fl >> 8) & 255;
  const T (&lx)[BAND_LREC] = OP.lx;
  const T (&lb)[BAND_LREC] = OP.lb;
  const T (&rj)[BAND_NB] = OP.rj;
  const T rdr = OP.rdr, rrr = OP.rrr;
  if (fl & BF_PIVOT_X) {
    T x = lx[5];
#pragma unroll
    for (int k = 1; k < BAND_NB; k++) x = fma(-lx[k - 1], xs[lslot(PH, k)], x);
    x = fma(-lx[4], xs[NS], x);
    xs[ps] = x;
    LDSW(st.v[BS_DX]) = -x;
  }
  if (fl & BF_PIVOT_B) {
    T x = lb[BAND_NB];
#pragma unroll
    for (int k = 0; k < BAND_NB; k++) x = fma(-lb[k], xs[lslot(PH, k)], x);
    xs[NS] = x;
    if (okme) d_store<POL>(gd + (pd + borders[BAND_BW * __builtin_amdgcn_readfirstlane(st.v[BS_BORDER]) + BB_DOUT]), -x);
  }
  for (int i = 0; i < nrows; i++) {
    T J[BAND_NB], dr, rr;
    int dro;
    if (i == 0) {
#pragma unroll
      for (int k = 0; k < BAND_NB; k++) J[k] = rj[k];
      dr = rdr; rr = rrr; dro = row0.v[BR_DR];
    } else {
      RowRec rb;
      load_row(rb, recb, o + BAND_SW + BAND_RW * i);
#pragma unroll
      for (int k = 0; k < BAND_NB; k++) J[k] = LDSD(rb.v[BR_J0 + k]);
      dr = LDSD(rb.v[BR_DI]); rr = LDSD(rb.v[BR_RR]); dro = rb.v[BR_DR];
    }
    T acc = -rr;
#pragma unroll
    for (int k = 0; k < BAND_NB; k++) acc = fma(J[k], xs[lslot(PH, k)], acc);
    LDSW(dro) = rdiv(acc, dr, rrcp(dr));
  }
  if (fl & BF_ENTER_B) xs[NS] = T(0);
}

}  // namespace

// LDS of a workgroup: [part][NL] lane blocks | [part] record buffers | control block: per problem [rho | flags], one word "all done"
// NPC = operand pieces per epoch of the program the instance runs (BandPlan::npiece): 15, or 20 for the wide form (band.h) — the lane
// block (LANE_D elements, out ring and zero cell behind the pieces), the epoch block (EW words, EF(field)), the staging registers and
// the mover's issue / commit sequences follow it; steps, arithmetic and record format do not, so a pattern both forms can run gives
// bit-equal outputs.
// T = float: the element arrays of LaunchArgs (vals, rhs, d, L, rho_old, rho) hold float arrays (launch_band_f32); params are
// Float32 values widened to double, narrowed back here exactly.
// NPCX = BAND_NPIECE_RESIDENT (RES below): the program is the RESIDENT form of the 15-piece one (band.h) — a piece descriptor names the
// LDS slot its staged piece is committed to, an unused descriptor commits nothing (its slot may hold a block an earlier epoch
// loaded), and the forward sweep's slots reach into the out ring, which the kernel that stores factor records directly does not
// use.  Everything else is the 15-piece kernel.  (A value of the piece-count parameter, not a fourth parameter: the other
// instances keep their names and, every difference being `if constexpr`, their code.)
constexpr int BAND_NPIECE_RESIDENT = BAND_NPIECE + 256;
// NPCX = BAND_NPIECE_MOVER (MOV below): the resident program with the MOVER TABLE in place of its piece descriptors (band.h, BAND_MK_*):
// staging set K of a sweep has a kind fixed at compile time; a typed set forms its piece's address with one 64-bit scalar add — the
// table's byte offset on the workgroup's base of the array — and a per-lane offset that is computed once per launch, where the
// resident instance decodes array, layout, base, stride and lane offset of every piece in every epoch (about 60 instructions in
// front of four loads, on a kernel that instruction issue bounds: DESIGN section 4).  General sets decode as the resident instance does.
constexpr int BAND_NPIECE_MOVER = BAND_NPIECE + 512;
// NPCX = band_npcx_mover(POL): the mover-table instance under cache policy POL (BAND_POL_*, above fstep).  The mask rides on the
// piece-count parameter for the reason the two forms do: POL = 0 is BAND_NPIECE_MOVER itself, and every instance keeps its name.
constexpr int BAND_POL_SHIFT = 10;
constexpr int band_npcx_mover(int pol) { return BAND_NPIECE_MOVER + (pol << BAND_POL_SHIFT); }
#define EF(F) band_ef(F, NPC)
template <class T, int NL, int NPCX>
__global__ void __launch_bounds__(128, (NL <= 8 && NPCX == BAND_NPIECE ? 2 : 1)) band_newton_kernel(const BandDev P, const LaunchArgs Ain) {
  constexpr int POL = NPCX >> BAND_POL_SHIFT;
  constexpr bool MOV = (NPCX & ((1 << BAND_POL_SHIFT) - 1)) == BAND_NPIECE_MOVER;
  static_assert(POL == 0 || MOV, "a cache policy: the mover-table instance only");
  constexpr bool RES = NPCX == BAND_NPIECE_RESIDENT || MOV;
  constexpr int NPC = RES ? BAND_NPIECE : NPCX;
  static_assert(!RES || (direct_records(NL) && NPC == BAND_NPIECE && sizeof(T) == 8), "the resident form: Float64, 32 problems per workgroup, 15 pieces");
  constexpr int DBITS = RES ? BAND_RES_SLOT_SHIFT : 28;   // element bits of a piece descriptor
  constexpr int NI = NL / 8;
  constexpr int LANE_D = band_lane_elems(NPC), LOUT_OFF = band_lout_off(NPC), DX_OFF = band_dx_off(NPC), DR_OFF = band_dr_off(NPC),
                ZERO_OFF = band_zero_off(NPC), EW = band_ew(NPC);
  static_assert(NPC == BAND_NPIECE || NPC == BAND_NPIECE_WIDE, "fifteen or twenty operand pieces");
  constexpr int ES = (int)sizeof(T), LS = ES == 8 ? 3 : 2;   // bytes per element, their log2
  static_assert(ES == 8 || ES == 4, "double or float");
  extern __shared__ double lds[];
  const int mode = Ain.mode, batch = Ain.batch;
  T* const gvals = as_global(static_cast<T*>(Ain.vals));
  const T* const grhs = as_global(static_cast<const T*>(Ain.rhs));
  T* const gd = as_global(static_cast<T*>(Ain.d));
  T* const gL = as_global(static_cast<T*>(Ain.L));
  const int lane = threadIdx.x & 63;
  const int part = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lq = lane >> 3, le = lane & 7;
  const int prob0 = blockIdx.x * NL;
  // MODE_SOLVE = solve_ldl! behind a factorisation of this handle (src/solver_types.jl:69-77): the band kernels keep no factor a later
  // right-hand side could be run through (their six-double records hold z = c / d of the ONE right-hand side they were computed with),
  // so the solve factorises the same values again — the rho slots hold what the ladder left — and sweeps the new right-hand side
  // in the same launch: the arithmetic of the first attempt of newton_system!, no ladder, no outputs but d.
  const bool has_rhs = mode != MODE_FACTOR && grhs != nullptr;
  T* const ldsT = reinterpret_cast<T*>(lds);
  char* wblk = reinterpret_cast<char*>(ldsT + (size_t)part * NL * LANE_D);
  char* recb = reinterpret_cast<char*>(ldsT + (size_t)P.nparts * NL * LANE_D) + (size_t)part * BAND_REC_MAX * 4;
  double* ctrl = reinterpret_cast<double*>(reinterpret_cast<char*>(ldsT + (size_t)P.nparts * NL * LANE_D) + (size_t)P.nparts * BAND_REC_MAX * 4);
  const int* fops_g = as_global(P.fops[part]);
  const int* bops_g = as_global(P.bops[part]);
  cptr epochs = as_const(P.epochs[part]);
  cptr borders = as_const(P.borders[part]);
  const int nepochs = P.nepochs[part];
  const int nnz = P.nnz, N = P.N;
  const long long lsize = P.lsize;
  // mover: wave-uniform base pointers + 32-bit per-lane byte offsets (NL problems span < 4 GB)
  // cnl_options.batch_layout = 1: `vals` is given INTERLEAVED over groups of 32 problems in blocks of eight doubles — element e of
  // problem p of group g at
  // ((g * band_il_blocks(nnz) + e / 8) * 32 + p) * 8 + e % 8 — so that the eight 64-byte runs of a mover load are 512 contiguous bytes
  // and every 128-byte line that is fetched is used whole (16 384 problems: 12.5 -> 11.0 ms with vals and rhs interleaved, bit-equal).
  // Bit 1 of the layout word: the same for `rhs`.  d is problem-major always.
  // (the groups of the LAYOUT are 32 problems whatever the workgroup holds: a workgroup of 16 problems works on half a group)
  constexpr int G8 = BAND_IL_GROUP * 8;
  static_assert(BAND_IL_GROUP % NL == 0, "a workgroup's problems lie in one group of the interleaved layout");
  const bool vil = MOV || (Ain.layout & 1) != 0, ril = (Ain.layout & 2) != 0;
  const int vstride = vil ? G8 : 0, rstride = ril ? G8 : 0;
  const long long ilg = prob0 / BAND_IL_GROUP;        // group of the workgroup's problems
  const int ilp = (prob0 % BAND_IL_GROUP) * 8;        // ... and the offset of its first problem inside a block row
  const T* vbase = gvals + (vil ? ilg * band_il_blocks(nnz) * G8 + ilp : (long long)prob0 * nnz);
  const T* rbase = !has_rhs ? gvals : grhs + (ril ? ilg * band_il_blocks(N) * G8 + ilp : (long long)prob0 * N);
  // The factor records are private to the launch.  32 problems per workgroup: element-major over the workgroup's region, stored by
  // the compute lanes as they are computed (see frec_index; they used to go through the out ring and out with the mover, interleaved
  // in blocks of eight doubles: a record run that does not start on a block boundary wrote its first and last lines in two epochs, and
  // the backward pieces fetched them twice — 16 384 problems: 11.19 -> 10.70 ms).  8 or 16 problems: problem-major,
  // through the out ring.  The mover reads them back in the backward sweep.
  constexpr bool DREC = direct_records(NL);
  T* lbase_g = gL + (long long)prob0 * lsize + (DREC ? 0 : P.loff[part]);
  const int loff8 = DREC ? (int)P.loff[part] : 0;   // a multiple of 8
  T* const recp = lbase_g + (long long)loff8 * NL + (lane < NL ? lane : 0);   // compute lane's first record element (DREC)
  T* dbase = gd ? gd + (long long)prob0 * N : nullptr;
  unsigned movp[NI], ldsb[NI];   // problem of the lane inside the workgroup (clamped to the batch), LDS byte offset of its element
  bool movok[NI];
#pragma unroll
  for (int i = 0; i < NI; i++) {
    int pl = i * 8 + lq;
    movok[i] = prob0 + pl < batch;
    if (!movok[i]) pl = batch - 1 - prob0;
    movp[i] = (unsigned)pl;
    ldsb[i] = ((unsigned)(i * 8 + lq) * (unsigned)LANE_D + (unsigned)le) << LS;
  }
  // mover-table instance: problem group i of a lane lies a constant 8 * i lane blocks behind its group 0, so ONE register and the
  // offset field of the LDS instruction address all four groups (three registers and three additions per committed set less)
#define BAND_LDSB(I) (MOV ? ldsb[0] + (unsigned)((I) * 8 * LANE_D * ES) : ldsb[I])
  static_assert(!MOV || (3 * 8 + 8) * LANE_D * ES < 65536, "a workgroup's lane blocks lie inside the offset field of an LDS instruction");
  // mover-table instance: the lane's byte offset inside an aligned block row of `vals` / inside a factor piece (band.h, BAND_MK_*)
  unsigned movv[NI], movf[NI];
  if constexpr (MOV) {
#pragma unroll
    for (int i = 0; i < NI; i++) {
      movv[i] = (movp[i] * 8u + (unsigned)le) << LS;
      movf[i] = (movp[i] + (unsigned)le * (unsigned)NL) << LS;
    }
    static_assert(!MOV || (NL == BAND_IL_GROUP && BAND_MOV_EL_BYTES == NL * ES), "a typed offset counts rows of NL elements");
  }
  // compute lanes
  const bool clane = lane < NL;
  const int cprob = prob0 + (clane ? lane : 0);
  const bool valid = clane && cprob < batch;
  const int cpl = valid ? cprob - prob0 : batch - 1 - prob0;   // problem whose data this lane's block holds
  char* myb = wblk + (size_t)(clane ? lane : 0) * LANE_D * ES;
  const long long pv = vil ? ilg * band_il_blocks(nnz) * G8 + ilp + cpl * 8 : (long long)(prob0 + cpl) * nnz;
  const long long pr = ril ? ilg * band_il_blocks(N) * G8 + ilp + cpl * 8 : (long long)(prob0 + cpl) * N;
  for (int t = lane; t < NL; t += 64) *reinterpret_cast<T*>(wblk + ((size_t)t * LANE_D + ZERO_OFF) * ES) = T(0);   // every block's zero cell

  const T tol = (T)Ain.params[0], kdec = (T)Ain.params[2], kinc = (T)Ain.params[3], klarge = (T)Ain.params[4], rho0 = (T)Ain.params[5],
          rhomax = (T)Ain.params[6], rhomin = (T)Ain.params[7];
  T rho = T(0), wrote = T(0);
  T rho_old = (mode == MODE_NEWTON && valid) ? as_global(static_cast<T*>(Ain.rho_old))[cprob] : T(0);
  int nfact = 0;
  bool done = !valid, success = false, ovr = false;
  // (try_to_factorize keeps no records: a later solve_ldl! factorises again, see MODE_SOLVE above)
  const bool recst = valid && mode != MODE_FACTOR;   // (DREC)

  static_assert(NI <= 4, "at most four problem groups per mover lane");
  T stg[NPC][NI];        // operand pieces in flight
  int4 rstg0;            // step blocks in flight (one 16-byte word per lane: 256 ints)
  int pcs[NPC];          // piece descriptors of the epoch being loaded
  static_assert(BAND_REC_MAX <= 256, "record buffer: one dwordx4 per lane");
  // The mover is written for back-to-back issue: the NPC piece descriptors of an epoch come with one scalar load, unused
  // pieces are skipped with a wave-uniform branch (a load that hits in cache costs the CU's memory pipeline what any other costs),
  // every staged piece is written to LDS whether used or not (resident form: used pieces only, each to the slot its descriptor names).  One load per piece and problem group: base pointer and stride of the
  // piece's array are selected with scalar instructions, the lane's offset is problem * stride + element.  (Three guarded loads
  // made the compiler form all three 64-bit addresses of every piece up front — 96 NI VGPRs; selecting among per-array offset
  // arrays made it index them in scratch memory; lambdas instead of macros put every captured variable into scratch.)
#define BAND_ISSUE1(K, I) if constexpr (I < NI) stg[K][I] = *reinterpret_cast<const T*>(pb + ((movp[I] * strd + tl) << LS));
#define BAND_COMMIT1(K, I) if constexpr (I < NI) *reinterpret_cast<T*>(wblk + ldsb[I] + (BAND_IN_OFF + 8 * K) * ES) = stg[K][I];
  /* resident form: to the descriptor's slot (wave-uniform) */
#define BAND_COMMITR1(K, I) if constexpr (I < NI) *reinterpret_cast<T*>(wslot_ + BAND_LDSB(I)) = stg[K][I];
#define BAND_ISSUE_GEN(K)                                                                                                     \
  if (pcs[K] >= 0) {   /* (wave-uniform) */                                                                                   \
    const int pc = pcs[K];                                                                                                    \
    const int arr = pc >> 28;                                                                                                 \
    const int el_ = (pc & ((1 << DBITS) - 1)) + (arr == 2 ? loff8 : 0);                                                          \
    /* lane offset (elements) = problem * strd + tl, tl = t * tm + (t >> 3) * gap with t = m + element of the lane: the caller's    \
       arrays are problem-major (m = 0, t < 8: gap = 0) or interleaved in blocks of eight, the factor is element-major (see        \
       lbase_g: a row of NL elements per record element, tm = NL) or problem-major (DREC false) */                           \
    const bool il_ = arr == 0 ? vil : arr == 1 ? ril : DREC;   /* (wave-uniform) */                                           \
    const int ilw_ = arr == 2 ? NL * 8 : BAND_IL_GROUP * 8;    /* elements per block row: the factor's own layout / the ABI's */ \
    const int m_ = il_ ? (el_ & 7) : 0;                                                                                       \
    const unsigned gap_ = il_ && !(DREC && arr == 2) ? (unsigned)(ilw_ - 8) : 0u;                                              \
    const unsigned tm_ = arr == 2 && DREC ? (unsigned)NL : 1u;                                                                \
    const char* pb = (arr == 0 ? reinterpret_cast<const char*>(vbase) : arr == 1 ? reinterpret_cast<const char*>(rbase)       \
                                                                                 : reinterpret_cast<const char*>(lbase_g)) +   \
                     ((il_ ? (long long)(el_ >> 3) * ilw_ : (long long)el_) << LS);                                           \
    const unsigned strd = DREC ? (arr == 2 ? 1u : il_ ? 8u : arr == 0 ? (unsigned)nnz : (unsigned)N)                         \
                               : (il_ ? 8u : arr == 0 ? (unsigned)nnz : arr == 1 ? (unsigned)N : (unsigned)lsize);             \
    const unsigned t_ = (unsigned)m_ + (unsigned)le;                                                                          \
    const unsigned tl = t_ * tm_ + (t_ >> 3) * gap_;                                                                          \
    BAND_ISSUE1(K, 0) BAND_ISSUE1(K, 1) BAND_ISSUE1(K, 2) BAND_ISSUE1(K, 3)                                                   \
  }
  /* mover-table instance, typed set: the word is  byte offset | slot  (negative: unused) */
  // NT: the set's stream is read once per sweep and its loads are non-temporal under the instance's cache policy (a typed piece is
  // whole lines; general sets — rhs halves of a line, packed pieces — stay plain under every policy)
#define BAND_ISSUET1(K, I, VO, NT)                                                                                            \
  if constexpr (I < NI) {                                                                                                     \
    if constexpr ((POL & (NT)) != 0) stg[K][I] = __builtin_nontemporal_load(reinterpret_cast<const T*>(pb + VO[I]));          \
    else stg[K][I] = *reinterpret_cast<const T*>(pb + VO[I]);                                                                 \
  }
#define BAND_ISSUET(K, BASE, VO, NT)                                                                                          \
  if (pcs[K] >= 0) {   /* (wave-uniform) */                                                                                   \
    const char* pb = reinterpret_cast<const char*>(BASE) + (unsigned)(pcs[K] & ~BAND_MOV_SLOT_MASK);                          \
    BAND_ISSUET1(K, 0, VO, NT) BAND_ISSUET1(K, 1, VO, NT) BAND_ISSUET1(K, 2, VO, NT) BAND_ISSUET1(K, 3, VO, NT)               \
  }
  /* SW: the sweep (0 forward, 1 backward) — the kind of set K is band_mover_kind(SW, K); one code path per set */
#define BAND_ISSUE(K, SW)                                                                                                     \
  if constexpr (MOV && band_mover_kind(SW, K) == BAND_MK_VALS) { BAND_ISSUET(K, vbase, movv, BAND_POL_VALS_NT) }              \
  else if constexpr (MOV && band_mover_kind(SW, K) == BAND_MK_FACTOR) { BAND_ISSUET(K, lbase_g, movf, BAND_POL_FACTOR_NT) }   \
  else { BAND_ISSUE_GEN(K) }
  /* (at commit time pcs[] still holds the descriptors of the epoch being committed: the next epoch's are read behind the commit) */
#define BAND_COMMIT(K, SW)                                                                                                    \
  if constexpr (RES) {                                                                                                        \
    if (pcs[K] >= 0) {                                                                                                        \
      const int sl_ = MOV && band_mover_kind(SW, K) != BAND_MK_GENERAL ? pcs[K] & BAND_MOV_SLOT_MASK : (pcs[K] >> BAND_RES_SLOT_SHIFT) & 31; \
      char* wslot_ = wblk + (BAND_IN_OFF + 8 * sl_) * ES;                                                                     \
      BAND_COMMITR1(K, 0) BAND_COMMITR1(K, 1) BAND_COMMITR1(K, 2) BAND_COMMITR1(K, 3)                                         \
    }                                                                                                                         \
  } else { BAND_COMMIT1(K, 0) BAND_COMMIT1(K, 1) BAND_COMMIT1(K, 2) BAND_COMMIT1(K, 3) }
  // (macros, not lambdas: a closure made the compiler keep every captured variable — the staging registers included — in scratch memory)
#define BAND_ISSUE_DESC(EP, OFS) { cptr E_ = (EP) + (OFS); _Pragma("unroll") for (int k_ = 0; k_ < NPC; k_++) pcs[k_] = E_[k_]; }
  /* the epoch's step / row blocks (the streams are padded: reading past the epoch's blocks is harmless) */
#define BAND_ISSUE_REC(OPS, OPOFF) { rstg0 = (reinterpret_cast<const int4*>((OPS) + (OPOFF)) + lane)[0]; }
#define BAND_ISSUE_ALL(EP, OFS, OPS, OPOFF, SW)                                                                                   \
  {                                                                                                                           \
    BAND_ISSUE_DESC(EP, OFS)                                                                                                  \
    BAND_ISSUE(0, SW) BAND_ISSUE(1, SW) BAND_ISSUE(2, SW) BAND_ISSUE(3, SW) BAND_ISSUE(4, SW) BAND_ISSUE(5, SW) BAND_ISSUE(6, SW) BAND_ISSUE(7, SW)           \
    BAND_ISSUE(8, SW) BAND_ISSUE(9, SW) BAND_ISSUE(10, SW) BAND_ISSUE(11, SW) BAND_ISSUE(12, SW) BAND_ISSUE(13, SW) BAND_ISSUE(14, SW)                    \
    if constexpr (NPC > 15) { BAND_ISSUE(15, SW) BAND_ISSUE(16, SW) BAND_ISSUE(17, SW) BAND_ISSUE(18, SW) BAND_ISSUE(19, SW) }                    \
    BAND_ISSUE_REC(OPS, OPOFF)                                                                                                \
  }
  /* mover-table instance: ONE wait for everything in flight (vmcnt 0, the other counters open) in front of the commit.  The loads  \
     are issued under wave-uniform branches, so the compiler cannot count them and waits in front of every ds_write of every set —   \
     sixty waits, of which the first (all but the newest three operations) already drains the queue.  Behind this one it places none. */ \
#define BAND_COMMIT_ALL(SW)                                                                                                     \
  {                                                                                                                           \
    if constexpr (MOV) __builtin_amdgcn_s_waitcnt(BAND_WAIT_VM0);                                                             \
    BAND_COMMIT(0, SW) BAND_COMMIT(1, SW) BAND_COMMIT(2, SW) BAND_COMMIT(3, SW) BAND_COMMIT(4, SW) BAND_COMMIT(5, SW) BAND_COMMIT(6, SW) BAND_COMMIT(7, SW)   \
    BAND_COMMIT(8, SW) BAND_COMMIT(9, SW) BAND_COMMIT(10, SW) BAND_COMMIT(11, SW) BAND_COMMIT(12, SW) BAND_COMMIT(13, SW) BAND_COMMIT(14, SW)             \
    if constexpr (NPC > 15) { BAND_COMMIT(15, SW) BAND_COMMIT(16, SW) BAND_COMMIT(17, SW) BAND_COMMIT(18, SW) BAND_COMMIT(19, SW) }               \
    reinterpret_cast<int4*>(recb)[lane] = rstg0;                                                                              \
  }
  // the next epoch's loads go out in four groups behind the first four steps of the current one: 4 + 4 + 4 + 3 pieces, 5 + 5 + 5 + 5 in
  // the wide form; the last group takes the step blocks along
#define BAND_ISSUE_G0(SW)                                                                                                       \
  if constexpr (NPC > 15) { BAND_ISSUE(0, SW) BAND_ISSUE(1, SW) BAND_ISSUE(2, SW) BAND_ISSUE(3, SW) BAND_ISSUE(4, SW) }                           \
  else { BAND_ISSUE(0, SW) BAND_ISSUE(1, SW) BAND_ISSUE(2, SW) BAND_ISSUE(3, SW) }
#define BAND_ISSUE_G1(SW)                                                                                                       \
  if constexpr (NPC > 15) { BAND_ISSUE(5, SW) BAND_ISSUE(6, SW) BAND_ISSUE(7, SW) BAND_ISSUE(8, SW) BAND_ISSUE(9, SW) }                           \
  else { BAND_ISSUE(4, SW) BAND_ISSUE(5, SW) BAND_ISSUE(6, SW) BAND_ISSUE(7, SW) }
#define BAND_ISSUE_G2(SW)                                                                                                       \
  if constexpr (NPC > 15) { BAND_ISSUE(10, SW) BAND_ISSUE(11, SW) BAND_ISSUE(12, SW) BAND_ISSUE(13, SW) BAND_ISSUE(14, SW) }                      \
  else { BAND_ISSUE(8, SW) BAND_ISSUE(9, SW) BAND_ISSUE(10, SW) BAND_ISSUE(11, SW) }
#define BAND_ISSUE_G3(SW)                                                                                                       \
  if constexpr (NPC > 15) { BAND_ISSUE(15, SW) BAND_ISSUE(16, SW) BAND_ISSUE(17, SW) BAND_ISSUE(18, SW) BAND_ISSUE(19, SW) }                      \
  else { BAND_ISSUE(12, SW) BAND_ISSUE(13, SW) BAND_ISSUE(14, SW) }

  // mover-table instance, EPOCH-BLOCK LOOK-AHEAD: no field of an epoch block is fetched where it is needed.  With the last issue
  // group of an epoch, lanes 0 .. EW-1 load word `lane` of the block TWO epochs ahead into ebk (one VGPR) — a vector load among the
  // mover's, which the commit's wait retires; behind the commit v_readlane hands out the NEXT epoch's mover words and step-block
  // offset, and the next epoch's own fields (steps, record bases, solution ranges), which wait in SGPRs for a turn of the loop
  // (*N below).  So ebk is free again before the load that refills it, and neither sweep holds a scalar load outside the border
  // pivots: a lone wavefront per SIMD stood through each of their round trips (five per epoch pair, each waited for on the spot),
  // and while one was pending every LDS wait was a wait for all.  Both ends of a sweep clamp the block index, and every rung of
  // the ladder primes ebk and the *N anew.
  const int* const epochs_g = as_global(P.epochs[part]);
  int ebk = 0, nstN = 0, lb1N = 0, lb2N = 0, xloN = 0, xcN = 0, rloN = 0, rcN = 0, roffN = 0;
  /* (the lane number is formed anew at each load, by an asm the compiler does not move: kept in a register through the loops it  \
     would push one more value into scratch) */                                                                                  \
#define BAND_EBK_LOAD(B)                                                                                                         \
  {                                                                                                                              \
    int el_;                                                                                                                     \
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(el_));                                   \
    ebk = epochs_g[(B) * EW + (el_ < EW ? el_ : EW - 1)];                                                                        \
  }
#define BAND_EBK(F) __builtin_amdgcn_readlane(ebk, EF(F))
#define BAND_EBK_DESC(F0) { _Pragma("unroll") for (int k_ = 0; k_ < NPC; k_++) pcs[k_] = __builtin_amdgcn_readlane(ebk, EF(F0) + k_); }
  constexpr int BAND_WAIT_VM0 = 0x0F70;   // s_waitcnt vmcnt(0): vmcnt = bits 15:14 and 3:0, expcnt (6:4) and lgkmcnt (11:8) at their maxima

  Win<T> W;
  int npos = 0, nzer = 0;
  T lj[6], zj[4];   // junction factor (first wavefront)
  for (int q = 0; q < 6; q++) lj[q] = T(0);
  for (int q = 0; q < 4; q++) zj[q] = T(0);
  while (true) {
    // ================= forward: assembly, elimination, forward substitution =================
#pragma unroll
    for (int q = 0; q < NS * (NS + 1) / 2; q++) W.S[q] = T(0);
#pragma unroll
    for (int q = 0; q < NS; q++) { W.X[q] = T(0); W.c[q] = T(0); }
    W.S55 = T(0); W.c5 = T(0);
    npos = 0; nzer = 0;
    BAND_ISSUE_ALL(epochs, EF(BE_FP), fops_g, 0, 0)
    if constexpr (MOV) {
      nstN = epochs[EF(BE_NSTEP)]; lb1N = epochs[EF(BE_LBASE)]; lb2N = epochs[EF(BE_LBASE2)];
      BAND_EBK_LOAD(nepochs > 1 ? 1 : 0)
    }
    for (int e = 0; e < nepochs; e++) {
      cptr E = epochs + e * EW;
      BAND_COMMIT_ALL(0)
      // the next epoch's loads are issued in four groups behind the first four steps (a burst of 34 loads stalled the wavefront on
      // the CU's memory pipeline for ~2 500 cycles per epoch, in-kernel stamps), still four steps ahead of their use
      const bool more_ = e + 1 < nepochs;
      if constexpr (!MOV) { if (more_) BAND_ISSUE_DESC(epochs + (e + 1) * EW, EF(BE_FP)) }
      // The steps of the epoch: step t works on the slots of phase t (every epoch but the last has BAND_EPOCH steps), so the eight
      // instantiations follow each other in straight-line code and the window keeps its registers from step to step.
      // first record element of each half of the epoch, less the out ring's offset that the program's BS_LB / BS_LX carry
      int nst, recb1, recb2;
      if constexpr (MOV) {
        // (ebk holds the block of epoch e + 1, or of the last epoch again)
        nst = nstN; recb1 = lb1N - LOUT_OFF; recb2 = lb2N - LOUT_OFF;
        BAND_EBK_DESC(BE_FP)
        roffN = BAND_EBK(BE_FOFF); nstN = BAND_EBK(BE_NSTEP); lb1N = BAND_EBK(BE_LBASE); lb2N = BAND_EBK(BE_LBASE2);
      } else {
        nst = E[EF(BE_NSTEP)]; recb1 = E[EF(BE_LBASE)] - LOUT_OFF; recb2 = E[EF(BE_LBASE2)] - LOUT_OFF;
      }
      int o = 0;
      // the blocks of step t + 1 (step block + first row block) are read from the record buffer while step t computes; the step
      // reads all its operands at its top (one LDS round trip).  (A third stage — operands a step ahead — was measured: no gain,
      // 170 more registers.)
      Rec stC, stN;
      RowRec rwC, rwN;
      load_rec<MOV>(stC, recb, 0);
      load_row<MOV>(rwC, recb, BAND_SW);
#define BAND_FSTEP(PHV)                                                                                                     \
      if (PHV < nst) {                                                                                                      \
        const int fl = __builtin_amdgcn_readfirstlane(stC.v[BS_FLAGS]);                                                     \
        const int onext = o + BAND_SW + BAND_RW * ((fl >> 8) & 255);                                                        \
        if (PHV + 1 < nst) { load_rec<MOV>(stN, recb, onext); load_row<MOV>(rwN, recb, onext + BAND_SW); }                            \
        if (clane) {                                                                                                        \
          FOps<T> op_;                                                                                                      \
          fload(op_, stC, rwC, fl, myb);                                                                                    \
          fstep<PHV, NL, POL>(W, op_, stC, fl, recb, o, myb, gvals, grhs, borders, pv, pr, has_rhs, rho, ovr, tol, npos, nzer, vstride, rstride, \
                         recp, PHV < BAND_EPOCH / 2 ? recb1 : recb2, recst);                                              \
        }                                                                                                                   \
        o = onext; stC = stN; rwC = rwN;                                                                                    \
      }
      // mover-table instance (BAND_FSTEP_X): the two sets of block registers alternate by step parity — the step of phase PH reads set
      // PH % 2 (SC / RC) and loads the next step's blocks into the other (SN / RN) — instead of being copied behind every step: the
      // copies were about 270 v_mov per forward epoch, on a kernel that instruction issue bounds
#define BAND_FSTEP_P(PHV, SC, SN, RC, RN)                                                                                   \
      if (PHV < nst) {                                                                                                      \
        const int fl = __builtin_amdgcn_readfirstlane(SC.v[BS_FLAGS]);                                                      \
        const int onext = o + BAND_SW + BAND_RW * ((fl >> 8) & 255);                                                        \
        if (PHV + 1 < nst) { load_rec<MOV>(SN, recb, onext); load_row<MOV>(RN, recb, onext + BAND_SW); }                              \
        if (clane) {                                                                                                        \
          FOps<T> op_;                                                                                                      \
          fload(op_, SC, RC, fl, myb);                                                                                      \
          fstep<PHV, NL, POL>(W, op_, SC, fl, recb, o, myb, gvals, grhs, borders, pv, pr, has_rhs, rho, ovr, tol, npos, nzer, vstride, rstride, \
                         recp, PHV < BAND_EPOCH / 2 ? recb1 : recb2, recst);                                              \
        }                                                                                                                   \
        o = onext;                                                                                                          \
      }
#define BAND_FSTEP_X(PHV) if constexpr (MOV) { if constexpr (PHV % 2 == 0) { BAND_FSTEP_P(PHV, stC, stN, rwC, rwN) } else { BAND_FSTEP_P(PHV, stN, stC, rwN, rwC) } } else { BAND_FSTEP(PHV) }
      // !DREC: the out ring holds the factor records of half an epoch; whole pieces are read from it (all reads first), lanes past
      // the records do not store
#define BAND_LFLUSH(LB, LC)                                                                                                 \
      if constexpr (!DREC) {                                                                                                \
        if (mode != MODE_FACTOR) {                                                                                          \
          const int lc_ = (LC);                                                                                             \
          char* lout = reinterpret_cast<char*>(lbase_g) + ((long long)(LB) << LS);                                          \
          T lx_[BAND_LOUT_MAX / 8][NI];                                                                                     \
          _Pragma("unroll") for (int cpc = 0; cpc < BAND_LOUT_MAX / 8; cpc++)                                               \
            _Pragma("unroll") for (int i = 0; i < NI; i++) lx_[cpc][i] = *reinterpret_cast<const T*>(wblk + ldsb[i] + (LOUT_OFF + 8 * cpc) * ES); \
          _Pragma("unroll") for (int cpc = 0; cpc < BAND_LOUT_MAX / 8; cpc++)                                               \
            _Pragma("unroll") for (int i = 0; i < NI; i++)                                                                  \
              if (movok[i] && cpc * 8 + le < lc_)                                                                           \
                *reinterpret_cast<T*>(lout + (((movp[i] * (unsigned)lsize + (unsigned)le) << LS) + 8 * ES * cpc)) = lx_[cpc][i]; \
        }                                                                                                                   \
      }
      BAND_FSTEP_X(0)
      if (more_) { BAND_ISSUE_G0(0) }
      BAND_FSTEP_X(1)
      if (more_) { BAND_ISSUE_G1(0) }
      BAND_FSTEP_X(2)
      if (more_) { BAND_ISSUE_G2(0) }
      BAND_FSTEP_X(3)
      if constexpr (MOV) { if (more_) { BAND_ISSUE_G3(0) BAND_ISSUE_REC(fops_g, roffN) BAND_EBK_LOAD(e + 2 < nepochs ? e + 2 : nepochs - 1) } }
      else if (more_) { BAND_ISSUE_G3(0) BAND_ISSUE_REC(fops_g, epochs[(e + 1) * EW + EF(BE_FOFF)]) }
      BAND_LFLUSH(E[EF(BE_LBASE)], E[EF(BE_LCNT)])
      BAND_FSTEP_X(4) BAND_FSTEP_X(5) BAND_FSTEP_X(6) BAND_FSTEP_X(7)
      static_assert(BAND_EPOCH == 8, "eight step instantiations per epoch");
      if (nst == BAND_EPOCH) {
        // behind a full epoch the slots 0 .. 3 are dead (pivoted in phases 4 .. 7): give them a constant, so that only the ten
        // entries among the live slots, their border row and right-hand side are carried from epoch to epoch (the junction
        // behind the loop reads every entry, which would otherwise keep all 52 in registers through the whole sweep)
#pragma unroll
        for (int a = 0; a < NS; a++)
#pragma unroll
          for (int b = 0; b <= a; b++)
            if (b < 4) W.S[sidx(a, b)] = T(0);
#pragma unroll
        for (int a = 0; a < 4; a++) { W.X[a] = T(0); W.c[a] = T(0); }
      }
      BAND_LFLUSH(E[EF(BE_LBASE2)], E[EF(BE_LCNT2)])
    }
    // ================= junction + inertia rule + rho ladder (src/solver_types.jl:90-97, src/CaNNOLeS.jl:1023-1047) ==========
    int tpos = npos, tzer = nzer;
    if (P.nparts == 2) {
      // windows to LDS (slot order): the junction reads both with run-time slot numbers
      if (clane) {
        T* ex = reinterpret_cast<T*>(myb + EXCH_OFF * ES);
#pragma unroll
        for (int q = 0; q < NS * (NS + 1) / 2; q++) ex[q] = W.S[q];
#pragma unroll
        for (int q = 0; q < NS; q++) ex[36 + q] = W.c[q];
        ex[44] = (T)npos; ex[45] = (T)nzer;
      }
      __syncthreads();
      if (part == 0 && clane) {
        const T* exL = reinterpret_cast<const T*>(myb + EXCH_OFF * ES);
        const T* exR = reinterpret_cast<const T*>(myb + (size_t)NL * LANE_D * ES + EXCH_OFF * ES);
        const int tL = P.m0 % NS, tR = (P.n - 1 - P.m0) % NS;
        T SJ[10], cJ[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int aL = (tL + i) % NS, aR = (tR - i + NS) % NS;
#pragma unroll
          for (int j = 0; j <= i; j++) {
            const int bL = (tL + j) % NS, bR = (tR - j + NS) % NS;
            const int iL = aL >= bL ? aL * (aL + 1) / 2 + bL : bL * (bL + 1) / 2 + aL;
            const int iR = aR >= bR ? aR * (aR + 1) / 2 + bR : bR * (bR + 1) / 2 + aR;
            SJ[i * (i + 1) / 2 + j] = exL[iL] + exR[iR];
          }
          cJ[i] = exL[36 + aL] + exR[36 + aR];
        }
        tpos += (int)exR[44]; tzer += (int)exR[45];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const T d = SJ[sidx(i, i)];
          tpos += d > tol;
          tzer += fabs(d) <= tol;
          const T r = rrcp(d);
          zj[i] = rdiv(cJ[i], d, r);
          T w[4];
#pragma unroll
          for (int a = i + 1; a < 4; a++) { w[a] = SJ[sidx(a, i)]; lj[sidx(a - 1, i)] = rdiv(w[a], d, r); }
#pragma unroll
          for (int a = i + 1; a < 4; a++) {
#pragma unroll
            for (int b = i + 1; b <= a; b++) SJ[sidx(a, b)] = fma(w[a], -lj[sidx(b - 1, i)], SJ[sidx(a, b)]);
            cJ[a] = fma(w[a], -zj[i], cJ[a]);
          }
        }
      }
    }
    bool alldone = true;
    if (part == 0) {
      const bool ok = tpos == P.nvar && tzer == 0;
      if (mode == MODE_FACTOR) {
        if (valid) {
          as_global(Ain.success)[cprob] = ok ? 1 : 0;
          if (Ain.npos) as_global(Ain.npos)[cprob] = tpos;
          if (Ain.nzero) as_global(Ain.nzero)[cprob] = tzer;
        }
        done = true;
      } else if (mode == MODE_SOLVE) {
        success = ok;   // (a problem whose factorisation fails the inertia rule has no factor: its rows of d stay untouched)
        done = true;
      } else if (!done) {
        nfact++;
        if (ok) { done = true; success = true; }
        else if (nfact == 1) {
          rho = rho_old == T(0) ? rho0 : fmax(rhomin, kdec * rho_old);
          ovr = true; wrote = rho;
        } else if (rho <= rhomax) {
          rho = rho_old == T(0) ? klarge * rho : kinc * rho;
          if (rho <= rhomax) wrote = rho; else done = true;
        } else done = true;
      }
      alldone = __all(done || !clane);
      if (clane) { ctrl[lane] = rho; ctrl[NL + lane] = (ovr ? 1.0 : 0.0) + (success ? 2.0 : 0.0); }
      if (lane == 0) ctrl[2 * NL] = alldone ? 1.0 : 0.0;
    }
    if (P.nparts == 2) {
      __syncthreads();
      if (part == 1) {
        if (clane) { rho = (T)ctrl[lane]; const int f = (int)ctrl[NL + lane]; ovr = f & 1; success = f & 2; }
        alldone = ctrl[2 * NL] != 0.0;
      }
      __syncthreads();   // the control block is rewritten by the next rung
    }
    if (alldone) break;
  }
  if (mode == MODE_FACTOR) {
    if (mode == MODE_NEWTON && part == 0 && valid) as_global(Ain.success)[cprob] = 1;
    return;
  }
  // ================= backward: d = -K^-1 rhs where the factorisation succeeded =================
  {
    T xs[NS + 1];
#pragma unroll
    for (int q = 0; q < NS + 1; q++) xs[q] = T(0);
    if (P.nparts == 2) {
      if (part == 0 && clane) {
        T xj[4];
        xj[3] = zj[3];
        xj[2] = fma(-lj[sidx(2, 2)], xj[3], zj[2]);
        xj[1] = fma(-lj[sidx(2, 1)], xj[3], fma(-lj[sidx(1, 1)], xj[2], zj[1]));
        xj[0] = fma(-lj[sidx(2, 0)], xj[3], fma(-lj[sidx(1, 0)], xj[2], fma(-lj[sidx(0, 0)], xj[1], zj[0])));
        T* ex = reinterpret_cast<T*>(myb + EXCH_OFF * ES);
        T* exR = reinterpret_cast<T*>(myb + (size_t)NL * LANE_D * ES + EXCH_OFF * ES);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          ex[i] = xj[i]; exR[i] = xj[i];
          if (valid && success) d_store<POL>(gd + ((long long)cprob * N + P.m0 + i), -xj[i]);
        }
      }
      __syncthreads();
      if (clane) {
        const T* ex = reinterpret_cast<const T*>(myb + EXCH_OFF * ES);
        const int t0 = part == 0 ? P.m0 % NS : (P.n - 1 - P.m0) % NS;
#pragma unroll
        for (int s = 0; s < NS; s++) {
          // junction variable i sits in slot (t0 + i) % 8 (first part) / (t0 - i) % 8 (second part)
          const int i = part == 0 ? (s - t0 + NS) % NS : (t0 - s + NS) % NS;
          xs[s] = i < 4 ? ex[i] : T(0);
        }
      }
    }
    // which problems store: flags of the workgroup in the control block
    if (part == 0 && clane) ctrl[NL + lane] = (valid && success) ? 2.0 : 0.0;
    __syncthreads();
    bool movst[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) movst[i] = movok[i] && ctrl[NL + i * 8 + lq] != 0.0;
    const bool okme = valid && ctrl[NL + lane % NL] != 0.0 && clane;
    const long long pd = (long long)(prob0 + cpl) * N;
    BAND_ISSUE_ALL(epochs + (nepochs - 1) * EW, EF(BE_BP), bops_g, 0, 1)
    if constexpr (MOV) {
      cptr EL = epochs + (nepochs - 1) * EW;
      nstN = EL[EF(BE_NSTEP)]; xloN = EL[EF(BE_DXLO)]; xcN = EL[EF(BE_DXCNT)]; rloN = EL[EF(BE_DRLO)]; rcN = EL[EF(BE_DRCNT)];
      BAND_EBK_LOAD(nepochs > 1 ? nepochs - 2 : 0)
    }
    for (int e = nepochs - 1; e >= 0; e--) {
      cptr E = epochs + e * EW;
      BAND_COMMIT_ALL(1)
      const bool more_ = e > 0;
      int nst, xlo, xc, rlo, rc;
      if constexpr (MOV) {
        // (ebk holds the block of epoch e - 1, or of epoch 0 again)
        nst = nstN; xlo = xloN; xc = xcN; rlo = rloN; rc = rcN;
        BAND_EBK_DESC(BE_BP)
        roffN = BAND_EBK(BE_BOFF); nstN = BAND_EBK(BE_NSTEP);
        xloN = BAND_EBK(BE_DXLO); xcN = BAND_EBK(BE_DXCNT); rloN = BAND_EBK(BE_DRLO); rcN = BAND_EBK(BE_DRCNT);
      } else {
        if (more_) BAND_ISSUE_DESC(epochs + (e - 1) * EW, EF(BE_BP))
        nst = E[EF(BE_NSTEP)];
      }
      int o = 0;
      Rec stC, stN;
      RowRec rwC, rwN;
      // (mover-table instance: the step of phase PH reads its blocks from set PH % 2, and the first step of the epoch is nst - 1)
      if (!MOV || (nst & 1)) { load_rec<MOV>(stC, recb, 0); load_row<MOV>(rwC, recb, BAND_SW); }
      else { load_rec<MOV>(stN, recb, 0); load_row<MOV>(rwN, recb, BAND_SW); }
#define BAND_BSTEP(PHV)                                                                                                     \
      if (PHV < nst) {                                                                                                      \
        const int fl = __builtin_amdgcn_readfirstlane(stC.v[BS_FLAGS]);                                                     \
        const int onext = o + BAND_SW + BAND_RW * ((fl >> 8) & 255);                                                        \
        if (PHV > 0) { load_rec<MOV>(stN, recb, onext); load_row<MOV>(rwN, recb, onext + BAND_SW); }                                  \
        if (clane) {                                                                                                        \
          BOps<T> op_;                                                                                                      \
          bload(op_, stC, rwC, fl, myb);                                                                                    \
          bstep<PHV, POL>(xs, op_, stC, rwC, fl, recb, o, myb, borders, gd, pd, okme);                                           \
        }                                                                                                                   \
        o = onext; stC = stN; rwC = rwN;                                                                                    \
      }
#define BAND_BSTEP_P(PHV, SC, SN, RC, RN)                                                                                   \
      if (PHV < nst) {                                                                                                      \
        const int fl = __builtin_amdgcn_readfirstlane(SC.v[BS_FLAGS]);                                                      \
        const int onext = o + BAND_SW + BAND_RW * ((fl >> 8) & 255);                                                        \
        if (PHV > 0) { load_rec<MOV>(SN, recb, onext); load_row<MOV>(RN, recb, onext + BAND_SW); }                                    \
        if (clane) {                                                                                                        \
          BOps<T> op_;                                                                                                      \
          bload(op_, SC, RC, fl, myb);                                                                                      \
          bstep<PHV, POL>(xs, op_, SC, RC, fl, recb, o, myb, borders, gd, pd, okme);                                             \
        }                                                                                                                   \
        o = onext;                                                                                                          \
      }
#define BAND_BSTEP_X(PHV) if constexpr (MOV) { if constexpr (PHV % 2 == 0) { BAND_BSTEP_P(PHV, stC, stN, rwC, rwN) } else { BAND_BSTEP_P(PHV, stN, stC, rwN, rwC) } } else { BAND_BSTEP(PHV) }
      BAND_BSTEP_X(7)
      if (more_) { BAND_ISSUE_G0(1) }
      BAND_BSTEP_X(6)
      if (more_) { BAND_ISSUE_G1(1) }
      BAND_BSTEP_X(5)
      if (more_) { BAND_ISSUE_G2(1) }
      BAND_BSTEP_X(4)
      if constexpr (MOV) { if (more_) { BAND_ISSUE_G3(1) BAND_ISSUE_REC(bops_g, roffN) BAND_EBK_LOAD(e > 2 ? e - 2 : 0) } }
      else if (more_) { BAND_ISSUE_G3(1) BAND_ISSUE_REC(bops_g, epochs[(e - 1) * EW + EF(BE_BOFF)]) }
      BAND_BSTEP_X(3) BAND_BSTEP_X(2) BAND_BSTEP_X(1) BAND_BSTEP_X(0)
      // solution components of the epoch
      if constexpr (!MOV) { xlo = E[EF(BE_DXLO)]; xc = E[EF(BE_DXCNT)]; rlo = E[EF(BE_DRLO)]; rc = E[EF(BE_DRCNT)]; }
      char* dxo = reinterpret_cast<char*>(dbase) + ((long long)xlo << LS);
      char* dro = reinterpret_cast<char*>(dbase) + ((long long)rlo << LS);
      {
        T dx_[NI], dr_[BAND_DR_MAX / 8][NI];
#pragma unroll
        for (int i = 0; i < NI; i++) dx_[i] = *reinterpret_cast<const T*>(wblk + BAND_LDSB(i) + DX_OFF * ES);
#pragma unroll
        for (int cpc = 0; cpc < BAND_DR_MAX / 8; cpc++)
#pragma unroll
          for (int i = 0; i < NI; i++) dr_[cpc][i] = *reinterpret_cast<const T*>(wblk + BAND_LDSB(i) + (DR_OFF + 8 * cpc) * ES);
#pragma unroll
        for (int i = 0; i < NI; i++)
          if (movst[i] && le < xc) d_store<POL>(reinterpret_cast<T*>(dxo + ((movp[i] * (unsigned)N + (unsigned)le) << LS)), dx_[i]);
#pragma unroll
        for (int cpc = 0; cpc < BAND_DR_MAX / 8; cpc++)
#pragma unroll
          for (int i = 0; i < NI; i++)
            if (movst[i] && cpc * 8 + le < rc) d_store<POL>(reinterpret_cast<T*>(dro + (((movp[i] * (unsigned)N + (unsigned)le) << LS) + 8 * ES * cpc)), dr_[cpc][i]);
      }
    }
  }
  // ================= outputs of newton_system! =================
  if (part == 0 && mode == MODE_NEWTON) {
    if (nfact > 1 && rho <= rhomax) rho_old = rho;
    if (valid) {
      as_global(static_cast<T*>(Ain.rho))[cprob] = rho;
      as_global(static_cast<T*>(Ain.rho_old))[cprob] = rho_old;
      as_global(Ain.nfact)[cprob] = nfact;
      as_global(Ain.success)[cprob] = success ? 1 : 0;
    }
    // rho slots of the problems that climbed (src/CaNNOLeS.jl:1031,1038,1044-1046): the last nvar entries of vals
    for (int q = 0; q < NL; q++) {
      const int nf = __builtin_amdgcn_readlane(nfact, q);
      const int vq = __builtin_amdgcn_readlane((int)valid, q);
      if (nf > 1 && vq) {
        T wq;
        if constexpr (ES == 8) wq = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(wrote), q), __builtin_amdgcn_readlane(__double2loint(wrote), q));
        else wq = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wrote), q));
        if (vil) {
          T* vg = gvals + ilg * band_il_blocks(nnz) * G8 + ilp + q * 8;
          for (int i = lane; i < P.nvar; i += 64) vg[band_il_offset(nnz - P.nvar + i, vstride)] = wq;
        } else {
          T* vt = gvals + (long long)(prob0 + q) * nnz + (nnz - P.nvar);
          for (int i = lane; i < P.nvar; i += 64) vt[i] = wq;
        }
      }
    }
  }
}

#undef EF

// The wide instances.  LDS: a Float64 lane block is 193 * 8 = 1 544 bytes, so two parts of 32 problems take 98.8 KB (one workgroup
// per CU), of 16 problems 49.4 KB (three); a Float32 block is 772 bytes.  Registers: stg grows by 5 * NI elements, and
// the Float64 instance of 32 problems, which spills 43 VGPRs at 15 pieces, would spill 148 (508 bytes of scratch, reloads inside the
// epoch loop) — it does not exist: band_wide_has(8, 32) is false and a wide Float64 handle runs 16 problems per workgroup at every
// batch.  The 8-problem wide instances are bounded for one workgroup per SIMD pair instead of two, which keeps them out of scratch.
bool band_wide_has(int esz, int nl) { return nl == 8 || nl == 16 || (nl == 32 && esz == 4); }

size_t band_lds_bytes(int nparts, int nl, int esz, int npiece) {
  return (size_t)nparts * nl * band_lane_elems(npiece) * esz + (2 * (size_t)nl + 8) * sizeof(double) + (size_t)nparts * BAND_REC_MAX * 4;
}

template <class T>
static hipError_t launch_band_t(const BandDev& P, int nl, const LaunchArgs& a, hipStream_t stream, int npiece) {
  if (npiece != BAND_NPIECE && npiece != BAND_NPIECE_WIDE) return hipErrorInvalidConfiguration;
  const bool wide = npiece == BAND_NPIECE_WIDE;
  const size_t ldsb = band_lds_bytes(P.nparts, nl, (int)sizeof(T), npiece);
  const int grid = (a.batch + nl - 1) / nl;
  auto go = [&](auto kern) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_attr_cap((int)ldsb));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * P.nparts), ldsb, stream, P, a);
    return hipGetLastError();
  };
  if (wide) {
    if constexpr (sizeof(T) == 4) { if (nl == 32) return go(band_newton_kernel<T, 32, BAND_NPIECE_WIDE>); }
    if (nl == 16) return go(band_newton_kernel<T, 16, BAND_NPIECE_WIDE>);
    if (nl == 8) return go(band_newton_kernel<T, 8, BAND_NPIECE_WIDE>);
    return hipErrorInvalidConfiguration;
  }
  if (nl == 32) return go(band_newton_kernel<T, 32, BAND_NPIECE>);
  if (nl == 16) return go(band_newton_kernel<T, 16, BAND_NPIECE>);
  if (nl == 8) return go(band_newton_kernel<T, 8, BAND_NPIECE>);
  return hipErrorInvalidConfiguration;
}

// the resident instance (named behind the others: instances are emitted in the order they are first named, and the others keep their
// place in the code object)
static hipError_t launch_band_resident(const BandDev& P, int nl, const LaunchArgs& a, hipStream_t stream, int npiece);

static hipError_t launch_band_mover(const BandDev& P, int nl, const LaunchArgs& a, hipStream_t stream, int npiece, int policy);

hipError_t launch_band(const BandDev& P, int nl, const LaunchArgs& a, hipStream_t stream, int npiece, bool resident, bool mover, int policy) {
  if ((mover && !resident) || (policy && !mover)) return hipErrorInvalidConfiguration;
  return mover ? launch_band_mover(P, nl, a, stream, npiece, policy) : resident ? launch_band_resident(P, nl, a, stream, npiece) : launch_band_t<double>(P, nl, a, stream, npiece);
}
hipError_t launch_band_f32(const BandDev& P, int nl, const LaunchArgs& a, hipStream_t stream, int npiece) { return launch_band_t<float>(P, nl, a, stream, npiece); }

static hipError_t launch_band_resident(const BandDev& P, int nl, const LaunchArgs& a, hipStream_t stream, int npiece) {
  if (nl != 32 || npiece != BAND_NPIECE || !(a.layout & 1)) return hipErrorInvalidConfiguration;
  const size_t ldsb = band_lds_bytes(P.nparts, nl, (int)sizeof(double), npiece);
  auto kern = band_newton_kernel<double, 32, BAND_NPIECE_RESIDENT>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_attr_cap((int)ldsb));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((a.batch + nl - 1) / nl), dim3(64 * P.nparts), ldsb, stream, P, a);
  return hipGetLastError();
}

// the mover-table instance (named last, for the same reason)
// ... and its instances under a cache policy (tuning band_cache_policy, BAND_POL_*), behind it.  BAND_POLICY_MASKS is the list of the
// masks that are built; band_policy_built answers for plan creation.  Measured (tools/time_band_policy.py: masks
// 1, 3, 7, 11, 23, 27 against 0 in one process): 7 — both typed load streams and the record stores non-temporal — is the fastest and
// the library's default; d stores stay plain (non-temporal they cost 6 %: the halves of a line of d meet in L2).  To measure another
// mask, name it here.
#define BAND_POLICY_MASKS(X) X(7)
bool band_policy_built(int policy) {
#define X(M) if (policy == (M)) return true;
  BAND_POLICY_MASKS(X)
#undef X
  return policy == 0;
}
static hipError_t launch_band_mover(const BandDev& P, int nl, const LaunchArgs& a, hipStream_t stream, int npiece, int policy) {
  if (nl != 32 || npiece != BAND_NPIECE || !(a.layout & 1)) return hipErrorInvalidConfiguration;
  const size_t ldsb = band_lds_bytes(P.nparts, nl, (int)sizeof(double), npiece);
  auto kern = band_newton_kernel<double, 32, BAND_NPIECE_MOVER>;
#define X(M) if (policy == (M)) kern = band_newton_kernel<double, 32, band_npcx_mover(M)>;
  BAND_POLICY_MASKS(X)
#undef X
  if (!band_policy_built(policy)) return hipErrorInvalidConfiguration;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_attr_cap((int)ldsb));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((a.batch + nl - 1) / nl), dim3(64 * P.nparts), ldsb, stream, P, a);
  return hipGetLastError();
}

}  // namespace cnl
