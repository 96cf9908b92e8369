// dense_impl.h — what the two element types of the dense backend share on the host (dense.hip: double, dense_f32.hip: float).
// Internal to those two files.  The device structure (DnDev / DnDevF) and the kernels are per file; everything here is index data,
// allocation, and the hipGraph cache of a handle, and is written once: the setup routines are templates over the device structure,
// whose fields carry the same names in both files and whose element type is read off its pointers.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "dense.h"

namespace cnl {

namespace dn {
constexpr int TS = 64;       // tile order (both element types)
constexpr int TT = TS * TS;  // elements per tile
constexpr int KT = 16;       // rows per chunk of the J'WJ kernels (both element types)
}  // namespace dn

#define DCHK(x)                                                                               \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess) { err = std::string(#x) + ": " + hipGetErrorString(e_); return 4; } \
  } while (0)

// A call is a fixed sequence of ~50 short dependent launches; replayed as a hipGraph the boundary between two of them costs
// ~1.7 us instead of ~2.7 us (tools/microbench.hip).  Graphs are cached per argument set (the pointers are baked in).
struct GraphKey {
  int mode = -1;
  const void* p[10] = {};
  double params[9] = {};
  long long extra = 0;
  bool operator==(const GraphKey& o) const {
    if (mode != o.mode || extra != o.extra) return false;
    for (int i = 0; i < 10; i++) if (p[i] != o.p[i]) return false;
    for (int i = 0; i < 9; i++) if (params[i] != o.params[i]) return false;
    return true;
  }
};
struct GraphEntry { GraphKey key; hipGraphExec_t exec = nullptr; hipGraph_t graph = nullptr; };

// the state of a handle that does not depend on the element type; each file derives its own with the device structure in it
struct DenseState {
  int64_t batch = 1;
  bool f32 = false;  // the float form (dense_f32.hip): dense_run_f32 only
  bool general = false;
  bool factored = false;
  std::vector<void*> allocs;
  std::vector<GraphEntry> graphs;
  hipStream_t cap = nullptr;
  bool use_graph = true;
  bool panel2 = true;  // column-block panel kernel (dn_panel2)
  bool panel2_auto = true;  // ... chosen by batch x tiles (setup_common)
  int misses = 0;  // consecutive calls whose argument set was not cached (a caller that hands over fresh buffers every step)
  virtual ~DenseState() = default;
};

namespace dn {

template <class T>
int dalloc_(DenseState* st, T** p, size_t count, std::string& err, bool zero = false) {
  void* q = nullptr;
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) { err = std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e); return 4; }
  st->allocs.push_back(q);
  if (zero && hipMemset(q, 0, bytes) != hipSuccess) { err = "hipMemset failed"; return 4; }
  *p = (T*)q;
  return 0;
}
template <class T>
int upload_(DenseState* st, const T** p, const std::vector<T>& v, std::string& err) {
  T* q = nullptr;
  int rc = dalloc_(st, &q, v.size(), err);
  if (rc) return rc;
  if (!v.empty() && hipMemcpy(q, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { err = "hipMemcpy failed"; return 4; }
  *p = q;
  return 0;
}

// sizes, tile lists and buffers common to both forms.  panel2_fn / panel2_lds: the column-block panel kernel and the dynamic LDS it
// has to opt in to (nullptr: its LDS is static)
template <class Dev>
int setup_common(DenseState* st, Dev& d, int ns, int nv, int64_t batch, const void* panel2_fn, int panel2_lds, std::string& err) {
  using E = typename std::remove_pointer<decltype(d.S0)>::type;
  d.ns = ns; d.nv = nv; d.T = (ns + TS - 1) / TS; d.nsp = d.T * TS;
  d.nlt = d.T * (d.T + 1) / 2;
  // The column-block panel kernel shortens the latency of a step at the price of T workgroups per problem that each refactorise
  // the diagonal tile with four wavefronts (the one-wavefront kernel: T / 3 workgroups).  It pays while the step is latency-bound:
  // measured crossovers at 96 .. 640 problems of order 256 (T = 4) and at 32 problems of order 1050 (T = 17).
  if (st->panel2_auto) st->panel2 = (long long)batch * d.T <= 512;
  if (st->panel2 && panel2_fn && hipFuncSetAttribute(panel2_fn, hipFuncAttributeMaxDynamicSharedMemorySize, panel2_lds) != hipSuccess) {
    (void)hipGetLastError();
    st->panel2 = false;  // the one-wavefront-per-tile panel kernel needs no opt-in
  }
  std::vector<int> lI, lJ;
  for (int J = 0; J < d.T; J++) for (int I = J; I < d.T; I++) { lI.push_back(I); lJ.push_back(J); }
  int rc;
  if ((rc = upload_(st, &d.lI, lI, err))) return rc;
  if ((rc = upload_(st, &d.lJ, lJ, err))) return rc;
  const size_t B = (size_t)batch, mat = (size_t)d.T * d.T * TT;
  if ((rc = dalloc_(st, &d.S0, B * mat, err, true))) return rc;
  if ((rc = dalloc_(st, &d.S, B * mat, err, true))) return rc;
  if ((rc = dalloc_(st, &d.G, B * mat, err, true))) return rc;
  if ((rc = dalloc_(st, &d.Wn, B * d.T * TT, err, true))) return rc;
  for (E** v : {&d.dv, &d.rsh, &d.y, &d.x})
    if ((rc = dalloc_(st, v, B * d.nsp, err, true))) return rc;
  for (E** v : {&d.part1, &d.part2, &d.partA, &d.partB})
    if ((rc = dalloc_(st, v, B * d.T * d.T * 64, err, true))) return rc;
  if ((rc = dalloc_(st, &d.cnt, B * 4, err, true))) return rc;
  if ((rc = dalloc_(st, &d.st, B, err, true))) return rc;
  return 0;
}

// the residual-block form: sizes, the J'WJ work partition, the H entries per tile, the gather lists and the buffers of J
template <class Dev>
int setup_blocks(DenseState* st, Dev& d, const DensePlan& P, int64_t batch, int syrk_wgs, const void* panel2_fn, int panel2_lds, std::string& err) {
  d.n = P.n; d.m = P.m; d.p = P.p; d.nnz = P.nnz;
  d.mp = ((P.m + 63) / 64) * 64;
  d.Tn = (P.n + TS - 1) / TS; d.npj = d.Tn * TS;
  d.ntl = d.Tn * (d.Tn + 1) / 2;
  d.npos_ok = P.n;
  int rc;
  if ((rc = setup_common(st, d, P.n + P.p, P.n, batch, panel2_fn, panel2_lds, err))) return rc;
  // J'WJ work partition: the (problem, tile, row chunk) space in equal shares, two workgroups per CU
  std::vector<int> sy_tp;
  int npieces = 0;
  {
    d.Tm = (d.Tn + 1) / 2; d.nml = d.Tm * (d.Tm + 1) / 2;
    const long long nch = d.mp / KT, units = (long long)batch * d.nml * nch;
    int nwg = 512;
    if (syrk_wgs > 0) nwg = syrk_wgs;
    nwg = (int)std::min<long long>(nwg, units);
    std::vector<int> wg(nwg + 1, 0), pb, ptl, pc0, pc1;
    for (int w = 0; w < nwg; w++) {
      long long u = units * w / nwg;
      const long long u1 = units * (w + 1) / nwg;
      while (u < u1) {
        const long long tile = u / nch, c0 = u % nch, c1 = std::min(nch, c0 + (u1 - u));
        pb.push_back((int)(tile / d.nml)); ptl.push_back((int)(tile % d.nml)); pc0.push_back((int)c0); pc1.push_back((int)c1);
        u += c1 - c0;
      }
      wg[w + 1] = (int)pb.size();
    }
    npieces = (int)pb.size();
    sy_tp.assign((size_t)batch * d.nml + 1, 0);
    for (int q = 0; q < npieces; q++) sy_tp[(size_t)pb[q] * d.nml + ptl[q] + 1]++;
    for (size_t q = 0; q + 1 < sy_tp.size(); q++) sy_tp[q + 1] += sy_tp[q];  // pieces are generated in (problem, tile, chunk) order
    d.ks = nwg;
    if ((rc = upload_(st, &d.sy_wg, wg, err))) return rc;
    if ((rc = upload_(st, &d.sy_b, pb, err))) return rc;
    if ((rc = upload_(st, &d.sy_tl, ptl, err))) return rc;
    if ((rc = upload_(st, &d.sy_ch0, pc0, err))) return rc;
    if ((rc = upload_(st, &d.sy_ch1, pc1, err))) return rc;
    if ((rc = upload_(st, &d.sy_tp, sy_tp, err))) return rc;
  }
  // H entries grouped by lower tile and unique position, COO order inside a position
  {
    const int64_t ns = d.ns;
    std::vector<int> order(P.hslot.size());
    std::iota(order.begin(), order.end(), 0);
    auto tkey = [&](int e) {
      const int64_t pos = P.hpos[e], i = pos % ns, j = pos / ns;
      const int64_t I = i >> 6, J = j >> 6;
      const int64_t lt = J * d.T - (J * (J - 1)) / 2 + (I - J);
      return (lt << 12) | ((i & 63) + 64 * (j & 63));
    };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return tkey(a) < tkey(b); });
    std::vector<int> ht_ptr(d.nlt + 1, 0), hu_loc, hu_ptr, hslot;
    int64_t prev = -1;
    for (int e : order) {
      const int64_t key = tkey(e);
      if (key != prev) {
        hu_loc.push_back((int)(key & 4095)); hu_ptr.push_back((int)hslot.size());
        ht_ptr[(key >> 12) + 1]++;
        prev = key;
      }
      hslot.push_back(P.hslot[e]);
    }
    hu_ptr.push_back((int)hslot.size());
    for (int t = 0; t < d.nlt; t++) ht_ptr[t + 1] += ht_ptr[t];
    if ((rc = upload_(st, &d.ht_ptr, ht_ptr, err))) return rc;
    if ((rc = upload_(st, &d.hu_loc, hu_loc, err))) return rc;
    if ((rc = upload_(st, &d.hu_ptr, hu_ptr, err))) return rc;
    if ((rc = upload_(st, &d.hslot, hslot, err))) return rc;
  }
  if ((rc = upload_(st, &d.jslot, P.jslot, err))) return rc;
  if ((rc = upload_(st, &d.dslot, P.dslot, err))) return rc;
  const size_t B = (size_t)batch;
  if ((rc = dalloc_(st, &d.Jd, B * d.mp * d.npj, err, true))) return rc;
  if ((rc = dalloc_(st, &d.Jw, B * d.mp * d.npj, err, true))) return rc;
  if ((rc = dalloc_(st, &d.w, B * d.mp, err, true))) return rc;
  if ((rc = dalloc_(st, &d.slab, (size_t)npieces * 4 * TT, err))) return rc;
  if ((rc = dalloc_(st, &d.jxp, B * (d.npj / 32) * d.mp, err))) return rc;
  return 0;
}

// replay the cached graph of this argument set, or capture it first (fallback: plain launches)
template <class F>
int run_cached(DenseState* st, const GraphKey& key, hipStream_t stream, std::string& err, F enqueue) {
  if (!st->use_graph) return enqueue(stream);
  for (auto& g : st->graphs)
    if (g.key == key) {
      st->misses = 0;
      DCHK(hipGraphLaunch(g.exec, stream));
      return 0;
    }
  // Capture + instantiation cost far more than the launches they replace: a caller whose pointers change with every call
  // (fresh device buffers per step) would pay them each time.  After a few misses in a row such a handle stays on plain
  // launches (a hit resets the count, so alternating between a few fixed argument sets keeps its graphs).
  if (++st->misses > 4) return enqueue(stream);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (stream && hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return enqueue(stream);  // the caller captures
  if (!st->cap && hipStreamCreateWithFlags(&st->cap, hipStreamNonBlocking) != hipSuccess) { st->use_graph = false; return enqueue(stream); }
  if (hipStreamBeginCapture(st->cap, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    if (getenv("CNL_VERBOSE")) fprintf(stderr, "[cnl] dense: hipStreamBeginCapture failed, plain launches\n");
    (void)hipGetLastError(); st->use_graph = false; return enqueue(stream);
  }
  const int rc = enqueue(st->cap);
  GraphEntry ge;
  ge.key = key;
  const hipError_t e1 = hipStreamEndCapture(st->cap, &ge.graph);
  if (rc) { if (ge.graph) (void)hipGraphDestroy(ge.graph); return rc; }
  hipError_t e2 = hipSuccess;
  if (e1 != hipSuccess || (e2 = hipGraphInstantiate(&ge.exec, ge.graph, nullptr, nullptr, 0)) != hipSuccess) {
    if (getenv("CNL_VERBOSE")) fprintf(stderr, "[cnl] dense: graph capture failed (%s / %s), plain launches\n", hipGetErrorString(e1), hipGetErrorString(e2));
    (void)hipGetLastError();
    if (ge.graph) (void)hipGraphDestroy(ge.graph);
    st->use_graph = false;
    return enqueue(stream);
  }
  if (st->graphs.size() >= 8) {
    // the evicted graph may still be running on whatever stream its last caller used (the _dev calls are asynchronous):
    // drain the device first (rare: the ninth distinct argument set of a handle)
    (void)hipDeviceSynchronize();
    (void)hipGraphExecDestroy(st->graphs.front().exec);
    (void)hipGraphDestroy(st->graphs.front().graph);
    st->graphs.erase(st->graphs.begin());
  }
  st->graphs.push_back(ge);
  // (tests/test_dense_gpu.py::test_dense_graph_cache_states reads the states of this cache off the line below: keep its wording)
  if (getenv("CNL_VERBOSE")) fprintf(stderr, "[cnl] dense: call sequence captured as a graph (%zu cached)\n", st->graphs.size());
  DCHK(hipGraphLaunch(ge.exec, stream));
  return 0;
}

inline int blocks(long long n) { return (int)((n + 255) / 256); }

// zero `bytes` (a multiple of 16, p 16-byte aligned: whole tiles) with a kernel on `stream` (dense_f32.hip).  Both general forms zero
// S0 with it inside their captured sequence, NOT with hipMemsetAsync: the memset node of a replayed graph was seen to fill with
// something other than zeros.  The kernel lives in dense_f32.hip so that dense.hip's device code stays as it is.
void zero_async(void* p, size_t bytes, hipStream_t stream);

}  // namespace dn

}  // namespace cnl
