// Exercises csrc/batch_arrays.h — the table of a handle's per-problem arrays and the view that moves them to a part of the batch — on
// host buffers, and prints one line per check: tests/test_batch_arrays_cpu.py compares the lines with the ones it holds as literals.
// Host only — the header includes the standard library alone.  Problem b's region of every buffer is filled with the byte b, so the
// first and the last byte of what a view addresses say which problems it covers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../cannoles.jl_amd/csrc/batch_arrays.h"

namespace {

constexpr int B = 9, TASKS = 5, NBUF = 6, NSLOT = NBUF + 2;
const int64_t STRIDE[NBUF] = {1, 4, 8, 12, 4099, 2 * TASKS * (int64_t)sizeof(int)};

// slots of different pointer types, as a handle has them; the last two stay null
struct Owner {
  unsigned char* a1 = nullptr;
  int* a4 = nullptr;
  double* a8 = nullptr;
  void* a12 = nullptr;
  void* odd = nullptr;
  int* cnt = nullptr;
  void* none_v = nullptr;
  int* none_i = nullptr;
  std::vector<void**> slots() {
    return {(void**)&a1, (void**)&a4, (void**)&a8, &a12, &odd, (void**)&cnt, &none_v, (void**)&none_i};
  }
};

std::vector<const unsigned char*> values(Owner& o) {
  std::vector<const unsigned char*> v;
  for (void** s : o.slots()) { const unsigned char* p; std::memcpy(&p, s, sizeof p); v.push_back(p); }
  return v;
}

// every buffer addresses problems [b0, b0 + nb): first byte b0, last byte of the nb-th region b0 + nb - 1; the null slots are null
bool covers(Owner& o, int b0, int nb) {
  const std::vector<const unsigned char*> v = values(o);
  for (int k = 0; k < NBUF; k++)
    if (!v[k] || v[k][0] != b0 || v[k][nb * STRIDE[k] - 1] != b0 + nb - 1) return false;
  return !v[NBUF] && !v[NBUF + 1];
}

void line(const char* what, bool ok) { std::printf("%s: %s\n", what, ok ? "ok" : "FAILED"); }

}  // namespace

int main() {
  using cnl::BatchArrays; using cnl::BatchView;
  std::vector<std::vector<unsigned char>> buf(NBUF);
  for (int k = 0; k < NBUF; k++) {
    buf[k].resize((size_t)(B * STRIDE[k]));
    for (int b = 0; b < B; b++) std::memset(buf[k].data() + b * STRIDE[k], b, (size_t)STRIDE[k]);
  }
  Owner o;
  o.a1 = buf[0].data(); o.a4 = (int*)buf[1].data(); o.a8 = (double*)buf[2].data(); o.a12 = buf[3].data(); o.odd = buf[4].data(); o.cnt = (int*)buf[5].data();
  BatchArrays t;
  bool added = true;
  {
    const std::vector<void**> s = o.slots();
    for (int k = 0; k < NSLOT; k++) added = added && t.add(s[k], k < NBUF ? STRIDE[k] : 16);
  }
  line("add", added && t.size() == NSLOT);
  const std::vector<const unsigned char*> base = values(o);

  { BatchView v(t, 3); line("single view (3, 4)", covers(o, 3, 4)); }
  line("single view restored", values(o) == base);
  { BatchView v(t, 0); line("edge (0, 9)", covers(o, 0, B) && values(o) == base); }
  { BatchView v(t, B - 1); line("edge (8, 1)", covers(o, B - 1, 1)); }
  line("edges restored", values(o) == base);

  {
    BatchView v1(t, 2);
    const std::vector<const unsigned char*> l1 = values(o);
    line("nested level 1 (2, 6)", covers(o, 2, 6));
    {
      BatchView v2(t, 3);
      const std::vector<const unsigned char*> l2 = values(o);
      line("nested level 2 (2 + 3, 3)", covers(o, 5, 3));
      {
        BatchView v3(t, 1);
        line("nested level 3 (2 + 3 + 1, 2)", covers(o, 6, 2));
      }
      line("nested level 3 closed", values(o) == l2 && covers(o, 5, 3));
    }
    line("nested level 2 closed", values(o) == l1 && covers(o, 2, 6));
  }
  line("nested level 1 closed", values(o) == base);

  // two halves, one after the other: each from the unshifted base
  bool halves = true;
  for (int part = 0; part < 2; part++) {
    const int b0 = part ? 5 : 0, nb = part ? 4 : 5;
    halves = halves && values(o) == base;
    BatchView v(t, b0);
    halves = halves && covers(o, b0, nb);
  }
  line("sibling views (0, 5) then (5, 4)", halves && values(o) == base);

  {
    void* extra = buf[0].data();
    const int n = t.size();
    line("add rejects a duplicate slot", !t.add((void**)&o.a8, 8) && !t.add(&o.none_v, 4));
    line("add rejects a zero stride", !t.add(&extra, 0));
    line("add rejects a negative stride", !t.add(&extra, -8));
    line("add rejects a null slot", !t.add(nullptr, 8));
    line("rejections register nothing", t.size() == n && t.add(&extra, 8) && t.size() == n + 1);
    void* more[BatchArrays::kMax] = {};
    bool filled = true;
    for (int k = t.size(); k < BatchArrays::kMax; k++) filled = filled && t.add(&more[k], 8);
    line("add rejects what a full table cannot hold", filled && t.size() == BatchArrays::kMax && !t.add(&more[0], 8));
  }

  // the registrations of a Float64 handle (handle.h: dalloc_batch / register_batch; capi_handle.cpp), from constants in place of the
  // plan's sizes: elements of 8 bytes, ints of 4
  {
    constexpr int64_t esz = 8, lsize = 1000 + 16, gs_doubles = 300 + 64, work_doubles = 222, cstride = 70, N2 = 31, band_lsize = 606, tasks = TASKS;
    struct { void *L, *gs, *scratch, *cbuf, *d2, *Lband; int *xpos, *xzer, *gcnt, *sub_cnt; int32_t* blk_ok; } h{};
    struct { const char* name; void** slot; int64_t stride; } reg[] = {
        {"d_L", &h.L, lsize * esz}, {"d_gs", &h.gs, gs_doubles * esz}, {"d_scratch", &h.scratch, work_doubles * esz},
        {"d_cbuf", &h.cbuf, cstride * esz}, {"d_d2", &h.d2, N2 * esz}, {"d_xpos", (void**)&h.xpos, sizeof(int)}, {"d_xzer", (void**)&h.xzer, sizeof(int)},
        {"d_gcnt", (void**)&h.gcnt, 2 * sizeof(int)}, {"d_blk_ok", (void**)&h.blk_ok, sizeof(int32_t)},
        {"d_sub_cnt", (void**)&h.sub_cnt, 2 * tasks * (int64_t)sizeof(int)}, {"d_Lband", &h.Lband, band_lsize * esz}};
    BatchArrays ht;
    for (const auto& r : reg)
      if (!ht.add(r.slot, r.stride)) { line("handle table", false); return 1; }
    for (int k = 0; k < ht.size(); k++) std::printf("stride %s %lld\n", reg[k].name, (long long)ht[k].stride);
  }
  return 0;
}
