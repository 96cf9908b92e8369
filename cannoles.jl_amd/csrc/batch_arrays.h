// batch_arrays.h — the per-problem device arrays of a handle, as a table: one record per array (where the handle keeps its base pointer,
// and the bytes one problem takes of it), and a view that moves every registered pointer to problem b0 for as long as it lives
// (handle.h: dalloc_batch registers, SubBatch opens the view).  Pure host code, standard library only, no allocation:
// tests/c_abi/batch_arrays_table.cpp compiles it alone.
#pragma once
#include <cstdint>
#include <cstring>

namespace cnl {

struct BatchArray {
  void** slot;      // the address of the owner's base pointer (of whatever pointer type: read and written as bytes)
  int64_t stride;   // bytes per problem
};

class BatchArrays {
 public:
  static constexpr int kMax = 16;   // (a handle has 13)
  BatchArrays() = default;
  BatchArrays(const BatchArrays&) = delete;   // (the slots point into ONE owner)
  BatchArrays& operator=(const BatchArrays&) = delete;
  // false — and nothing registered — for a stride that is not positive, a null slot, a slot that is in the table already, a full table
  bool add(void** slot, int64_t bytes_per_problem) {
    if (!slot || bytes_per_problem <= 0 || n_ == kMax) return false;
    for (int k = 0; k < n_; k++)
      if (items_[k].slot == slot) return false;
    items_[n_++] = {slot, bytes_per_problem};
    return true;
  }
  int size() const { return n_; }
  const BatchArray& operator[](int k) const { return items_[k]; }

 private:
  BatchArray items_[kMax] = {};
  int n_ = 0;
};

// Problems [b0, ...) of every registered array: each pointer that is not null is advanced by b0 strides, counted from where it
// points NOW — a view opened inside another one is relative to it —, and put back when the view goes.  An absent array (null) stays
// absent.  Views are closed in the reverse order of their opening (they are scoped objects).
class BatchView {
 public:
  BatchView(const BatchArrays& table, int64_t b0) : table_(table), n_(table.size()) {
    for (int k = 0; k < n_; k++) {
      saved_[k] = load(table[k].slot);
      if (saved_[k]) store(table[k].slot, saved_[k] + b0 * table[k].stride);
    }
  }
  ~BatchView() {
    for (int k = 0; k < n_; k++) store(table_[k].slot, saved_[k]);
  }
  BatchView(const BatchView&) = delete;
  BatchView& operator=(const BatchView&) = delete;

 private:
  // (the slot is an int*, a void*, ... of its owner: copied as bytes, which no pointer type objects to)
  static char* load(void** slot) { char* p; std::memcpy(&p, slot, sizeof p); return p; }
  static void store(void** slot, char* p) { std::memcpy(slot, &p, sizeof p); }
  const BatchArrays& table_;
  const int n_;   // (an array registered while the view is open is not the view's)
  char* saved_[BatchArrays::kMax];
};

}  // namespace cnl
