// at2v_hostmem.h — the host ranges a context knows to be pinned (at2v_host_alloc / at2v_host_register, include/at2v.h
// ABI 9). The host-buffer calls ask it, per array and per chunk, whether the bytes they are about to upload lie wholly
// inside one known range: then the DMA upload is submitted from the caller's memory, otherwise the bytes take the
// staging slot. A sorted vector of disjoint ranges, looked up by binary search. Plain C++ with no HIP or HSA dependency:
// the CPU context (which only records ranges) and tests/host/hostmem_host.cpp use the same code.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace at2v {

struct HostRange {
  uintptr_t base = 0;  // the caller's address of the first byte
  size_t len = 0;      // bytes, > 0
  uintptr_t dma = 0;   // what the DMA engine is given for `base` (the runtime's agent address; 0 on a CPU context)
  bool owned = false;  // at2v_host_alloc (freed by at2v_host_free / at2v_destroy), else registered in place
};

class HostRegistry {
 public:
  // false: len == 0, the range wraps the address space, or it overlaps a known range (adjacent ranges do not overlap)
  bool insert(const HostRange& r) {
    if (!insertable(r.base, r.len)) return false;
    v_.insert(first_ending_after(r.base), r);
    return true;
  }
  // whether insert would accept [base, base + len)
  bool insertable(uintptr_t base, size_t len) const {
    if (len == 0 || base + len < base) return false;
    const auto it = first_ending_after(base);
    return it == v_.end() || it->base >= base + len;
  }
  // the range holding every byte of [p, p + len), or nullptr. len == 0 holds no byte: nullptr.
  const HostRange* find(const void* p, size_t len) const {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (len == 0 || a + len < a) return nullptr;
    const auto it = first_ending_after(a);
    if (it == v_.end() || it->base > a || a + len > it->base + it->len) return nullptr;
    return &*it;
  }
  // the range that starts at p (not one that merely holds p), or nullptr
  const HostRange* at(const void* p) const {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const auto it = first_ending_after(a);
    return it != v_.end() && it->base == a ? &*it : nullptr;
  }
  // removes the range that starts at p; false if there is none
  bool remove(const void* p, HostRange* out = nullptr) {
    const HostRange* r = at(p);
    if (!r) return false;
    if (out) *out = *r;
    v_.erase(v_.begin() + (r - v_.data()));
    return true;
  }
  size_t size() const { return v_.size(); }
  const std::vector<HostRange>& ranges() const { return v_; }  // ascending by base

 private:
  // the first range whose end lies above a: the only one that can hold or overlap an address >= a from below
  std::vector<HostRange>::const_iterator first_ending_after(uintptr_t a) const {
    return std::upper_bound(v_.begin(), v_.end(), a,
                            [](uintptr_t x, const HostRange& r) { return x < r.base + r.len; });
  }
  std::vector<HostRange> v_;
};

}  // namespace at2v
