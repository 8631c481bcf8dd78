// Host test of the pinned-range registry (csrc/at2v_hostmem.h), built with -fsanitize=address,undefined and run as a
// program by tests/test_hostmem_host.py. Addresses are numbers here; nothing is dereferenced.
//   hostmem_host random SEED OPS   OPS random insert / lookup / remove operations against a brute-force list
//   hostmem_host edges             the edge cases of a lookup, one "name ok" line each
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "at2v_hostmem.h"

using at2v::HostRange;
using at2v::HostRegistry;

static const void* P(uintptr_t a) { return reinterpret_cast<const void*>(a); }

struct Brute {
  std::vector<HostRange> v;
  bool overlaps(uintptr_t b, size_t n) const {
    for (const HostRange& r : v)
      if (b < r.base + r.len && r.base < b + n) return true;
    return false;
  }
  const HostRange* find(uintptr_t a, size_t n) const {
    if (n == 0) return nullptr;
    for (const HostRange& r : v)
      if (r.base <= a && a + n <= r.base + r.len) return &r;
    return nullptr;
  }
  bool remove(uintptr_t a) {
    for (size_t i = 0; i < v.size(); ++i)
      if (v[i].base == a) {
        v.erase(v.begin() + (long)i);
        return true;
      }
    return false;
  }
};

static int fail(const char* what, unsigned long op) {
  std::printf("MISMATCH %s at op %lu\n", what, op);
  return 1;
}

static int run_random(unsigned long seed, unsigned long ops) {
  std::mt19937_64 rng(seed);
  HostRegistry reg;
  Brute br;
  // a small address space, so that overlaps, exact fits and neighbours are common
  const uintptr_t kSpace = 4096;
  unsigned long inserts = 0, refused = 0, hits = 0, removes = 0;
  for (unsigned long op = 0; op < ops; ++op) {
    const unsigned kind = (unsigned)(rng() % 8);
    const uintptr_t a = 64 + (uintptr_t)(rng() % kSpace);
    const size_t n = (size_t)(rng() % 96);  // 0 included
    if (kind < 2) {
      HostRange r;
      r.base = a;
      r.len = n;
      r.dma = a + 0x100000;
      r.owned = (rng() & 1) != 0;
      const bool want = n != 0 && !br.overlaps(a, n);
      if (reg.insert(r) != want) return fail("insert", op);
      if (want) br.v.push_back(r), ++inserts;
      else ++refused;
    } else if (kind < 6) {
      const HostRange* g = reg.find(P(a), n);
      const HostRange* w = br.find(a, n);
      if ((g == nullptr) != (w == nullptr)) return fail("find", op);
      if (g && (g->base != w->base || g->len != w->len || g->dma != w->dma || g->owned != w->owned))
        return fail("find range", op);
      if (g) ++hits;
      const HostRange* s = reg.at(P(a));
      bool starts = false;
      for (const HostRange& r : br.v) starts = starts || r.base == a;
      if ((s != nullptr) != starts) return fail("at", op);
    } else {
      // half of the removals aim at the start of a known range
      uintptr_t t = a;
      if (!br.v.empty() && (rng() & 1)) t = br.v[(size_t)(rng() % br.v.size())].base;
      HostRange out;
      const bool want = br.find(t, 1) != nullptr && br.find(t, 1)->base == t;
      const bool got = reg.remove(P(t), &out);
      if (got != want) return fail("remove", op);
      if (got && out.base != t) return fail("remove range", op);
      if (want) br.remove(t), ++removes;
    }
    if (reg.size() != br.v.size()) return fail("size", op);
    const std::vector<HostRange>& rs = reg.ranges();
    for (size_t i = 1; i < rs.size(); ++i)
      if (rs[i - 1].base + rs[i - 1].len > rs[i].base) return fail("order", op);
  }
  std::printf("ops %lu inserts %lu refused %lu hits %lu removes %lu\n", ops, inserts, refused, hits, removes);
  return 0;
}

#define EDGE(name, cond)                          \
  do {                                            \
    const bool ok_ = (cond);                      \
    std::printf("%s %s\n", name, ok_ ? "ok" : "FAILED"); \
    if (!ok_) bad = 1;                            \
  } while (0)

static int run_edges() {
  int bad = 0;
  HostRegistry reg;
  HostRange a;
  a.base = 0x1000;
  a.len = 0x100;
  a.dma = 0x7000;
  EDGE("insert", reg.insert(a));
  EDGE("whole_range", reg.find(P(0x1000), 0x100) != nullptr);
  EDGE("ends_at_end", reg.find(P(0x10f0), 0x10) != nullptr);
  EDGE("one_past_end", reg.find(P(0x10f0), 0x11) == nullptr);
  EDGE("starts_one_before", reg.find(P(0xfff), 2) == nullptr);
  EDGE("first_byte", reg.find(P(0x1000), 1) != nullptr && reg.find(P(0x1000), 1)->dma == 0x7000);
  EDGE("last_byte", reg.find(P(0x10ff), 1) != nullptr);
  EDGE("byte_at_end", reg.find(P(0x1100), 1) == nullptr);
  EDGE("zero_length_inside", reg.find(P(0x1010), 0) == nullptr);
  EDGE("zero_length_insert_refused", !reg.insert(HostRange{0x3000, 0, 0, false}));
  // adjacent ranges: allowed, and a slice across their seam lies in neither
  EDGE("adjacent_after", reg.insert(HostRange{0x1100, 0x80, 0x9000, true}));
  EDGE("adjacent_before", reg.insert(HostRange{0xf00, 0x100, 0xa000, false}));
  EDGE("across_seam", reg.find(P(0x10f8), 0x10) == nullptr && reg.find(P(0xff8), 0x10) == nullptr);
  EDGE("seam_sides", reg.find(P(0x10f8), 8)->base == 0x1000 && reg.find(P(0x1100), 8)->base == 0x1100 &&
                         reg.find(P(0xff8), 8)->base == 0xf00);
  // overlaps refused: inside, covering, across the start, across the end, the same range again
  EDGE("overlap_inside", !reg.insert(HostRange{0x1010, 0x10, 0, false}));
  EDGE("overlap_covering", !reg.insert(HostRange{0xe00, 0x1000, 0, false}));
  EDGE("overlap_start", !reg.insert(HostRange{0xeff, 2, 0, false}));
  EDGE("overlap_end", !reg.insert(HostRange{0x117f, 2, 0, false}));
  EDGE("overlap_same", !reg.insert(a));
  EDGE("wraps_refused", !reg.insert(HostRange{~(uintptr_t)0 - 4, 16, 0, false}));
  EDGE("find_wraps", reg.find(P(~(uintptr_t)0 - 4), 16) == nullptr);
  // remove: only by the start of a range
  EDGE("remove_interior", !reg.remove(P(0x1001)));
  EDGE("remove_unknown", !reg.remove(P(0x5000)));
  HostRange out;
  EDGE("remove_start", reg.remove(P(0x1000), &out) && out.len == 0x100 && out.dma == 0x7000);
  EDGE("remove_twice", !reg.remove(P(0x1000)));
  EDGE("gone", reg.find(P(0x1000), 1) == nullptr && reg.find(P(0x1100), 1) != nullptr && reg.size() == 2);
  EDGE("reinsert", reg.insert(a) && reg.size() == 3);
  return bad;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::strcmp(argv[1], "edges") == 0) return run_edges();
  if (argc >= 4 && std::strcmp(argv[1], "random") == 0)
    return run_random(std::strtoul(argv[2], nullptr, 0), std::strtoul(argv[3], nullptr, 0));
  std::fprintf(stderr, "usage: hostmem_host random SEED OPS | edges\n");
  return 2;
}
