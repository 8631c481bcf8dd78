// at2v_cache_select.h — the selection arithmetic of a sender-cache compaction: which entries stay. Plain C++ with no
// HIP header, so cache_select_kernel (at2v_kern_cache.h) and a host test (tests/host/cache_select_host.cpp) run the
// same function.
//
// A compaction keeps every pinned entry (at2v_sender_preload with AT2V_SENDER_PIN) whatever its age, then the youngest
// unpinned entries: every one younger than T and `rem` of age T. The keep target is 3/4 of the capacity, so a later
// launch has a quarter of the payloads for new keys; a preload that needs `room` payloads lowers it to
// min(3/4 capacity, capacity - room). hist[] counts the UNPINNED entries that hold a payload, by age (63 = 63 or older).
// With no pins and no room request the result is what the compaction computed before pins existed.
#pragma once
#include <cstdint>

#ifndef AT2V_SELECT_HD
#if defined(__HIPCC__)
#define AT2V_SELECT_HD __host__ __device__
#else
#define AT2V_SELECT_HD
#endif
#endif

namespace at2v {

struct CacheSelection {
  int threshold;             // T: unpinned entries of age < T stay; 64: all of them
  unsigned long long rem;    // ... and this many of age T
  unsigned long long target; // payloads the compaction may keep, pinned ones included
};

AT2V_SELECT_HD inline CacheSelection cache_select(unsigned long long pinned, const unsigned long long hist[64],
                                                  unsigned long long capacity, unsigned long long room) {
  CacheSelection s;
  s.target = capacity * 3 / 4;
  if (room > capacity) room = capacity;
  if (capacity - room < s.target) s.target = capacity - room;
  // pinned entries are kept first (the context keeps them at or below capacity / 2, and a call's room request too, so
  // they fit the target; if they ever did not, no unpinned entry stays)
  const unsigned long long budget = pinned < s.target ? s.target - pinned : 0;
  unsigned long long kept = 0;
  s.threshold = 64;
  s.rem = 0;
  for (int a = 0; a < 64; ++a) {
    const unsigned long long h = hist[a];
    if (kept + h > budget) {
      s.threshold = a;
      s.rem = budget - kept;
      break;
    }
    kept += h;
  }
  return s;
}

}  // namespace at2v
