// cache_select_host.cpp — the selection arithmetic of a sender-cache compaction (csrc/at2v_cache_select.h: what
// cache_select_kernel runs on the device) as a host program, built with -fsanitize=address,undefined by
// tests/test_cache_select_host.py. The header includes no HIP header, so this is the very function the kernel calls.
//   cache_select_host legacy SEED ROUNDS   no pins, no room request: equal to a literal restatement of the loop
//                                          cache_select_kernel ran before pins existed, over random histograms
//   cache_select_host pins SEED ROUNDS     random pins / histograms / room requests: every pinned entry is kept, the
//                                          total kept is at most the target, at least `room` payloads come free
//   cache_select_host edges                the extremes, one "name ok" line each
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "at2v_cache_select.h"

namespace {

using u64 = unsigned long long;

// the select kernel's loop as it stood before pins (kept here word for word as the reference of the legacy case)
void legacy_select(const u64 hist[64], u64 capacity, int& T, u64& rem) {
  const u64 target = capacity * 3 / 4;
  u64 kept = 0;
  rem = 0;
  T = 64;
  for (int a = 0; a < 64; ++a) {
    const u64 h = hist[a];
    if (kept + h > target) {
      T = a;
      rem = target - kept;
      break;
    }
    kept += h;
  }
}

// what the compact kernel keeps under a selection: every pinned entry, every unpinned one younger than T, rem of age T
u64 kept_total(const at2v::CacheSelection& s, u64 pinned, const u64 hist[64]) {
  u64 k = pinned;
  for (int a = 0; a < 64 && a < s.threshold; ++a) k += hist[a];
  if (s.threshold < 64) k += s.rem;
  return k;
}

// a histogram of `total` entries: spread, or heaped into a few buckets
void random_hist(std::mt19937_64& rng, u64 total, u64 hist[64]) {
  std::memset(hist, 0, 64 * sizeof(u64));
  const int shape = (int)(rng() % 4);
  for (u64 i = 0; i < total; ++i) {
    int a;
    if (shape == 0) a = (int)(rng() % 64);
    else if (shape == 1) a = (int)(rng() % 4);
    else if (shape == 2) a = 63 - (int)(rng() % 3);
    else a = (int)((rng() % 8) * (rng() % 8));
    hist[a > 63 ? 63 : a] += 1;
  }
}

#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      std::fprintf(stderr, "%s:%d: requirement failed: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                                        \
    }                                                                                  \
  } while (0)

int run_legacy(uint64_t seed, long rounds) {
  std::mt19937_64 rng(seed);
  long cuts = 0, whole = 0;
  for (long r = 0; r < rounds; ++r) {
    const u64 capacity = r % 7 == 0 ? 1 + rng() % 8 : 16ull << (rng() % 10);
    const u64 total = rng() % (capacity + 1);  // entries that hold a payload: at most the capacity
    u64 hist[64];
    random_hist(rng, total, hist);
    int T;
    u64 rem;
    legacy_select(hist, capacity, T, rem);
    const at2v::CacheSelection s = at2v::cache_select(0, hist, capacity, 0);
    REQUIRE(s.threshold == T && s.rem == rem);
    REQUIRE(s.target == capacity * 3 / 4);
    (T < 64 ? cuts : whole) += 1;
  }
  std::printf("rounds %ld cuts %ld whole %ld\n", rounds, cuts, whole);
  return 0;
}

int run_pins(uint64_t seed, long rounds) {
  std::mt19937_64 rng(seed);
  long cuts = 0, roomy = 0;
  for (long r = 0; r < rounds; ++r) {
    const u64 capacity = 2 * (1 + rng() % 512);
    const u64 pinned = rng() % (capacity / 2 + 1);  // the context's limits: pins and a call's keys, capacity / 2 each
    const u64 room = rng() % 3 == 0 ? 0 : rng() % (capacity / 2 + 1);
    const u64 total = rng() % (capacity - pinned + 1);  // unpinned entries that hold a payload
    u64 hist[64];
    random_hist(rng, total, hist);
    const at2v::CacheSelection s = at2v::cache_select(pinned, hist, capacity, room);
    const u64 want_target = capacity * 3 / 4 < capacity - room ? capacity * 3 / 4 : capacity - room;
    REQUIRE(s.target == want_target);
    REQUIRE(s.threshold >= 0 && s.threshold <= 64);
    if (s.threshold < 64) REQUIRE(s.rem <= hist[s.threshold]);  // (the compact kernel takes at most what the bucket holds)
    const u64 kept = kept_total(s, pinned, hist);
    REQUIRE(kept >= pinned);            // everything pinned is kept (it is never in the histogram: never cut)
    REQUIRE(kept <= s.target);          // ... and the total kept is at most the target
    REQUIRE(capacity - kept >= room);   // at least `room` payloads come free
    // nothing is dropped without need: either everything stays or the target is met exactly
    REQUIRE(kept == pinned + total || kept == s.target);
    cuts += s.threshold < 64;
    roomy += room > 0;
  }
  std::printf("rounds %ld cuts %ld room_requests %ld\n", rounds, cuts, roomy);
  return 0;
}

int run_edges() {
  u64 hist[64];
  {  // all entries in bucket 0: the cut is at age 0 and takes the remainder from that bucket
    std::memset(hist, 0, sizeof hist);
    hist[0] = 64;
    const at2v::CacheSelection s = at2v::cache_select(0, hist, 64, 0);
    REQUIRE(s.threshold == 0 && s.rem == 48 && s.target == 48);
    std::printf("all_in_bucket_0 ok\n");
  }
  {  // ... with a room request of half the capacity
    const at2v::CacheSelection s = at2v::cache_select(0, hist, 64, 32);
    REQUIRE(s.threshold == 0 && s.rem == 32 && s.target == 32);
    std::printf("all_in_bucket_0_room ok\n");
  }
  {  // pins exactly capacity / 2, the rest young: the pins stay, 16 of the others
    std::memset(hist, 0, sizeof hist);
    hist[0] = 32;
    const at2v::CacheSelection s = at2v::cache_select(32, hist, 64, 0);
    REQUIRE(s.threshold == 0 && s.rem == 16 && kept_total(s, 32, hist) == 48);
    std::printf("pins_half ok\n");
  }
  {  // pins exactly capacity / 2 and a room request of capacity / 2: only the pins stay
    const at2v::CacheSelection s = at2v::cache_select(32, hist, 64, 32);
    REQUIRE(s.target == 32 && s.threshold == 0 && s.rem == 0 && kept_total(s, 32, hist) == 32);
    std::printf("pins_half_room_half ok\n");
  }
  {  // an empty cache
    std::memset(hist, 0, sizeof hist);
    const at2v::CacheSelection s = at2v::cache_select(0, hist, 64, 0);
    REQUIRE(s.threshold == 64 && s.rem == 0 && kept_total(s, 0, hist) == 0);
    const at2v::CacheSelection z = at2v::cache_select(0, hist, 64, 32);
    REQUIRE(z.threshold == 64 && z.rem == 0);
    std::printf("empty ok\n");
  }
  {  // old entries only: everything fits, nothing is cut
    std::memset(hist, 0, sizeof hist);
    hist[63] = 48;
    const at2v::CacheSelection s = at2v::cache_select(0, hist, 64, 0);
    REQUIRE(s.threshold == 64 && kept_total(s, 0, hist) == 48);
    hist[63] = 49;
    const at2v::CacheSelection t = at2v::cache_select(0, hist, 64, 0);
    REQUIRE(t.threshold == 63 && t.rem == 48);
    std::printf("oldest_bucket ok\n");
  }
  {  // inputs outside the context's limits never wrap: more pins than the target keeps no unpinned entry, a room
     // request above the capacity keeps nothing but the pins
    std::memset(hist, 0, sizeof hist);
    hist[0] = 4;
    const at2v::CacheSelection s = at2v::cache_select(60, hist, 64, 0);
    REQUIRE(s.threshold == 0 && s.rem == 0);
    const at2v::CacheSelection t = at2v::cache_select(0, hist, 64, 1000);
    REQUIRE(t.target == 0 && t.threshold == 0 && t.rem == 0);
    std::printf("beyond_limits ok\n");
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "legacy")) return run_legacy(std::strtoull(argv[2], nullptr, 0), std::atol(argv[3]));
  if (argc == 4 && !std::strcmp(argv[1], "pins")) return run_pins(std::strtoull(argv[2], nullptr, 0), std::atol(argv[3]));
  if (argc == 2 && !std::strcmp(argv[1], "edges")) return run_edges();
  std::fprintf(stderr, "usage: cache_select_host legacy|pins SEED ROUNDS | edges\n");
  return 2;
}
