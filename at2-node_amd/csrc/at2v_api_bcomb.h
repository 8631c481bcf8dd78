// at2v_api_bcomb.h — the process-wide registry of the combs of B (part of the one translation unit at2v_api.hip).
//
// The combs of B, shared by every comb context of the process on a device (round 6, VERDICT r5 "Next" 3): built by the
// first context that needs one (on its stream, synchronously, under the registry's lock: a few ms since they are built by
// additions), freed with the last. A node's ingest queue and its batch contexts hold one 872 MB + 67 MB pair per device
// instead of one each.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "at2v_launch.h"

namespace {

struct SharedBComb {
  int device, bits;
  int4* p;
  int refs;
};
std::mutex g_bcomb_mu;
std::vector<SharedBComb>& bcomb_registry() {
  static std::vector<SharedBComb> r;
  return r;
}

hipError_t bcomb_acquire(int device, int bits, hipStream_t st, const int4** out) {
  std::lock_guard<std::mutex> lk(g_bcomb_mu);
  for (SharedBComb& b : bcomb_registry())
    if (b.device == device && b.bits == bits) {
      ++b.refs;
      *out = b.p;
      return hipSuccess;
    }
  int4* p = nullptr;
  void* scratch = nullptr;
  hipError_t e = hipMalloc((void**)&p, at2v::bcomb_bytes(bits));
  if (e == hipSuccess) e = hipMalloc(&scratch, at2v::bcomb_scratch_bytes());
#if AT2V_EXP_BCOMB_NOBUILD  // EXPERIMENT (wrong verdicts on the hit path): the hit-list table allocated but never written
  const bool build = bits == at2v::bcomb_lat_bits();
#else
  const bool build = true;
#endif
  if (e == hipSuccess && build) e = at2v::launch_build_bcomb(p, bits, scratch, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (scratch) (void)hipFree(scratch);
  if (e != hipSuccess) {
    if (p) (void)hipFree(p);
    return e;
  }
  bcomb_registry().push_back({device, bits, p, 1});
  *out = p;
  return hipSuccess;
}

void bcomb_release(const int4* p) {
  if (!p) return;
  std::lock_guard<std::mutex> lk(g_bcomb_mu);
  std::vector<SharedBComb>& r = bcomb_registry();
  for (size_t i = 0; i < r.size(); ++i)
    if (r[i].p == p) {
      if (--r[i].refs == 0) {
        (void)hipFree(r[i].p);
        r.erase(r.begin() + (long)i);
      }
      return;
    }
}

}  // namespace
