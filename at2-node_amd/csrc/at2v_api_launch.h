// at2v_api_launch.h — the one verify launch path of a context (a piece of at2v_api.hip). Every verify launch of a context goes through launch_shard(). A device has kScratchSets scratch sets (per-wave tables,
// chunk-queue counter, pacing lines) used in turn: a launch waits only for the launch that last used its set (an event,
// whatever stream that ran on), so launches on DIFFERENT caller streams overlap: the next batch's blocks take the CUs the
// previous launch's last blocks leave, instead of the device idling through its end-of-launch drain (+3.6% on
// back-to-back config-2 batches, profiles/r03i). The verdict words are zeroed before the kernel, so a chunk that no wave
// wrote fails closed.
#pragma once
#include "at2v_api_cache.h"

namespace {

bool scratch_ok(const Shard& s) {
  for (int j = 0; j < s.sets; ++j)
    if (!s.scratch[j].p) return false;
  return s.btab.p != nullptr;
}

// One verify launch on shard s (current device = s.device), on `stream`, with the shard's next scratch set. Cached
// launches may overlap too: they share the tag table through atomics, each has its own claim slot (and waits for that
// slot's previous builds), and every cached launch after a compaction waits for it (cache_before_launch).
hipError_t launch_shard(at2v_ctx* ctx, Shard& s, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                        uint32_t msg_bytes, const uint32_t* off, uint32_t n, uint32_t* verdicts, hipStream_t stream,
                        bool zero_verdicts = true, bool pipeline = false) {
  // a chunk of the host-buffer pipeline whose batch is above small_batch_max: the throughput kernels at every chunk
  // size, with dense grids (launch_verify)
  const uint32_t pair_max = pipeline ? 0u : ctx->pair_max;
  if (!verdicts || !pk || !scratch_ok(s)) return hipErrorInvalidValue;  // (never launch on a null buffer)
  if (ctx->test_fail_launches) {  // test hook: a launch failure, as a faulting device would report it
    --ctx->test_fail_launches;
    return hipErrorLaunchFailure;
  }
  const int j = (int)(s.next_set++ % (unsigned)s.sets);
  hipError_t e = hipStreamWaitEvent(stream, s.scratch_free[j], 0);
  // the cache serves the throughput kernel (launches above small_batch_max records; with combs, every launch)
  SenderCache* c = (s.cache && (n > pair_max || s.cache->args.comb)) ? s.cache : nullptr;
  // the four-wave comb kernel of small batches writes every verdict word of the launch whatever the verdicts (its
  // blocks stride over all chunks), so the zeroing is left out there: one dependent memset less on the latency path
  if (c && c->args.comb && n <= pair_max) zero_verdicts = false;
  if (e == hipSuccess && zero_verdicts) e = hipMemsetAsync(verdicts, 0, ((size_t)n + 31) / 32 * 4, stream);
  const int cs = c ? (int)(c->launches % kClaimSlots) : 0;
  if (e == hipSuccess && c) e = cache_before_launch(*c, s, stream, cs);
  at2v::CacheArgs ca{};
  if (c) {
    c->args.count_word = at2v::kCtlClaims0 + cs;
    c->args.new_list = (uint4*)c->claim_list[cs].p;
    c->args.epoch = (uint32_t)++c->launches;
    ca = c->args;
  }
  at2v::PartArgs pa{};
  const bool part = c && ctx->partition && n > pair_max;
  if (e == hipSuccess && part) {
    const size_t need = (size_t)n * at2v::part_bytes_per_record();
    if (s.part[j].cap < need) {  // grows: the set's previous launch (it reads the old lists) must be done first
      e = hipEventSynchronize(s.scratch_free[j]);
      if (e == hipSuccess) e = s.part[j].ensure(need);
    }
    uint32_t* base = (uint32_t*)s.part[j].p;
    pa = at2v::PartArgs{base, base + n, base + 2 * (size_t)n, nullptr};
  }
  if (e == hipSuccess)
    e = at2v::launch_verify(pk, sig, msg, msg_bytes, off, n, (int)ctx->policy, verdicts, (int4*)s.scratch[j].p,
                            (const int4*)s.btab.p, s.grid, pair_max, stream, c ? &ca : nullptr,
                            part ? &pa : nullptr, pipeline ? 1 : 0);
  if (e == hipSuccess && c) {
    // claims of this launch -> payloads on the build stream (later launches use them; this one did not wait)
    e = hipEventRecord(c->claims_ready[cs], stream);
    if (e == hipSuccess) e = enqueue_cache_build(*c, PendingBuild{ca, std::min(n, ca.capacity), cs});
  }
  if (e == hipSuccess) e = hipEventRecord(s.scratch_free[j], stream);
  return e;
}

}  // namespace
