// at2v_api_cache.h — the sender cache's host protocol: claim slots, compaction, thrash guard (a piece of at2v_api.hip).
//
// Per-sender A cache of one device (at2v_opts.sender_cache; at2v_cache.h). Cached launch L claims new keys
// into claim slot b = L % kClaimSlots; after the launch the build stream (the context's own stream) builds the slot's
// payloads, flips them valid, frees the slot (slot_free[b]) and copies the counters for the host, so no launch waits for
// a build unless kClaimSlots launches in a row are still waiting for theirs. When a launch finds the free list empty,
// the host learns it from that copy and enqueues a compaction on the build stream (cache_before_launch); no launch waits
// for it.
#pragma once
#include "at2v_api_bcomb.h"
#include "at2v_api_ctx.h"
#include "at2v_cache.h"

namespace {

constexpr int kClaimSlots = 8;
struct PendingBuild {  // a launch's builds, enqueued on the build stream after it
  at2v::CacheArgs args{};
  uint32_t max_claims = 0;
  int slot = 0;
};
struct SenderCache {
  at2v::CacheArgs args{};
  DevBuf tags[2], entries[2];  // the live tag table / entries ([cur]) and the compaction target ([cur ^ 1])
  int cur = 0;
  DevBuf payload, free_slots, used, ctl, seen, claim_list[kClaimSlots];
  DevBuf keys, key_status;  // a key list of at2v_sender_preload / _unpin / _query and its status bytes
  const int4* bcomb = nullptr;      // the combs of B, shared by the process's comb contexts on this device (bcomb_acquire)
  const int4* bcomb_lat = nullptr;
  // Builds run on the context's own stream (the shard's), which a caller's launches on its own streams never use: a
  // separate build stream would share one of the process's 4 hardware queues (GPU_MAX_HW_QUEUES, round robin) with a
  // caller's stream, whose next copy or launch then waited behind a 0.8 ms comb build (config 5 p99).
  hipStream_t build = nullptr;
  hipEvent_t claims_ready[kClaimSlots] = {};  // launch stream, after the launch that filled slot b
  hipEvent_t slot_free[kClaimSlots] = {};     // build stream, after slot b's flip
  hipEvent_t built = nullptr;                 // build stream, after the last flip
  // recorded after the last compaction (build stream). Until it has completed, launches read the old table and claim
  // nothing; the first launch after it swaps the tables. So no launch probes a tag table that is still being filled or
  // pops the free list while it is being rebuilt, whatever stream it runs on (in round 4 a launch on the other
  // scratch set's stream could overlap a compaction enqueued on its neighbour's stream).
  hipEvent_t compacted = nullptr;
  unsigned long long* host_ctl = nullptr;  // pinned copy of the device counters, refreshed after every cached launch
  hipEvent_t ctl_copied = nullptr;
  bool copy_pending = false;
  bool compact_pending = false;  // a launch found the cache full: compact before a later launch
  bool compacting = false;       // a compaction is enqueued on the build stream and has not been swapped in yet
  uint64_t launches = 0;  // launch epochs (entries record the last launch that used them)
  // Thrash guard (round 6, VERDICT r5 "Next" 2): a compaction that had to evict entries used by the latest launch
  // (its age threshold is 0: the working set is larger than the cache and every cached key is still in use) would only
  // trade comb builds for other keys of the same worth. The cache then stops claiming for freeze_len launches (8,
  // doubling up to 256 while compactions keep cutting at age 0; a compaction that cuts older entries resets it), so the
  // keys it holds keep serving and no build is spent on churn.
  uint64_t compactions_seen = 0;
  uint32_t freeze_len = 0, freeze_left = 0;
};

void free_cache(SenderCache*& c) {
  if (!c) return;
  if (c->build) (void)hipStreamSynchronize(c->build);  // (the shard's stream: destroyed with the shard)
  for (DevBuf* b : {&c->tags[0], &c->tags[1], &c->entries[0], &c->entries[1], &c->payload, &c->free_slots, &c->used,
                    &c->ctl, &c->seen, &c->keys, &c->key_status})
    b->release();
  bcomb_release(c->bcomb);
  bcomb_release(c->bcomb_lat);
  for (DevBuf& b : c->claim_list) b.release();
  if (c->host_ctl) (void)hipHostFree(c->host_ctl);
  for (hipEvent_t ev : {c->built, c->compacted, c->ctl_copied})
    if (ev) (void)hipEventDestroy(ev);
  for (int j = 0; j < kClaimSlots; ++j) {
    if (c->claims_ready[j]) (void)hipEventDestroy(c->claims_ready[j]);
    if (c->slot_free[j]) (void)hipEventDestroy(c->slot_free[j]);
  }
  delete c;
  c = nullptr;
}

// Per-sender cache for `capacity` distinct keys on the current device: 2x as many tag slots (open addressing at
// load <= 1/2), one payload per key. AT2V_TEST_CACHE_FP_BITS (tests only) keeps that many fingerprint bits, so distinct
// keys collide and the byte comparison in the verify kernels is exercised.
int init_cache(Shard& s, uint32_t capacity, uint64_t seed, bool comb, bool admit_first, bool bcomb_wide) {
  SenderCache* c = new (std::nothrow) SenderCache;
  if (!c) return AT2V_E_OOM;
  s.cache = c;
  if (capacity > (1u << 24)) capacity = 1u << 24;
  uint32_t cap = 1024;
  while (cap < 2ull * capacity) cap <<= 1;
  at2v::CacheArgs& a = c->args;
  a.cap = cap;
  a.capacity = capacity;
  a.seed = seed;
  a.fp_mask = ~0ull;
  a.comb = comb ? 1 : 0;
  a.admit_first = admit_first ? 1 : 0;
  // the sighting filter: 2^21 fingerprints (16 MB), so a key seen twice within ~a million records is still found
  a.seen_mask = (1u << 21) - 1;
  if (const char* b = at2v::test_env("AT2V_TEST_CACHE_FP_BITS")) {
    const int bits = std::atoi(b);
    if (bits > 0 && bits < 64) a.fp_mask = (1ull << bits) - 1ull;
  }
  const size_t ctl_bytes = (size_t)at2v::cache_ctl_words() * 8;
  for (int t = 0; t < 2; ++t) {
    AT2V_TRY(c->tags[t].ensure((size_t)cap * 8));
    AT2V_TRY(c->entries[t].ensure((size_t)cap * at2v::cache_entry_bytes()));
    // (on the shard's stream, as every other operation of a context: a process that never touches the null stream maps
    // one hardware queue less)
    AT2V_TRY(hipMemsetAsync(c->tags[t].p, 0, c->tags[t].cap, s.stream));
    AT2V_TRY(hipMemsetAsync(c->entries[t].p, 0, c->entries[t].cap, s.stream));  // every entry invalid
  }
  AT2V_TRY(c->payload.ensure((size_t)capacity * at2v::cache_payload_bytes(a.comb)));
  AT2V_TRY(c->free_slots.ensure((size_t)capacity * 4));
  AT2V_TRY(c->used.ensure((size_t)capacity * 4));
  AT2V_TRY(c->ctl.ensure(ctl_bytes));
  AT2V_TRY(hipMemsetAsync(c->ctl.p, 0, c->ctl.cap, s.stream));
  AT2V_TRY(c->seen.ensure(((size_t)a.seen_mask + 1) * 8));
  AT2V_TRY(hipMemsetAsync(c->seen.p, 0, c->seen.cap, s.stream));
  for (int j = 0; j < kClaimSlots; ++j) AT2V_TRY(c->claim_list[j].ensure((size_t)capacity * 16));
  a.tags = (unsigned long long*)c->tags[0].p;
  a.entries = (int4*)c->entries[0].p;
  a.payload = (int4*)c->payload.p;
  a.free_slots = (uint32_t*)c->free_slots.p;
  a.ctl = (unsigned long long*)c->ctl.p;
  a.seen = (unsigned long long*)c->seen.p;
  a.new_list = (uint4*)c->claim_list[0].p;
  if (comb) {  // the combs of B, built once: 16-bit windows (low-latency kernel and every other comb path) and 20-bit
               // ones for the hit-list kernel, 24-bit with AT2V_CTX_BCOMB_WIDE
    const int lat_bits = at2v::bcomb_lat_bits();
    const int bits = bcomb_wide ? at2v::bcomb_wide_bits() : at2v::bcomb_mid_bits();
    AT2V_TRY(bcomb_acquire(s.device, lat_bits, s.stream, &c->bcomb_lat));
    AT2V_TRY(bcomb_acquire(s.device, bits, s.stream, &c->bcomb));
    a.bcomb_lat = c->bcomb_lat;
    a.bcomb = c->bcomb;
    a.bcomb_bits = bits;
  }
  AT2V_TRY(at2v::launch_cache_init(a, s.stream));
  AT2V_TRY(hipStreamSynchronize(s.stream));
  AT2V_TRY(hipHostMalloc((void**)&c->host_ctl, c->ctl.cap, hipHostMallocDefault));
  std::memset(c->host_ctl, 0, c->ctl.cap);
  c->build = s.stream;
  AT2V_TRY(hipEventCreateWithFlags(&c->ctl_copied, hipEventDisableTiming));
  for (int j = 0; j < kClaimSlots; ++j) {  // recorded once, so the first waits are no-ops
    AT2V_TRY(hipEventCreateWithFlags(&c->claims_ready[j], hipEventDisableTiming));
    AT2V_TRY(hipEventCreateWithFlags(&c->slot_free[j], hipEventDisableTiming));
    AT2V_TRY(hipEventRecord(c->claims_ready[j], s.stream));
    AT2V_TRY(hipEventRecord(c->slot_free[j], c->build));
  }
  AT2V_TRY(hipEventCreateWithFlags(&c->built, hipEventDisableTiming));
  AT2V_TRY(hipEventRecord(c->built, c->build));
  AT2V_TRY(hipEventCreateWithFlags(&c->compacted, hipEventDisableTiming));
  AT2V_TRY(hipEventRecord(c->compacted, c->build));
  return AT2V_OK;
}

// the counters' copy has landed (ctl_copied complete): what it says about compactions (thrash guard) and a full cache
void cache_note_ctl_copy(SenderCache& c) {
  c.copy_pending = false;
  if (c.host_ctl[at2v::kCtlCompactions] > c.compactions_seen) {  // a compaction has run since the last look
    c.compactions_seen = c.host_ctl[at2v::kCtlCompactions];
    if (c.host_ctl[at2v::kCtlThreshold] == 0) {
      c.freeze_len = c.freeze_len ? std::min<uint32_t>(2 * c.freeze_len, 256) : 8;
      c.freeze_left = c.freeze_len;
    } else {
      c.freeze_len = 0;
    }
  }
  if (c.host_ctl[at2v::kCtlFull] && !c.freeze_left) c.compact_pending = true;
}

// stream `st` (the build stream) waits for every launch so far: the last one on each scratch set
hipError_t wait_all_launches(Shard& s, hipStream_t st) {
  hipError_t r = hipSuccess;
  for (int k = 0; k < s.sets && r == hipSuccess; ++k) r = hipStreamWaitEvent(st, s.scratch_free[k], 0);
  return r;
}

// the cache's arguments pointed at the spare tables ([cur ^ 1]): what a compaction fills and the next swap makes live
at2v::CacheArgs spare_tables(const SenderCache& c) {
  at2v::CacheArgs a = c.args;
  a.tags = (unsigned long long*)c.tags[c.cur ^ 1].p;
  a.entries = (int4*)c.entries[c.cur ^ 1].p;
  return a;
}

// a completed compaction's tables become the live ones
void cache_swap_tables(SenderCache& c) {
  const at2v::CacheArgs sp = spare_tables(c);
  c.cur ^= 1;
  c.args.tags = sp.tags;
  c.args.entries = sp.entries;
  c.compacting = false;
}

// a compaction into the spare tables on the build stream; `room`: payloads a preload needs free afterwards, else 0
hipError_t enqueue_compaction(SenderCache& c, uint32_t room) {
  const at2v::CacheArgs sp = spare_tables(c);
  at2v::CacheCompactArgs x{sp.tags, sp.entries, (uint32_t*)c.used.p, room};
  hipError_t e = at2v::launch_cache_compact(c.args, x, c.build);
  if (e == hipSuccess) e = hipEventRecord(c.compacted, c.build);
  return e;
}

// Before a cached launch on `stream`: wait until the launch's claim slot is free; if an earlier launch found the cache
// full (its counters' copy has landed), enqueue a compaction on the build stream, behind every launch and build issued
// so far. Launches issued while it runs look keys up in the old table and claim nothing (CacheArgs::no_claim), so they
// neither wait for it nor touch what it rebuilds (the free list, the spare table). The first launch after it has
// completed swaps the tables in; from then on the build stream also waits for every launch issued before the swap, so a
// payload an evicted entry still held (maybe read by a lookup-only launch) is rebuilt for another key only once those
// launches are done.
hipError_t cache_before_launch(SenderCache& c, Shard& s, hipStream_t stream, int j) {
  hipError_t e = hipStreamWaitEvent(stream, c.slot_free[j], 0);
  if (e == hipSuccess && c.copy_pending && hipEventQuery(c.ctl_copied) == hipSuccess) cache_note_ctl_copy(c);
  if (e == hipSuccess && c.compacting && hipEventQuery(c.compacted) == hipSuccess) {
    e = wait_all_launches(s, c.build);
    if (e == hipSuccess) cache_swap_tables(c);
  }
  if (e == hipSuccess && c.compact_pending && !c.compacting) {
    e = wait_all_launches(s, c.build);  // (the builds before it are on the build stream already)
    if (e == hipSuccess) e = enqueue_compaction(c, 0);
    if (e == hipSuccess) {
      c.compacting = true;
      c.compact_pending = false;
    }
  }
  c.args.no_claim = c.compacting || c.freeze_left ? 1 : 0;
  if (c.freeze_left) --c.freeze_left;
  return e;
}

// The builds of a cached launch's claim slot (build stream: after the launch, payloads, flip, slot free), then the
// counters' copy for the host (the compaction check of a later launch reads kCtlFull from it): on the context's stream,
// so the caller's stream carries only the verify kernel.
hipError_t enqueue_cache_build(SenderCache& c, const PendingBuild& b) {
  hipError_t e = hipStreamWaitEvent(c.build, c.claims_ready[b.slot], 0);
  if (e == hipSuccess) e = at2v::launch_cache_build(b.args, b.max_claims, c.build);
  if (e == hipSuccess) e = hipEventRecord(c.slot_free[b.slot], c.build);
  if (e == hipSuccess) e = hipEventRecord(c.built, c.build);
  // A new copy only once the host has seen the previous one: re-recording the event behind every launch's builds would
  // keep it "not ready" for as long as launches arrive faster than the build stream drains, and the host would never
  // learn that the cache is full (compaction starved; the counters it reads may be a few launches old instead).
  if (e == hipSuccess && !c.copy_pending) {
    e = hipMemcpyAsync(c.host_ctl, c.ctl.p, c.ctl.cap, hipMemcpyDeviceToHost, c.build);
    if (e == hipSuccess) e = hipEventRecord(c.ctl_copied, c.build);
    c.copy_pending = e == hipSuccess;
  }
  return e;
}

// the control words, copied behind everything on the build stream; without `wait` the caller's next wait there covers it
using CtlWords = std::vector<unsigned long long>;
hipError_t read_ctl(SenderCache& c, CtlWords& w, bool wait) {
  w.assign((size_t)at2v::cache_ctl_words(), 0);
  hipError_t e = hipMemcpyAsync(w.data(), c.ctl.p, w.size() * 8, hipMemcpyDeviceToHost, c.build);
  if (e == hipSuccess && wait) e = hipStreamSynchronize(c.build);
  return e;
}

// payloads still free according to control words w: the free list after the last compaction less those handed out since
uint64_t payloads_free(const CtlWords& w, uint64_t capacity) {
  const uint64_t fc = std::min<uint64_t>(w[at2v::kCtlFreeCount], capacity);
  return fc - std::min<uint64_t>(w[at2v::kCtlFreeHead], fc);
}

}  // namespace
