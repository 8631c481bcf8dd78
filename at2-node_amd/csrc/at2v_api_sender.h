// at2v_api_sender.h — known senders: at2v_sender_preload / _unpin / _query (a piece of at2v_api.hip), on
// the sender cache of at2v_api_cache.h through its build stream.
// A CPU context, and a GPU context without a sender cache, only decode: every hip* call below is behind a shard's cache.
#pragma once
#include <map>

#include "at2v_api_hostcall.h"

namespace {

using SenderKey = std::array<uint8_t, 32>;

// the call's distinct keys in first-appearance order, and each listed key's index among them
void distinct_keys(const uint8_t* pk, size_t n, std::vector<SenderKey>& keys, std::vector<uint32_t>& index) {
  std::map<SenderKey, uint32_t> seen;
  index.assign(n, 0);
  keys.clear();
  for (size_t i = 0; i < n; ++i) {
    SenderKey k;
    std::memcpy(k.data(), pk + 32 * i, 32);
    const auto at = seen.emplace(k, (uint32_t)keys.size());
    if (at.second) keys.push_back(k);
    index[i] = at.first->second;
  }
}

// the shard's cache with no compaction under way: the build stream is behind every launch issued so far, and a
// compaction that was enqueued has completed and its tables are the live ones (what cache_before_launch does once the
// compaction's event has fired, here with a host wait: the calls that need it are synchronous)
hipError_t cache_settle(SenderCache& c, Shard& s) {
  hipError_t e = wait_all_launches(s, c.build);
  if (e == hipSuccess && c.compacting) {
    e = hipEventSynchronize(c.compacted);
    if (e == hipSuccess) cache_swap_tables(c);
  }
  return e;
}

// the key list on the device (build stream), its status bytes behind it
hipError_t upload_keys(SenderCache& c, const std::vector<SenderKey>& keys, at2v::CacheKeyList& l) {
  hipError_t e = c.keys.ensure(keys.size() * 32);
  if (e == hipSuccess) e = c.key_status.ensure(keys.size());
  if (e == hipSuccess) e = hipMemcpyAsync(c.keys.p, keys.data(), keys.size() * 32, hipMemcpyHostToDevice, c.build);
  l = at2v::CacheKeyList{(const uint8_t*)c.keys.p, (uint32_t)keys.size(), (uint8_t*)c.key_status.p};
  return e;
}

// the list's status bytes as table `a` has them (build stream, then a host wait)
hipError_t query_keys(SenderCache& c, const at2v::CacheArgs& a, const at2v::CacheKeyList& l, std::vector<uint8_t>& st) {
  st.assign(l.n, 0);
  hipError_t e = at2v::launch_cache_query(a, l, c.build);
  if (e == hipSuccess) e = hipMemcpyAsync(st.data(), l.status, l.n, hipMemcpyDeviceToHost, c.build);
  if (e == hipSuccess) e = hipStreamSynchronize(c.build);
  return e;
}

// One shard's preload (current device = s.device): a launch-shaped step on the build stream. The keys go up; entries the
// list already has are given the call's epoch, so a compaction that makes room keeps them; if the free list cannot hold
// the new keys (or a compaction is due anyway) one compaction runs, with the room request, and is swapped in; then the
// preload kernel claims into the call's claim slot, the usual builds and flip follow, and the statuses are read back.
hipError_t preload_shard(SenderCache& c, Shard& s, const std::vector<SenderKey>& keys, bool pin,
                         std::vector<uint8_t>& st) {
  hipError_t e = cache_settle(c, s);
  at2v::CacheKeyList l{};
  if (e == hipSuccess) e = upload_keys(c, keys, l);
  const int cs = (int)(c.launches % kClaimSlots);
  if (e == hipSuccess) e = hipStreamWaitEvent(c.build, c.slot_free[cs], 0);
  c.args.epoch = (uint32_t)++c.launches;  // entries the call creates or finds count as used by the latest launch
  if (e == hipSuccess) e = at2v::launch_cache_pin(c.args, l, at2v::kPinTouch, c.build);
  CtlWords w;
  if (e == hipSuccess) e = read_ctl(c, w, /*wait=*/false);
  if (e == hipSuccess) e = query_keys(c, c.args, l, st);  // (waits: every launch and build so far is done)
  if (e != hipSuccess) return e;
  if (c.copy_pending) cache_note_ctl_copy(c);  // (its copy is behind us on the build stream)
  size_t fresh = 0;
  for (uint8_t b : st) fresh += (b & AT2V_SENDER_CACHED) ? 0 : 1;
  if (fresh > payloads_free(w, c.args.capacity) || c.compact_pending) {
    e = enqueue_compaction(c, (uint32_t)fresh);
    if (e == hipSuccess) e = hipStreamSynchronize(c.build);
    if (e != hipSuccess) return e;
    cache_swap_tables(c);
    c.compact_pending = false;
    // the thrash guard judges compactions that traffic caused: this one was asked for (its cut may well be at age 0)
    c.compactions_seen = w[at2v::kCtlCompactions] + 1;
  }
  at2v::CacheArgs ca = c.args;
  ca.count_word = at2v::kCtlClaims0 + cs;
  ca.new_list = (uint4*)c.claim_list[cs].p;
  ca.admit_first = 1;  // an explicit request is not a sighting
  ca.no_claim = 0;     // ... and no compaction is running: the freeze of the thrash guard does not apply either
  e = at2v::launch_cache_preload(ca, l, pin ? at2v::kPinSet : at2v::kPinTouch, c.build);
  if (e == hipSuccess) e = hipEventRecord(c.claims_ready[cs], c.build);
  if (e == hipSuccess)
    e = enqueue_cache_build(c, PendingBuild{ca, std::min<uint32_t>((uint32_t)keys.size(), ca.capacity), cs});
  if (e == hipSuccess) e = hipEventSynchronize(c.built);
  if (e == hipSuccess) e = query_keys(c, c.args, l, st);
  return e;
}

bool has_sender_cache(const at2v_ctx* ctx) { return !ctx->shards.empty() && ctx->shards[0].cache; }

// What the three calls share. The keys' decode status (`bad`, with `decode`) is all a context without a sender cache
// has to say. Otherwise: the distinct keys; `host`, the call's own step before any device work (anything but AT2V_OK
// ends the call); `step` on every shard in turn; and per distinct key the AND of the status bytes the steps read
// (`all`), cleared unless the key is cached on every device. `status`, if given: per listed key, bad | all.
struct SenderCall {
  std::vector<uint8_t> bad, all;
  std::vector<SenderKey> keys;
  std::vector<uint32_t> index;
};
template <class Host, class Step>
int sender_call(at2v_ctx* ctx, const uint8_t* pk, size_t n, bool decode, uint8_t* status, SenderCall& sc, Host&& host,
                Step&& step) {
  if (!ctx || (n && !pk) || n >= (1u << 31)) return AT2V_E_INVALID;
  if (n == 0) return AT2V_OK;
  try {
    sc.bad.assign(n, 0);
    if (decode) at2v::cpu_sender_status(ctx->cpu, pk, n, sc.bad.data());
    if (!has_sender_cache(ctx)) {
      if (status) std::memcpy(status, sc.bad.data(), n);
      return AT2V_OK;
    }
    distinct_keys(pk, n, sc.keys, sc.index);
    const int rc = host();
    if (rc != AT2V_OK) return rc;
    sc.all.assign(sc.keys.size(), AT2V_SENDER_CACHED | AT2V_SENDER_PINNED);
    std::vector<uint8_t> st;
    hipError_t e = hipSuccess;
    {
      const DeviceScope keep;
      for (Shard& s : ctx->shards) {
        e = hipSetDevice(s.device);
        if (e == hipSuccess) e = step(*s.cache, s, st);
        if (e != hipSuccess) break;
        for (size_t k = 0; k < st.size(); ++k) sc.all[k] &= st[k];
      }
    }
    if (e != hipSuccess) return hip_code(e);
    for (uint8_t& b : sc.all)
      if (!(b & AT2V_SENDER_CACHED)) b = 0;  // not cached on every device: not cached, and no pin to count
    if (status)
      for (size_t i = 0; i < n; ++i) status[i] = (uint8_t)(sc.bad[i] | sc.all[sc.index[i]]);
    return AT2V_OK;
  } catch (const std::bad_alloc&) {
    return AT2V_E_OOM;
  }
}

}  // namespace

int at2v_sender_preload(at2v_ctx* ctx, const uint8_t* pk, size_t n, uint32_t flags, uint8_t* status) {
  if (flags & ~AT2V_SENDER_PIN) return AT2V_E_INVALID;
  const bool pin = (flags & AT2V_SENDER_PIN) != 0;
  SenderCall sc;
  const int rc = sender_call(
      ctx, pk, n, /*decode=*/true, status, sc,
      [&] {
        const size_t limit = ctx->shards[0].cache->args.capacity / 2;
        if (sc.keys.size() > limit) return AT2V_E_INVALID;
        if (pin) {
          size_t add = 0;
          for (const SenderKey& k : sc.keys) add += ctx->pinned.count(k) ? 0 : 1;
          if (ctx->pinned.size() + add > limit) return AT2V_E_INVALID;
        }
        quiesce_host_calls(ctx);
        // (before the device work: the devices' pin marks are never ahead of this set, also when a shard fails below)
        if (pin) ctx->pinned.insert(sc.keys.begin(), sc.keys.end());
        return AT2V_OK;
      },
      [&](SenderCache& c, Shard& s, std::vector<uint8_t>& st) { return preload_shard(c, s, sc.keys, pin, st); });
  if (rc == AT2V_OK && pin)
    for (size_t k = 0; k < sc.all.size(); ++k)
      if (!sc.all[k]) ctx->pinned.erase(sc.keys[k]);
  return rc;
}

int at2v_sender_unpin(at2v_ctx* ctx, const uint8_t* pk, size_t n) {
  SenderCall sc;
  return sender_call(
      ctx, pk, n, /*decode=*/false, nullptr, sc,
      [&] {
        for (const SenderKey& k : sc.keys) ctx->pinned.erase(k);
        return AT2V_OK;
      },
      [&](SenderCache& c, Shard& s, std::vector<uint8_t>&) {
        at2v::CacheKeyList l{};
        hipError_t e = cache_settle(c, s);  // (a compaction under way copies the marks: clear them after it)
        if (e == hipSuccess) e = upload_keys(c, sc.keys, l);
        if (e == hipSuccess) e = at2v::launch_cache_pin(c.args, l, at2v::kPinClear, c.build);
        if (e == hipSuccess) e = hipStreamSynchronize(c.build);  // (the upload's source dies with this frame)
        return e;
      });
}

int at2v_sender_query(at2v_ctx* ctx, const uint8_t* pk, size_t n, uint8_t* status) {
  if (n && !status) return AT2V_E_INVALID;
  SenderCall sc;
  return sender_call(
      ctx, pk, n, /*decode=*/true, status, sc,
      [&] {
        std::memcpy(status, sc.bad.data(), n);  // (what a failing device leaves the caller with)
        return AT2V_OK;
      },
      [&](SenderCache& c, Shard&, std::vector<uint8_t>& st) {
        at2v::CacheKeyList l{};
        hipError_t e = upload_keys(c, sc.keys, l);
        // Reads only, and changes nothing of the cache's state on the host either: a compaction that is enqueued but not
        // swapped in yet is ahead of the query on the build stream, so the query reads the tables it fills (what the next
        // launch will swap in) without swapping them.
        if (e == hipSuccess) e = query_keys(c, c.compacting ? spare_tables(c) : c.args, l, st);
        return e;
      });
}
