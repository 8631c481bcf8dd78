// at2v_kern_cache.h — the per-sender A cache on the device: lookup, classify kernel, build and compaction kernels.
// A piece of the kernels translation unit: at2v_kernels.hip includes the at2v_kern_*.h pieces in order (tables, cache,
// comb, sign, btab) and compiles them with its own kernels and launchers into one object. Each piece uses only the
// shared headers and the pieces before it.
#pragma once
#include <hip/hip_runtime.h>

#include "at2v_cache.h"
#include "at2v_cache_select.h"
#include "at2v_comb.h"
#include "at2v_kern_tables.h"

namespace at2v {

// ---- per-sender A cache (at2v_opts.sender_cache; at2v_cache.h) ----
// An entry (4 granules, one 64-byte line): key = the 32 bytes of A, meta = {dalek decode verdict of A, valid, payload
// index u (-1: none), epoch of the last launch that used it}, mark = {pinned, 0, 0, 0} (written by cache_pin_kernel
// only: no lookup, claim or hit reads or writes the fourth granule). A fingerprint only nominates an entry: a record takes it
// only if it is valid (its payload built and flipped by an earlier launch's build stream) and all 32 key bytes equal the
// record's A, so a collision, a claim without a payload or an entry still being built costs speed, never a verdict.
// Plain loads of an entry may be stale across XCDs inside one launch; every stale state (valid = 0, a zero key) only
// turns a hit into a miss, because an entry's key never changes while its tag table is live and valid only goes 0 -> 1.
constexpr int kCacheEntryGranules = 4;
constexpr int kCtlWords = kCtlWordsTotal;

__device__ AT2V_INLINE uint64_t cache_fingerprint(const uint32_t a[8], uint64_t seed, uint64_t mask) {
  uint64_t h = seed;
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    h ^= (uint64_t)a[i] | ((uint64_t)a[i + 1] << 32);
    h *= 0x9e3779b97f4a7c15ull;
    h ^= h >> 29;
  }
  h *= 0xbf58476d1ce4e5b9ull;
  h ^= h >> 32;
  return (h & mask) | 1ull;  // never 0 (= free)
}

// One record per lane, called by every lane of a wave (ballots): find A's entry by fingerprint (open addressing, 32
// probes) or claim a free tag (64-bit CAS). Lanes of the wave that want the same new key elect one leader (the lowest
// lane), which claims for all of them. A claim takes a payload index from the free list (one atomic per wave) and writes
// the entry's key and meta {0, valid 0, u, epoch}; claims that got a payload are appended to the launch's claim set for
// the build stream. A claim that finds the free list empty (u = -1) or a record whose probe path is full flags the cache
// full (compaction before the next launch). Returns the entry slot or -1.
// statistics of a caller that sums its lookups itself (wave-uniform), instead of one atomic per counter per wave
struct LookupStats {
  uint32_t found = 0, claimed = 0, failed = 0, sighted = 0;
};

__device__ AT2V_INLINE int cache_lookup_wave(const CacheArgs& c, const uint32_t a[8], int lane, bool active = true,
                                             LookupStats* st = nullptr) {
  const uint32_t mask = c.cap - 1;
  int slot = -1, claimed = 0, found = 0, want = 0;
  uint64_t fp = cache_fingerprint(a, c.seed, c.fp_mask);
  uint32_t h = (uint32_t)(fp >> 17) & mask, k = 0;
  for (; k < 32; ++k) {  // phase 1: find the key, or the first free tag on its probe path
    const unsigned long long t =
        __hip_atomic_load(c.tags + ((h + k) & mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == fp) {
      slot = (int)((h + k) & mask);
      found = 1;
      break;
    }
    if (t == 0) {
      want = 1;
      break;
    }
  }
  // a lane past the end of the batch (it recomputes the last record) looks up but neither claims nor counts as a sighting
  if (!active) want = 0;
  // a lane whose key is deferred (no claims while a compaction runs, or a first sighting) is a plain miss, not a failure
  int deferred = 0;
  if (c.no_claim && want) {  // a compaction is running: look up only (the records of a new key are misses)
    want = 0;
    deferred = 1;
  }
  int leader = lane, nsame = 0;
  {
    uint64_t pending = __ballot(want);
    while (pending) {  // one iteration per distinct wanted key in the wave
      const int L = __ffsll((long long)pending) - 1;
      const uint64_t fpL = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(fp >> 32), L) << 32) |
                           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)fp, L);
      const int same = want && fp == fpL;
      const uint64_t sm = __ballot(same);
      if (same) {
        leader = L;
        nsame = __popcll(sm);
      }
      pending &= ~sm;
    }
  }
  const int follower = want && leader != lane;
  // admission: the wave's leader of a new key claims it only at its second sighting (or with 2+ records in this wave)
  int sighted = 0;
  if (want && !follower && !c.admit_first && nsame < 2) {
    unsigned long long* sp = c.seen + ((uint32_t)(fp >> 40) & c.seen_mask);
    if (__hip_atomic_load(sp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != fp) {
      __hip_atomic_store(sp, (unsigned long long)fp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sighted = 1;
    }
  }
  {
    const int ls = __shfl(sighted, leader);  // (every lane takes part in the shuffle)
    if (want && ls) deferred = 1;
  }
  if (want && !follower && !sighted) {  // phase 2: claim along the probe path (a racing claimant may take the tag first)
    for (; k < 32; ++k) {
      const uint32_t j = (h + k) & mask;
      const unsigned long long old = atomicCAS(c.tags + j, 0ull, (unsigned long long)fp);
      if (old == 0) {
        slot = (int)j;
        claimed = 1;
        break;
      }
      if (old == fp) {
        slot = (int)j;
        found = 1;
        break;
      }
    }
  }
  {  // followers take their leader's outcome (a shuffle: every lane of the wave takes part)
    const int ls = __shfl(slot, leader);
    if (follower) {
      slot = ls;
      found = ls >= 0;
    }
  }
  const uint64_t below = (1ull << lane) - 1ull;
  const uint64_t cm = __ballot(claimed);
  unsigned long long pbase = 0;
  if (lane == 0 && cm) pbase = atomicAdd(c.ctl + kCtlFreeHead, (unsigned long long)__popcll(cm));
  pbase = __shfl(pbase, 0);
  int u = -1;
  if (claimed) {
    const unsigned long long q = pbase + (unsigned long long)__popcll(cm & below);
    const unsigned long long fc = __hip_atomic_load(c.ctl + kCtlFreeCount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (q < fc) u = (int)c.free_slots[q];
  }
  const uint64_t pm = __ballot(claimed && u >= 0);
  // (a tail lane past n is no failure either: it must not flag the cache full)
  const uint64_t fm = __ballot(found), xm = __ballot(slot < 0 && !deferred && active), sgm = __ballot(sighted);
  unsigned long long nbase = 0;
  if (st) {
    st->found += (uint32_t)__popcll(fm);
    st->claimed += (uint32_t)__popcll(cm);
    st->failed += (uint32_t)__popcll(xm);
    st->sighted += (uint32_t)__popcll(sgm);
  }
  if (lane == 0) {
    if (pm) nbase = atomicAdd(c.ctl + c.count_word, (unsigned long long)__popcll(pm));
    if (!st) {
      if (cm) atomicAdd(c.ctl + kCtlClaimed, (unsigned long long)__popcll(cm));
      if (fm) atomicAdd(c.ctl + kCtlFound, (unsigned long long)__popcll(fm));
      if (xm) atomicAdd(c.ctl + kCtlFailed, (unsigned long long)__popcll(xm));
      if (sgm) atomicAdd(c.ctl + kCtlSighted, (unsigned long long)__popcll(sgm));
    }
    // (a plain load first: a full cache under churn would otherwise have every wave exchange the same word)
    if ((cm != pm || xm) && __hip_atomic_load(c.ctl + kCtlFull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
      atomicExch(c.ctl + kCtlFull, 1ull);
  }
  nbase = __shfl(nbase, 0);
  if (claimed) {
    int4* e = c.entries + (size_t)slot * kCacheEntryGranules;
    e[0] = make_int4((int)a[0], (int)a[1], (int)a[2], (int)a[3]);
    e[1] = make_int4((int)a[4], (int)a[5], (int)a[6], (int)a[7]);
    e[2] = make_int4(0, 0, u, (int)c.epoch);  // valid once cache_flip_kernel has run (after the payload's build)
    if (u >= 0) c.new_list[nbase + (unsigned long long)__popcll(pm & below)] = make_uint4((uint32_t)slot, (uint32_t)u, 0u, 0u);
  }
  return slot;
}

// The record's entry is usable: valid and the key bytes equal. ok = A's decode verdict, u = payload index. A hit records
// this launch's epoch in the entry (the compaction keeps the most recently used entries).
__device__ AT2V_INLINE bool cache_hit(const CacheArgs& c, int slot, const uint32_t Aw[8], int& ok, int& u) {
  ok = 0;
  u = 0;
  if (slot < 0) return false;
  int4* e = c.entries + (size_t)slot * kCacheEntryGranules;
  const int4 k0 = e[0], k1 = e[1], m = e[2];
  ok = m.x;
  u = m.z;
  const bool hit = m.y == 1 && m.z >= 0 && (uint32_t)k0.x == Aw[0] && (uint32_t)k0.y == Aw[1] &&
                   (uint32_t)k0.z == Aw[2] && (uint32_t)k0.w == Aw[3] && (uint32_t)k1.x == Aw[4] &&
                   (uint32_t)k1.y == Aw[5] && (uint32_t)k1.z == Aw[6] && (uint32_t)k1.w == Aw[7];
  if (hit && (uint32_t)m.w != c.epoch) reinterpret_cast<int*>(e + 2)[3] = (int)c.epoch;
  if (!hit) u = 0;
  return hit;
}

// Verdict bits of a partitioned launch's wave (kPart: records in list order). When the wave's 64 records are 64
// consecutive records starting at a multiple of 64 (a list segment appended by one classify wave whose records all went
// to that list: the common case), lane 0 ORs two whole words; otherwise every valid record ORs its own bit. (64 atomics
// on the same two words from one instruction serialise in L2: +20% on a 1M-record comb launch, profiles/r05e.)
__device__ AT2V_INLINE void verdict_or(uint32_t* __restrict__ verdicts, uint32_t rec, int good, bool act, int lane) {
  const uint32_t r0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec);
  const int contig = __builtin_amdgcn_readfirstlane(__all(act && rec == r0 + (uint32_t)lane) && (r0 & 63u) == 0 ? 1 : 0);
  if (contig) {
    const uint64_t m = __ballot(good);
    if (lane == 0) {
      if ((uint32_t)m)
        __hip_atomic_fetch_or(verdicts + (r0 >> 5), (uint32_t)m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((uint32_t)(m >> 32))
        __hip_atomic_fetch_or(verdicts + (r0 >> 5) + 1, (uint32_t)(m >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  } else if (good && act) {
    __hip_atomic_fetch_or(verdicts + (rec >> 5), 1u << (rec & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The classify kernel of a partitioned cached launch: one record per lane, a wave takes kClassifyGroups consecutive
// 64-record groups (a block of 4 waves, 4 kClassifyGroups groups). Every sender is looked up exactly as the round-4
// kernels did in their chunk prologue (cache_lookup_wave: claims, sightings, epochs); the block then takes room in the
// two lists with one atomic per list and writes its hits (index, payload, decode verdict) and misses in group order,
// and adds its statistics with one atomic per counter. (One wave per group with per-wave atomics took 0.54-0.77 ms per
// 1M records: ~100k atomics on a handful of control words, profiles/r05f. Eight groups per wave and per-wave list
// atomics: the same atomic count as now, but each wave ran eight dependent lookup chains one after the other.)
// Block shape: kClassifyWaves waves x kClassifyGroups groups. Blocks of 16 waves x 4 groups (8x fewer list and
// statistics atomics on the same control words) measured no better on the distinct-key leg (0.977 against 0.982-0.987
// of plain, profiles/r05zi): the atomics are not what the classify kernel waits for.
constexpr int kClassifyGroups = 2;
constexpr int kClassifyWaves = 4;
__global__ __launch_bounds__(64 * kClassifyWaves) void cache_classify_kernel(const uint8_t* __restrict__ pk, uint32_t n,
                                                                              CacheArgs c, PartArgs p) {
  __shared__ uint32_t sstat[kClassifyWaves][8];
  __shared__ uint32_t sbase[2];
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;
  const uint32_t ngroups = (n + 63) / 64;
  const uint32_t g0 = (blockIdx.x * kClassifyWaves + (uint32_t)wib) * kClassifyGroups;
  LookupStats st;
  uint64_t hm[kClassifyGroups], am[kClassifyGroups];
  uint32_t info[kClassifyGroups];
  uint32_t nh = 0, na = 0, chunks = 0, chunk_hits = 0;
#pragma unroll
  for (int g = 0; g < kClassifyGroups; ++g) {
    hm[g] = am[g] = 0;
    info[g] = 0;
    if (g0 + g < ngroups) {  // wave-uniform
      const uint32_t i = (g0 + g) * 64 + lane;
      const bool active = i < n;
      uint32_t Aw[8];
      load8(Aw, pk + (size_t)(active ? i : n - 1) * 32);
      const int slot = cache_lookup_wave(c, Aw, lane, active, &st);
      int a_ok = 0, u = 0;
      const bool hit = cache_hit(c, slot, Aw, a_ok, u) && active;
      am[g] = __ballot(active);
      hm[g] = __ballot(hit);
      info[g] = ((uint32_t)u << 1) | (uint32_t)(a_ok & 1);
      nh += (uint32_t)__popcll(hm[g]);
      na += (uint32_t)__popcll(am[g]);
      ++chunks;
      chunk_hits += hm[g] == am[g] ? 1u : 0u;
    }
  }
  if (lane == 0) {
    sstat[wib][0] = chunks;
    sstat[wib][1] = chunk_hits;
    sstat[wib][2] = nh;
    sstat[wib][3] = st.found;
    sstat[wib][4] = st.claimed;
    sstat[wib][5] = st.failed;
    sstat[wib][6] = st.sighted;
    sstat[wib][7] = na - nh;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // the block's room in the two lists
    uint32_t th = 0, tm = 0;
    for (int w = 0; w < kClassifyWaves; ++w) {
      th += sstat[w][2];
      tm += sstat[w][7];
    }
    sbase[0] = th ? atomicAdd(p.counts, th) : 0u;
    sbase[1] = tm ? atomicAdd(p.counts + 1, tm) : 0u;
  }
  if (threadIdx.x < 7) {
    uint32_t v = 0;
    for (int w = 0; w < kClassifyWaves; ++w) v += sstat[w][threadIdx.x];
    const int k = threadIdx.x;
    const int word = k == 0 ? kCtlChunks : k == 1 ? kCtlChunkHits : k == 2 ? kCtlRecHits : k == 3 ? kCtlFound
                     : k == 4 ? kCtlClaimed : k == 5 ? kCtlFailed : kCtlSighted;
    if (v) atomicAdd(c.ctl + word, (unsigned long long)v);
  }
  __syncthreads();
  uint32_t hb = sbase[0], mb = sbase[1];
  for (int w = 0; w < wib; ++w) {  // (wave-uniform) the earlier waves' shares of the block's room
    hb += sstat[w][2];
    mb += sstat[w][7];
  }
  const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
  for (int g = 0; g < kClassifyGroups; ++g) {
    const uint32_t i = (g0 + g) * 64 + lane;
    const uint64_t mm = am[g] & ~hm[g];
    if ((hm[g] >> lane) & 1ull) {
      const uint32_t q = hb + (uint32_t)__popcll(hm[g] & below);
      p.hidx[q] = i;
      p.hinfo[q] = info[g];
    } else if ((mm >> lane) & 1ull) {
      p.midx[mb + (uint32_t)__popcll(mm & below)] = i;
    }
    hb += (uint32_t)__popcll(hm[g]);
    mb += (uint32_t)__popcll(mm);
  }
}

// ------------------------------------------------------------------ per-sender A cache kernels
// Build stream (after the launch that claimed the keys; at2v_cache.h): payloads of the claim set, then the flip that
// makes them valid. Compaction (launch stream, no cached launch or build in flight): the most recently used entries move
// to a fresh tag table, the other payloads go back to the free list.

__device__ AT2V_INLINE void entry_key(uint32_t a[8], const int4* ent) {
  const int4 k0 = ent[0], k1 = ent[1];
  a[0] = (uint32_t)k0.x; a[1] = (uint32_t)k0.y; a[2] = (uint32_t)k0.z; a[3] = (uint32_t)k0.w;
  a[4] = (uint32_t)k1.x; a[5] = (uint32_t)k1.y; a[6] = (uint32_t)k1.z; a[7] = (uint32_t)k1.w;
}

__device__ AT2V_INLINE unsigned long long claim_count(const CacheArgs& c) {
  return __hip_atomic_load(c.ctl + c.count_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Tables (combs off): one lane per claim of the set: dalek's decode verdict and [j]A (build_a_table, the verify
// kernel's own steps) into payload u; the key comes from the entry the claim wrote.
__global__ __launch_bounds__(256) void cache_build_kernel(CacheArgs c) {
  if (blockIdx.x == 0 && threadIdx.x == 0) c.ctl[kCtlBuildT0] = wall_clock64();  // (a vector store from one lane)
  const unsigned long long cnt = claim_count(c);
  for (uint32_t t = blockIdx.x * 256 + threadIdx.x; t < cnt; t += gridDim.x * 256) {
    const uint4 e = c.new_list[t];
    int4* ent = c.entries + (size_t)e.x * kCacheEntryGranules;
    uint32_t a[8];
    entry_key(a, ent);
    DevTabA tw{c.payload + (size_t)e.y * kTabAGranules, nullptr, 0, nullptr};  // store() only
    const int ok = build_a_table(a, tw);
    reinterpret_cast<int*>(ent + 2)[0] = ok;
  }
}

// One claim of the comb build: thread g of the claim's group (2^kPartsLog2 threads per position) writes its share of the
// comb of -A into payload u (comb_build_lane), g = 0 the decode verdict. The group is block- or wave-uniform.
template <int kPartsLog2>
__device__ AT2V_INLINE void comb_claim(const CacheArgs& c, uint32_t t, int g) {
  const uint4 e = c.new_list[t];
  int4* ent = c.entries + (size_t)e.x * kCacheEntryGranules;
  uint32_t a[8];
  entry_key(a, ent);
  int4* cb = c.payload + (size_t)e.y * (kCombBytes / 16);
  const int pos = g >> kPartsLog2;
  struct Mem {  // this position's entries in payload u (a lane reads back only entries it wrote itself)
    int4* row;
    __device__ AT2V_INLINE void put(int j, const uint32_t* w) const {
      int4* dst = row + (size_t)j * kCombGranules;
#pragma unroll
      for (int q = 0; q < kCombGranules; ++q)
        dst[q] = make_int4((int)w[4 * q], (int)w[4 * q + 1], (int)w[4 * q + 2], (int)w[4 * q + 3]);
    }
    __device__ AT2V_INLINE void get(int j, uint32_t* w) const {
      const int4* src = row + (size_t)j * kCombGranules;
#pragma unroll
      for (int q = 0; q < kCombGranules; ++q) {
        const int4 v = src[q];
        w[4 * q] = (uint32_t)v.x;
        w[4 * q + 1] = (uint32_t)v.y;
        w[4 * q + 2] = (uint32_t)v.z;
        w[4 * q + 3] = (uint32_t)v.w;
      }
    }
  } mem{cb + (size_t)(pos < kCombPos ? pos : 0) * kCombEntries * kCombGranules};
  const int ok = comb_build_lane<kPartsLog2>(a, pos, g & ((1 << kPartsLog2) - 1), mem);
  if (g == 0) reinterpret_cast<int*>(ent + 2)[0] = ok;
}

// Combs of a claim set (persistent grid): up to kCombWideMaxKeys claims, one 256-thread block per claim and 8 threads per
// position (profiles/r03zf); more claims, one wave per claim and 2 lanes per position (fewer redundant position chains
// once the waves outnumber the SIMDs).
__global__ __launch_bounds__(256) void cache_comb_kernel(CacheArgs c) {
  if (blockIdx.x == 0 && threadIdx.x == 0) c.ctl[kCtlBuildT0] = wall_clock64();  // (a vector store from one lane)
  const unsigned long long cnt = claim_count(c);
  if (cnt <= (unsigned long long)kCombWideMaxKeys) {
    for (uint32_t t = blockIdx.x; t < cnt; t += gridDim.x) comb_claim<kCombWideLog2>(c, t, (int)threadIdx.x);
  } else {
    const uint32_t nw = gridDim.x * 4;
    for (uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6); t < cnt; t += nw)
      comb_claim<kCombNarrowLog2>(c, t, (int)(threadIdx.x & 63));
  }
}

// After the build kernel (stream order: its payload stores are complete and written back): valid = 1 for every claim of
// the slot, then the slot's count is reset for the launch that reuses it.
__global__ __launch_bounds__(1024) void cache_flip_kernel(CacheArgs c) {
  const unsigned long long cnt = claim_count(c);
  for (uint32_t t = threadIdx.x; t < cnt; t += 1024) {
    const uint4 e = c.new_list[t];
    __hip_atomic_store(reinterpret_cast<int*>(c.entries + (size_t)e.x * kCacheEntryGranules + 2) + 1, 1,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (cnt) {  // the pass's device time (from the build kernel's first block to here) and its payload count
      c.ctl[kCtlBuildTicks] += wall_clock64() - c.ctl[kCtlBuildT0];
      c.ctl[kCtlBuilt] += cnt;
    }
    __hip_atomic_store(c.ctl + c.count_word, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// a fresh cache: every payload index free
__global__ __launch_bounds__(256) void cache_init_kernel(CacheArgs c) {
  for (uint32_t u = blockIdx.x * 256 + threadIdx.x; u < c.capacity; u += gridDim.x * 256) c.free_slots[u] = u;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    c.ctl[kCtlFreeCount] = c.capacity;
    c.ctl[kCtlFreeHead] = 0;
  }
}

__device__ AT2V_INLINE int entry_age(const CacheArgs& c, int4 m) {
  const uint32_t a = c.epoch - (uint32_t)m.w;
  return a > 63u ? 63 : (int)a;
}

__device__ AT2V_INLINE bool entry_pinned(const int4* ent) { return reinterpret_cast<const int*>(ent + 3)[0] == 1; }

// compaction 1: the entries that hold a payload (valid: every build has been flipped by now): the pinned ones are
// counted, the others go into the age histogram
__global__ __launch_bounds__(256) void cache_hist_kernel(CacheArgs c) {
  for (uint32_t s = blockIdx.x * 256 + threadIdx.x; s < c.cap; s += gridDim.x * 256) {
    if (c.tags[s] == 0) continue;
    const int4* e = c.entries + (size_t)s * kCacheEntryGranules;
    const int4 m = e[2];
    if (m.y != 1 || m.z < 0) continue;
    atomicAdd(c.ctl + (entry_pinned(e) ? kCtlPinned : kCtlHist + entry_age(c, m)), 1ull);
  }
}

// compaction 2 (one thread): keep every pinned entry, every other entry younger than T and `rem` of age T, at most 3/4
// of the capacity (less when a preload asks for room), so a later launch has a quarter of the payloads for new keys
// (cache_select, at2v_cache_select.h)
__global__ void cache_select_kernel(CacheArgs c, CacheCompactArgs x) {
  unsigned long long hist[64];
  for (int a = 0; a < 64; ++a) hist[a] = c.ctl[kCtlHist + a];
  const CacheSelection sel = cache_select(c.ctl[kCtlPinned], hist, c.capacity, x.room);
  c.ctl[kCtlThreshold] = (unsigned long long)sel.threshold;
  c.ctl[kCtlRemainder] = sel.rem;
  c.ctl[kCtlRemTaken] = 0;
  c.ctl[kCtlKept] = 0;
  c.ctl[kCtlFreeCount] = 0;
  c.ctl[kCtlFreeHead] = 0;
  c.ctl[kCtlFull] = 0;
  c.ctl[kCtlCompactions] += 1;
}

// compaction 3: kept entries are re-inserted into the fresh tag table (their payloads stay where they are)
__global__ __launch_bounds__(256) void cache_compact_kernel(CacheArgs c, CacheCompactArgs x) {
  const int T = (int)c.ctl[kCtlThreshold];
  const unsigned long long rem = c.ctl[kCtlRemainder];
  const uint32_t mask = c.cap - 1;
  for (uint32_t s = blockIdx.x * 256 + threadIdx.x; s < c.cap; s += gridDim.x * 256) {
    const unsigned long long fp = c.tags[s];
    if (fp == 0) continue;
    const int4* e = c.entries + (size_t)s * kCacheEntryGranules;
    const int4 m = e[2];
    if (m.y != 1 || m.z < 0) continue;  // a claim that never got a payload: its tag is dropped
    const int age = entry_age(c, m);
    const bool pinned = entry_pinned(e);
    const bool keep = pinned || age < T || (age == T && atomicAdd(c.ctl + kCtlRemTaken, 1ull) < rem);
    if (!keep) {
      atomicAdd(c.ctl + kCtlEvicted, 1ull);
      continue;
    }
    const uint32_t h = (uint32_t)(fp >> 17) & mask;
    for (uint32_t k = 0; k < c.cap; ++k) {  // fingerprints are unique in a table: the first free tag on the path
      const uint32_t j = (h + k) & mask;
      if (atomicCAS(x.new_tags + j, 0ull, fp) == 0ull) {
        int4* d = x.new_entries + (size_t)j * kCacheEntryGranules;
        d[0] = e[0];
        d[1] = e[1];
        d[2] = m;
        d[3] = e[3];  // the pin mark
        x.used[m.z] = 1;
        atomicAdd(c.ctl + kCtlKept, 1ull);
        break;
      }
    }
  }
}

// compaction 4: every payload index no kept entry holds is free again
__global__ __launch_bounds__(256) void cache_freelist_kernel(CacheArgs c, CacheCompactArgs x) {
  for (uint32_t u = blockIdx.x * 256 + threadIdx.x; u < c.capacity; u += gridDim.x * 256)
    if (!x.used[u]) c.free_slots[atomicAdd(c.ctl + kCtlFreeCount, 1ull)] = u;
}

// ------------------------------------------------------------------ known senders (at2v_sender_preload / _unpin / _query)

// The slot of A's entry, or -1: a probe along A's path that claims nothing, then all 32 key bytes compared (a fingerprint
// shared with another key is no entry of A's). Called in a kernel of its own, after whatever wrote the keys.
__device__ AT2V_INLINE int cache_probe(const CacheArgs& c, const uint32_t a[8]) {
  const uint32_t mask = c.cap - 1;
  const uint64_t fp = cache_fingerprint(a, c.seed, c.fp_mask);
  const uint32_t h = (uint32_t)(fp >> 17) & mask;
  for (uint32_t k = 0; k < 32; ++k) {
    const uint32_t j = (h + k) & mask;
    const unsigned long long t = __hip_atomic_load(c.tags + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == 0) return -1;
    if (t != fp) continue;
    uint32_t key[8];
    entry_key(key, c.entries + (size_t)j * kCacheEntryGranules);
    bool same = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) same = same && key[i] == a[i];
    return same ? (int)j : -1;  // (fingerprints are unique in a table)
  }
  return -1;
}

__device__ AT2V_INLINE uint8_t entry_status(const int4* ent) {
  const int4 m = ent[2];
  if (m.y != 1 || m.z < 0) return 0;
  return (uint8_t)(1u | (entry_pinned(ent) ? 2u : 0u));  // AT2V_SENDER_CACHED | AT2V_SENDER_PINNED
}

// Preload 1 (build stream, no launch in flight): one key per lane, looked up exactly as a launch's records are
// (cache_lookup_wave; the context passes admit_first = 1, no_claim = 0, the call's claim slot and epoch), so a new key
// claims a tag and a payload and lands in the claim list for cache_build_kernel / cache_comb_kernel and the flip.
// Duplicates within a wave elect one leader, duplicates across waves meet in the tag CAS.
__global__ __launch_bounds__(256) void cache_preload_kernel(CacheArgs c, CacheKeyList l) {
  const int lane = threadIdx.x & 63;
  for (uint32_t w0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; w0 < l.n; w0 += gridDim.x * 256) {  // wave-uniform
    const uint32_t i = w0 + (uint32_t)lane;
    const bool active = i < l.n;
    uint32_t Aw[8];
    load8(Aw, l.pk + (size_t)(active ? i : l.n - 1) * 32);
    (void)cache_lookup_wave(c, Aw, lane, active);
  }
}

// Preload 2 / unpin (a kernel of its own: every key the claims above wrote is visible): the entry of each listed key
// gets the call's epoch (kPinTouch, kPinSet: the compaction treats it as just used) and its pin mark set or cleared.
__global__ __launch_bounds__(256) void cache_pin_kernel(CacheArgs c, CacheKeyList l, int op) {
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < l.n; i += gridDim.x * 256) {
    uint32_t Aw[8];
    load8(Aw, l.pk + (size_t)i * 32);
    const int slot = cache_probe(c, Aw);
    if (slot < 0) continue;
    int4* e = c.entries + (size_t)slot * kCacheEntryGranules;
    if (op != kPinClear) reinterpret_cast<int*>(e + 2)[3] = (int)c.epoch;
    if (op != kPinTouch) reinterpret_cast<int*>(e + 3)[0] = op == kPinSet ? 1 : 0;
  }
}

// Query: status bits per listed key; reads only (no claim, no epoch, no counter, no kCtlFull).
__global__ __launch_bounds__(256) void cache_query_kernel(CacheArgs c, CacheKeyList l) {
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < l.n; i += gridDim.x * 256) {
    uint32_t Aw[8];
    load8(Aw, l.pk + (size_t)i * 32);
    const int slot = cache_probe(c, Aw);
    l.status[i] = slot < 0 ? (uint8_t)0 : entry_status(c.entries + (size_t)slot * kCacheEntryGranules);
  }
}

}  // namespace at2v
