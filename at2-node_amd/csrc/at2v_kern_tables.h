// at2v_kern_tables.h — kernel geometry, per-lane and fixed-base table accessors, comb entry readers, LDS staging,
// record loads.
// A piece of the kernels translation unit: at2v_kernels.hip includes the at2v_kern_*.h pieces in order (tables, cache,
// comb, sign, btab) and compiles them with its own kernels and launchers into one object. Each piece uses only the
// shared headers and the pieces before it.
#pragma once
#include <hip/hip_runtime.h>

#include "at2v_comb.h"
#include "at2v_verify.h"
#include "at2v_verify_fu.h"
#include "at2v_fe_fu.h"

namespace at2v {

// What a verify kernel of the cofactorless policies (0..2) hands its body as the policy: the same value, in a form the
// compiler can see is never POLICY_ZIP215, so every cofactored branch of the shared headers folds away in that kernel
// (at2v_kernels.hip; the ZIP215 twins pass the constant).
static_assert(POLICY_ZIP215 == 4 && (POLICY_DALEK_V1 | POLICY_LIBSODIUM_1_0_18 | POLICY_DALEK_V1_LEGACY) < 4,
              "the cofactorless policies fit two bits; ZIP215 does not");
__device__ AT2V_INLINE int cofactorless(int policy) { return policy & 3; }

constexpr int kBlock = 512;  // verify threads per block: 8 waves, both waves of every SIMD in one workgroup
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kVerifyWavesPerSimd = 2;  // register budget: 512 / waves VGPR+AGPR per lane
static_assert(kBlock == 512, "pacing pairs waves w and w^4 of an 8-wave workgroup");
// control words after the lane slots of a launch's `grid` blocks: [0] chunk queue counter; from word 16 on,
// one 64-byte progress line per wave (Pace)
constexpr size_t kCtlBytes(int grid) { return 64 + (size_t)grid * kWavesPerBlock * 64; }
constexpr int kBWin = 16;  // fixed-base window bits: table [0..2^(kBWin-1)]B
// Entry 0 of every per-lane table is the identity, so it is not stored per lane: a digit 0 reads one shared, L2-resident
// identity entry after the B tables instead. Per-lane tables hold [1..8]P (11% less table footprint and write traffic
// than [0..8]P, 1/16 of the entry reads served from L2).
constexpr int kIdentShared = 1;
constexpr int kTabAGranules = (9 - kIdentShared) * 10;  // entries 1..8 x 10 x 16 B (the slot; packed entries use 8)
constexpr int kLaneGranules = 2 * kTabAGranules;  // tables [j]A and [j](+-R)
constexpr int kNumBtabs = 2;                      // [j]B and [j 2^128]B
constexpr size_t kScratchPerWave = (size_t)kLaneGranules * 64 * 16;

// A value the compiler cannot prove wave-uniform but that is (the wave index in the block): as an SGPR, the LDS-DMA
// destinations (M0) need no v_readfirstlane per load.
#define AT2V_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)

// Per-lane table [1..8](-A) in global scratch. Layout: lane-contiguous, so the loads of one entry hit the same cache
// line per lane whatever entry index each lane selects. (r01 interleaved lanes per 16-byte
// granule: lanes with different digits then touched up to 9 different 1 KiB rows per load,
// ~9x read amplification — profiles/r01 FETCH_SIZE.)
// Entries are packed into 128 B, one cache line per entry instead of the cached form's two (the table reads
// of a verify go from ~16.9 to ~8.4 KB). Each coordinate is carried at the table build and its 10 limbs
// (255 bits, limb 1 given a 26th bit for its carry) packed into 8 words: word k holds limb k (k < 8) in its low 26 or
// 25 bits, and limbs 8 and 9 (51 bits) fill the words' free high bits.

// carried element -> 8 words
__device__ AT2V_INLINE void fu_pack8(uint32_t o[8], const fu& f) {
  const uint32_t hl = f.v[8] | (f.v[9] << 26), hh = f.v[9] >> 6;  // H = limb 8 | limb 9 << 26 (51 bits)
  o[0] = f.v[0] | (hl << 26);
  o[1] = f.v[1] | ((hl >> 6) << 26);
  o[2] = f.v[2] | ((hl >> 12) << 26);
  o[3] = f.v[3] | ((hl >> 18) << 25);
  o[4] = f.v[4] | ((hl >> 25) << 26);
  o[5] = f.v[5] | (((hl >> 31) | (hh << 1)) << 25);
  o[6] = f.v[6] | ((hh >> 6) << 26);
  o[7] = f.v[7] | ((hh >> 12) << 25);
}
__device__ AT2V_INLINE void fu_unpack8(fu& f, const uint32_t i[8]) {
  const uint32_t m26 = (1u << 26) - 1, m25 = (1u << 25) - 1;
  f.v[0] = i[0] & m26;
  f.v[1] = i[1] & m26;
  f.v[2] = i[2] & m26;
  f.v[3] = i[3] & m25;
  f.v[4] = i[4] & m26;
  f.v[5] = i[5] & m25;
  f.v[6] = i[6] & m26;
  f.v[7] = i[7] & m25;
  const uint32_t p5 = i[5] >> 25;
  const uint32_t hl = (i[0] >> 26) | ((i[1] >> 26) << 6) | ((i[2] >> 26) << 12) | ((i[3] >> 25) << 18) |
                      ((i[4] >> 26) << 25) | (p5 << 31);
  const uint32_t hh = (p5 >> 1) | ((i[6] >> 26) << 6) | ((i[7] >> 25) << 12);
  f.v[8] = hl & m26;
  f.v[9] = ((hl >> 26) | (hh << 6)) & m25;
}

struct DevTabA {
  int4* base;   // this lane's slot (global): entries kIdentShared..8, packed into 128 B each
  int4* stage;  // this wave's 10 x 1 KiB LDS staging buffer for the prefetched entry
  int lane;
  const int4* ident = nullptr;  // the shared identity entry (kIdentShared)
#ifdef AT2V_WAIT_PROBE
  mutable unsigned long long waited = 0, lds_waited = 0;
#endif
  template <class Cached>
  __device__ AT2V_INLINE void store(int e, const Cached& c) const {
    static_assert(sizeof(Cached) == 160, "cached point: 40 words");
    if (kIdentShared && e == 0) return;  // the identity lives in the shared entry
    const int32_t* w = reinterpret_cast<const int32_t*>(&c);
    uint32_t pw[32];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      fu x;
#pragma unroll
      for (int q = 0; q < 10; ++q) x.v[q] = (uint32_t)w[10 * k + q];
      fu_carry(x);
      fu_pack8(pw + 8 * k, x);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
      base[(e - kIdentShared) * 8 + q] =
          make_int4((int)pw[4 * q], (int)pw[4 * q + 1], (int)pw[4 * q + 2], (int)pw[4 * q + 3]);
  }
  // a decoded point parked in entry 8's space (verify_half_fu, AT2V_PARK_POINTS): 10 stores now, 10 loads and one wait
  // at unpark; entry 8 is the last one the table build writes
  template <class P3>
  __device__ AT2V_INLINE void park(const P3& p) const {
    static_assert(sizeof(P3) == 160, "p3 point: 40 words");
    const int32_t* w = reinterpret_cast<const int32_t*>(&p);
#pragma unroll
    for (int q = 0; q < 10; ++q)
      base[(8 - kIdentShared) * 10 + q] = make_int4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  }
  template <class P3>
  __device__ AT2V_INLINE void unpark(P3& p) const {
    int32_t* w = reinterpret_cast<int32_t*>(&p);
    int4 v[10];
#pragma unroll
    for (int q = 0; q < 10; ++q) v[q] = base[(8 - kIdentShared) * 10 + q];
#pragma unroll
    for (int q = 0; q < 10; ++q) {
      w[4 * q] = v[q].x;
      w[4 * q + 1] = v[q].y;
      w[4 * q + 2] = v[q].z;
      w[4 * q + 3] = v[q].w;
    }
  }
  // LDS-DMA (global_load_lds_dwordx4): entry e of every lane -> stage[q][lane], no VGPRs held while the
  // window's four doublings run
  __device__ AT2V_INLINE void prefetch(int e) const {
    const int4* src = (kIdentShared && e == 0) ? ident : base + (e - kIdentShared) * 8;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src + q),
                                       (__attribute__((address_space(3))) void*)(stage + q * 64), 16,
                                       0, 0);
  }
  template <class Cached>
  __device__ AT2V_INLINE void load_prefetched(Cached& c) const {
    static_assert(sizeof(Cached) == 160, "cached point: 40 words");
    AT2V_PROBE(waited, asm volatile("s_waitcnt vmcnt(0)" ::: "memory"));
    uint32_t pw[32];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int4 v = stage[q * 64 + lane];
      pw[4 * q] = (uint32_t)v.x;
      pw[4 * q + 1] = (uint32_t)v.y;
      pw[4 * q + 2] = (uint32_t)v.z;
      pw[4 * q + 3] = (uint32_t)v.w;
    }
    fu* cf = reinterpret_cast<fu*>(&c);
#pragma unroll
    for (int k = 0; k < 4; ++k) fu_unpack8(cf[k], pw + 8 * k);
  }
};

// The joint table of verify_half_fu_joint: entries 1..11 (packed as DevTabA's, stored by DevTabA::store) in the first
// 88 granules of the lane slot, read through the wave's two LDS stages as a double buffer (window i's entry through
// stage i & 1; the stage index is wave-uniform).
constexpr int kJointGranules = (kJointEntries - kIdentShared) * 8;
static_assert(kJointGranules <= kLaneGranules, "the joint table fits the lane slot");
struct DevTabJ {
  DevTabA t;   // base: the lane slot; stage: stage 0
  int stage1;  // stage 1, in granules from stage 0 (one base pointer: both stay provably LDS addresses)
  __device__ AT2V_INLINE int4* stage_of(int st) const { return t.stage + (st ? stage1 : 0); }
  template <class Cached>
  __device__ AT2V_INLINE void store(int e, const Cached& c) const {
    t.store(e, c);
  }
  // stage_just_read: the stage's previous entry was read with no arithmetic on it since (wait for those LDS reads)
  __device__ AT2V_INLINE void prefetch(int st, int e, bool stage_just_read) const {
    if (stage_just_read) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int4* src = (kIdentShared && e == 0) ? t.ident : t.base + (e - kIdentShared) * 8;
    int4* const stg = stage_of(st);
#pragma unroll
    for (int q = 0; q < 8; ++q)
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src + q),
                                       (__attribute__((address_space(3))) void*)(stg + q * 64), 16, 0, 0);
  }
  template <class Cached>
  __device__ AT2V_INLINE void load_prefetched(int st, Cached& c) const {
    static_assert(sizeof(Cached) == 160, "cached point: 40 words");
    AT2V_PROBE(t.waited, asm volatile("s_waitcnt vmcnt(0)" ::: "memory"));
    int4* const stg = stage_of(st);
    uint32_t pw[32];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int4 v = stg[q * 64 + t.lane];
      pw[4 * q] = (uint32_t)v.x;
      pw[4 * q + 1] = (uint32_t)v.y;
      pw[4 * q + 2] = (uint32_t)v.z;
      pw[4 * q + 3] = (uint32_t)v.w;
    }
    fu* cf = reinterpret_cast<fu*>(&c);
#pragma unroll
    for (int k = 0; k < 4; ++k) fu_unpack8(cf[k], pw + 8 * k);
  }
};

struct LdsTabB {
  const int4* lds;  // AT2V_BTAB_ENTRIES x 8 granules
  __device__ AT2V_INLINE void load(int e, ge_niels& n) const {
    int32_t w[32];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int4 v = lds[e * 8 + q];
      w[4 * q] = v.x;
      w[4 * q + 1] = v.y;
      w[4 * q + 2] = v.z;
      w[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      n.ypx.v[k] = w[k];
      n.ymx.v[k] = w[10 + k];
      n.xy2d.v[k] = w[20 + k];
    }
  }
};

// Fixed-base table [0..2^(kBWin-1)]B (affine Niels, 8 x 16 B per entry: 4.2 MB) in global memory, read through an
// LDS-DMA prefetch like the A entries.
constexpr int kBtabEntries = (1 << (kBWin - 1)) + 1;
struct DevTabB {
  const int4* base;
  int4* stage;  // this wave's 8 x 1 KiB LDS staging buffer
  int lane;
#ifdef AT2V_WAIT_PROBE
  mutable unsigned long long waited = 0, lds_waited = 0;
#endif
  __device__ AT2V_INLINE void prefetch(int e) const {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the stage may be shared with a just-read entry
#pragma unroll
    for (int q = 0; q < 8; ++q)
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(base + e * 8 + q),
                                       (__attribute__((address_space(3))) void*)(stage + q * 64), 16, 0, 0);
  }
  template <class Niels>
  __device__ AT2V_INLINE void load_prefetched(Niels& n) const {
    static_assert(sizeof(Niels) == 120, "Niels point: 30 words");
    AT2V_PROBE(waited, asm volatile("s_waitcnt vmcnt(0)" ::: "memory"));
    int32_t w[32];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int4 v = stage[q * 64 + lane];
      w[4 * q] = v.x;
      w[4 * q + 1] = v.y;
      w[4 * q + 2] = v.z;
      w[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      n.ypx.v[k] = w[k];
      n.ymx.v[k] = w[10 + k];
      n.xy2d.v[k] = w[20 + k];
    }
  }
};

// Per-wait probe of the comb kernel (a variant build: tools/build_variant.sh <tag> -DAT2V_COMB_PROBE, read by
// tools/ab_bench.py --probe through at2v_probe_read): s_memtime cycles per wave in each wait and phase of
// verify_chunks_comb4, summed over the launch. Product builds: just stmt.
#if defined(AT2V_COMB_PROBE) && defined(__HIP_DEVICE_COMPILE__)
#define AT2V_CPROBE(acc, stmt)                                  \
  do {                                                          \
    const unsigned long long t0_ = __builtin_amdgcn_s_memtime(); \
    stmt;                                                       \
    (acc) += __builtin_amdgcn_s_memtime() - t0_;                \
  } while (0)
#else
#define AT2V_CPROBE(acc, stmt) stmt
#endif
#ifdef AT2V_COMB_PROBE
enum {
  kCpAWait,     // A-comb entry: vmcnt wait before the stage is read
  kCpBWait,     // B-comb entry: the same
  kCpStage,     // lgkmcnt wait before a stage is refilled
  kCpRecord,    // the record's R, S, A, offsets loaded + the prechecks
  kCpSha,       // SHA-512(R || A || M) mod l, recodes (message loads included)
  kCpSums,      // the 26 A + 16 B comb additions (the three waits above included)
  kCpFinish,    // slot round trip, shared inversion, four encodes + compares
  kCpBook,      // list loads, verdict ORs, chunk ticket
  kCpChunk,     // chunk total
  kCpChunks,    // chunks (count)
  kCpLds,       // comb entries: lgkmcnt wait after the stage's LDS reads (forced in the probe build)
  kCpSlot,      // parked points: vmcnt wait after the slot loads of the inversion and encodes (forced likewise)
  kCpN
};
__device__ unsigned long long at2v_cprobe_acc[kCpN];
struct CombProbe {
  unsigned long long v[kCpN] = {};
};
#endif

// Comb entries (at2v_comb.h) by LDS-DMA into two alternating per-wave stages: the entry of the next addition lands while
// this one is computed. TabC: C[i][j] of this lane's key (CombEntry, kCombGranules); TabBC: D[i][j] (affine Niels, 8).
struct DevComb {
  const int4* base;  // this lane's key's comb
  int4* stage[2];    // this wave's two 10 KiB stages (wave-uniform)
  int lane;
#ifdef AT2V_COMB_PROBE
  mutable unsigned long long waited = 0, stage_waited = 0, lds_waited = 0;
#endif
  __device__ AT2V_INLINE void prefetch(int st, int i, int j) const {
    AT2V_CPROBE(stage_waited, asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"));  // the stage's previous entry is read
    const int4* src = base + ((size_t)i * kCombEntries + j) * kCombGranules;
#pragma unroll
    for (int q = 0; q < kCombGranules; ++q)
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src + q),
                                       (__attribute__((address_space(3))) void*)(stage[st] + q * 64), 16, 0, 0);
  }
  __device__ AT2V_INLINE void load_prefetched(int st, CombEntry& c) const {
    static_assert(sizeof(CombEntry) <= (size_t)kCombWords * 4, "comb entry words");
    AT2V_CPROBE(waited, asm volatile("s_waitcnt vmcnt(0)" ::: "memory"));
    int32_t w[kCombWords];
#pragma unroll
    for (int q = 0; q < kCombGranules; ++q) {
      const int4 v = stage[st][q * 64 + lane];
      w[4 * q] = v.x;
      w[4 * q + 1] = v.y;
      w[4 * q + 2] = v.z;
      w[4 * q + 3] = v.w;
    }
#ifdef AT2V_COMB_PROBE
    AT2V_CPROBE(lds_waited, asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"));
#endif
    int32_t* cw = reinterpret_cast<int32_t*>(&c);
#pragma unroll
    for (int q = 0; q < (int)(sizeof(CombEntry) / 4); ++q) cw[q] = w[q];
  }
};
template <int W>
struct DevBCombW {
  static constexpr int kBits = W;
  const int4* base;  // the context's comb of B (W-bit windows)
  int4* stage[2];
  int lane;
#ifdef AT2V_COMB_PROBE
  mutable unsigned long long waited = 0, stage_waited = 0, lds_waited = 0;
#endif
  __device__ AT2V_INLINE void prefetch(int st, int i, int j) const {
    AT2V_CPROBE(stage_waited, asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"));
    const int4* src = base + ((size_t)i * BCombGeom<W>::kEntries + j) * 8;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(src + q),
                                       (__attribute__((address_space(3))) void*)(stage[st] + q * 64), 16, 0, 0);
  }
  template <class Niels>
  __device__ AT2V_INLINE void load_prefetched(int st, Niels& n) const {
    static_assert(sizeof(Niels) == 120, "Niels point: 30 words");
    AT2V_CPROBE(waited, asm volatile("s_waitcnt vmcnt(0)" ::: "memory"));
    int32_t w[32];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int4 v = stage[st][q * 64 + lane];
      w[4 * q] = v.x;
      w[4 * q + 1] = v.y;
      w[4 * q + 2] = v.z;
      w[4 * q + 3] = v.w;
    }
#ifdef AT2V_COMB_PROBE
    AT2V_CPROBE(lds_waited, asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"));
#endif
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      n.ypx.v[k] = w[k];
      n.ymx.v[k] = w[10 + k];
      n.xy2d.v[k] = w[20 + k];
    }
  }
};
using DevBCombLat = DevBCombW<kBCombLatBits>;  // every context with combs (all other comb paths)

__device__ AT2V_INLINE void stage_btab(int4* lds) {
  const int4* src = reinterpret_cast<const int4*>(AT2V_BTAB);
  for (int i = threadIdx.x; i < AT2V_BTAB_ENTRIES * 8; i += blockDim.x) lds[i] = src[i];
  __syncthreads();
}

__device__ AT2V_INLINE void load8(uint32_t w[8], const uint8_t* p) {  // 32 bytes, 16-B aligned
  const uint4 a = reinterpret_cast<const uint4*>(p)[0];
  const uint4 b = reinterpret_cast<const uint4*>(p)[1];
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
  w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

// little-endian 32-bit word at byte address a of a buffer of `total` bytes; bytes >= total read as 0
__device__ AT2V_INLINE uint32_t load_u32_guarded(const uint8_t* buf, uint32_t a, uint32_t total) {
  if (a + 4 <= total) return *reinterpret_cast<const uint32_t*>(buf + a);
  uint32_t v = 0;
  for (uint32_t b = 0; b < 4; ++b)
    if (a + b < total) v |= (uint32_t)buf[a + b] << (8 * b);
  return v;
}

// store / load a group-local field element or p2 point in this lane's scratch slot (lane-contiguous)
__device__ AT2V_INLINE void slot_store(int4* dst, const int32_t* w, int nw) {
  for (int q = 0; q < (nw + 3) / 4; ++q)
    dst[q] = make_int4(w[4 * q], 4 * q + 1 < nw ? w[4 * q + 1] : 0, 4 * q + 2 < nw ? w[4 * q + 2] : 0,
                       4 * q + 3 < nw ? w[4 * q + 3] : 0);
}
__device__ AT2V_INLINE void slot_load(int32_t* w, const int4* src, int nw) {
  for (int q = 0; q < (nw + 3) / 4; ++q) {
    const int4 v = src[q];
    w[4 * q] = v.x;
    if (4 * q + 1 < nw) w[4 * q + 1] = v.y;
    if (4 * q + 2 < nw) w[4 * q + 2] = v.z;
    if (4 * q + 3 < nw) w[4 * q + 3] = v.w;
  }
}

__device__ AT2V_INLINE int wave_max_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o);
    v = u > v ? u : v;
  }
  return __builtin_amdgcn_readfirstlane(v);
}

}  // namespace at2v
