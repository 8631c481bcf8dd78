// at2v_kernels.hip — gfx950 kernels: batch verify (the hot path) and the GPU record generator / signer.
//
// Verify kernel layout (the half-size equation V = [c0]A + [c1]R - [t]B = 0 on the unsigned field of §3b):
//   * one lane = one signature; a wave owns a chunk of 64 records, so the verdict bits of a chunk are one
//     __ballot -> two uint32 words written by lane 0 (no atomics, no cross-wave traffic);
//   * persistent grid of 512-thread blocks (both waves of every SIMD in one workgroup, paced against each other); a
//     wave's first chunk is its index, later ones come from a per-launch queue counter; each wave reuses a fixed
//     160 KiB slice of the scratch buffer for its 64 lanes' tables [1..8]A and [1..8](+-R) (cached form packed into
//     128 B per entry, lane-contiguous; entry 0, the identity, is one shared entry after the B tables); verify_kernel,
//     which takes nothing from a sender cache, keeps ONE joint table of A and R there instead (11 entries, 2-bit
//     windows: verify_half_fu_joint, DESIGN.md §4b "Joint table");
//   * the fixed-base tables [0..2^15]B and [0..2^15] 2^128 B (affine Niels, 128 B per entry, 8.4 MB) are
//     built once per context and stay L2/MALL-resident; table entries reach the lanes by LDS-DMA;
//   * records are read straight from the ABI layout (pk n x 32, sig n x 64, msg + offsets) with
//     16-byte loads for A/R/S and 4-byte loads + v_alignbit for unaligned message words.
// The build switches that once selected other forms of these kernels are retired: DESIGN.md "Retired build switches".
#include <hip/hip_runtime.h>

#include "../../include/at2v.h"
#include "at2v_cache.h"
#include "at2v_comb.h"
#include "at2v_verify.h"
#include "at2v_verify_fu.h"
#include "at2v_fe_fu.h"
#include "at2v_launch.h"
// the pieces of this translation unit, in order: none needs a later one
#include "at2v_kern_tables.h"
#include "at2v_kern_cache.h"
#include "at2v_kern_comb.h"
#include "at2v_kern_sign.h"
#include "at2v_kern_btab.h"
#include "at2v_kern_transfer.h"

namespace at2v {

// Pacing of the two waves that share a SIMD (an 8-wave workgroup places waves w and w^4 on one SIMD;
// MI355X guide, "Two waves per SIMD"). VALU issue goes by priority, then age, so without it the older wave
// runs nearly unimpeded and the younger gets leftover slots. Each wave publishes its progress (work units,
// ~1 per ladder window) and raises its priority while it trails its partner. The partner's value is read
// one mark late (the load issued at mark k is consumed at mark k+1), so the loads' latency is hidden; a
// stale value only misjudges one interval. Stores are vector stores from lane 0.
struct Pace {
  uint32_t* mine;
  const uint32_t* mate;
  uint32_t prog;
  uint32_t mate_prog;
#ifdef AT2V_WAIT_PROBE
  unsigned long long probe[4] = {0, 0, 0, 0};  // digit reads, mid-window mark, chunk total, chunk-start loads
#endif
  __device__ AT2V_INLINE void mark(uint32_t units) { step(units); }
  __device__ AT2V_INLINE void window() { step(1); }
  __device__ AT2V_INLINE void mid() {}
  __device__ AT2V_INLINE void step(uint32_t units) {
    prog += units;
    const uint32_t behind = __builtin_amdgcn_readfirstlane((int)(mate_prog - prog) > 0 ? 1u : 0u);
    if (behind) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
    if ((threadIdx.x & 63) == 0) __hip_atomic_store(mine, prog, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    mate_prog = __hip_atomic_load(mate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// Half-size verification: one chunk of 64 records per wave, no final inversion. kCache: the per-sender A
// cache is on; a wave whose 64 records all hit it skips decoding A and building [j]A (slot_of / cache from
// cache_lookup_kernel + cache_build_kernel, launched just before on the same stream).
// The body is a device function under two kernels with their own parameter lists, so the uncached kernel keeps exactly
// round 2's signature and code (an extra-parameter template of it measured ~1% slower: profiles/r03b, r03d).
// Every verify kernel exists twice: under its own name for the cofactorless policies, which hands the
// body cofactorless(policy), a value the compiler can see is not POLICY_ZIP215, so the cofactored branches of the shared
// headers fold away and the kernel keeps the registers, scratch and code it had before that policy existed; and as
// <name>_zip215, which hands it the constant and is launched by ZIP215 contexts only (AT2V_LAUNCH_VERIFY).
// kPart (partitioned cached launches, at2v_cache.h PartArgs): chunks are 64 entries of the classify kernel's lists
// instead of 64 consecutive records: with kCache ([j]A tables) the hit list's chunks (every record cached: A's decode and
// table skipped) and then the miss list's, without it the miss list alone (the comb kernel takes the hits). A record's
// verdict bit is set by an atomic OR (the lists are in no particular order; the launcher zeroed the words).
template <bool kCache, bool kPart = false>
__device__ AT2V_INLINE void verify_chunks(
    int4* astage, int4* rstage, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig,
    const uint8_t* __restrict__ msg, uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy,
    uint32_t* __restrict__ verdicts, int4* __restrict__ scratch, const int4* __restrict__ btab,
    uint32_t* __restrict__ chunk_queue, const CacheArgs* cp, const PartArgs* pp = nullptr) {
  const int lane = threadIdx.x & 63;
  const int wib = AT2V_UNIFORM(threadIdx.x >> 6);  // wave-uniform: the LDS stage addresses live in SGPRs
  const uint32_t wave = blockIdx.x * kWavesPerBlock + wib;
  const uint32_t nwaves = gridDim.x * kWavesPerBlock;
  uint32_t nchunks = (n + 63) / 64;
  const uint32_t nwords = (n + 31) / 32;
  uint32_t nh = 0, nm = 0, hchunks = 0;
  if constexpr (kPart) {  // the list sizes the classify kernel left (same stream: complete)
    nh = kCache ? __builtin_amdgcn_readfirstlane(pp->counts[0]) : 0u;
    nm = __builtin_amdgcn_readfirstlane(pp->counts[1]);
    hchunks = (nh + 63) / 64;
    nchunks = hchunks + (nm + 63) / 64;
  }
  int4* slot = scratch + ((size_t)wave * 64 + lane) * kLaneGranules;
  const int4* ident = btab + (size_t)kNumBtabs * kBtabEntries * 8;  // shared identity entry after the B tables
  DevTabA ta{slot, astage + wib * 640, lane, ident};
  DevTabA tr{slot + kTabAGranules, rstage + wib * 640, lane, ident};
  const DevTabB tb0{btab, astage + wib * 640, lane};                      // [j]B, staged where A's entry was
  const DevTabB tb1{btab + (size_t)kBtabEntries * 8, rstage + wib * 640, lane};  // [j 2^128]B, in R's stage
  auto wmax = [](int v) { return wave_max_i32(v); };
  uint32_t* prog_lines = chunk_queue + 16;
  Pace pace{prog_lines + (size_t)wave * 16, prog_lines + (size_t)(wave ^ 4) * 16, 0u, 0u};
  if (lane == 0) __hip_atomic_store(pace.mine, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // Chunk c = wave first, then chunks nwaves + ticket from the per-launch queue counter (zeroed by the
  // launcher). The two waves of a SIMD do not get equal issue shares (arbitration by priority, then age), so
  // with a static c += nwaves split half the waves finished at 60% of the kernel time and their SIMDs ran the
  // rest on one wave at half throughput (tools/phase_bench wave timeline). Pulling chunks keeps
  // both waves busy until the queue drains. The ticket is a vector atomic from lane 0, broadcast with
  // readfirstlane, so the loop stays wavefront-uniform; every wave leaves after one ticket >= the chunk count.
  // First chunks: waves 0..3 of every block (one per SIMD) come before waves 4..7, so a launch with at most
  // 4 chunks per block runs every chunk on a SIMD of its own (blocks take the whole LDS: one per CU).
  constexpr uint32_t kHalf = kWavesPerBlock / 2;
  const uint32_t c_first = wib < (int)kHalf ? blockIdx.x * kHalf + wib
                                            : gridDim.x * kHalf + blockIdx.x * kHalf + (wib - kHalf);
  for (uint32_t c = c_first; c < nchunks;) {
    AT2V_PHASE(0);
#ifdef AT2V_WAIT_PROBE
    const unsigned long long t_chunk0 = __builtin_amdgcn_s_memtime();
#endif
    uint32_t i, ii;
    bool act;
    int phit = 0;        // kPart: a hit-list chunk (wave-uniform)
    uint32_t pinfo = 0;  // kPart: the hit's (payload << 1) | A's decode verdict
    if constexpr (kPart) {
      phit = c < hchunks ? 1 : 0;
      const uint32_t pos = (phit ? c : c - hchunks) * 64 + lane, cnt = phit ? nh : nm;
      const uint32_t pc = pos < cnt ? pos : cnt - 1;  // tail lanes recompute the list's last record; masked
      act = pos < cnt;
      i = ii = (phit ? pp->hidx : pp->midx)[pc];
      if (phit) pinfo = pp->hinfo[pc];
    } else {
      i = c * 64 + lane;
      ii = i < n ? i : n - 1;  // tail lanes recompute a real record; their bit is masked
      act = i < n;
    }
    uint32_t Rw[8], Sw[8], Aw[8];
    load8(Rw, sig + (size_t)ii * 64);
    load8(Sw, sig + (size_t)ii * 64 + 32);
    load8(Aw, pk + (size_t)ii * 32);
    const uint32_t o0 = off[ii];
    const uint32_t len = off[ii + 1] - o0;
#ifdef AT2V_WAIT_PROBE
    AT2V_PROBE(pace.probe[2], asm volatile("s_waitcnt vmcnt(0)" ::: "memory"));
#endif
    // message words: a wave whose messages all end >= 8 bytes before the buffer end reads two aligned words and
    // funnel-shifts them (no per-lane branch); otherwise every byte is bounds-checked (the last records of a batch)
    const int msg_fast =
        __builtin_amdgcn_readfirstlane(__all((uint64_t)o0 + len + 8 <= (uint64_t)msg_total) ? 1 : 0);
    const uint32_t* mw = reinterpret_cast<const uint32_t*>(msg) + (o0 >> 2);
    const uint32_t msh = (o0 & 3u) * 8;
    auto msg_unguarded = [=](uint32_t j) -> uint32_t { return __builtin_amdgcn_alignbit(mw[j + 1], mw[j], msh); };
    auto msg_guarded = [=](uint32_t j) -> uint32_t {
      const uint32_t a = o0 + 4 * j;
      const uint32_t a0 = a & ~3u, sh = (a & 3u) * 8;
      const uint32_t lo = load_u32_guarded(msg, a0, msg_total);
      if (sh == 0) return lo;
      const uint32_t hi = load_u32_guarded(msg, a0 + 4, msg_total);
      return __builtin_amdgcn_alignbit(hi, lo, sh);
    };
    auto touched = [] {};
    MsgSplit<decltype(msg_unguarded), decltype(msg_guarded), decltype(touched)> msgword{msg_fast, msg_unguarded,
                                                                                        msg_guarded, touched};
    int good;
    if (kCache) {
      const CacheArgs& cc = *cp;
      int a_ok = 0, u = 0, all_hit;
      if constexpr (kPart) {  // classified already
        all_hit = phit;
        a_ok = (int)(pinfo & 1u);
        u = (int)(pinfo >> 1);
      } else {
        // the chunk's senders: looked up (new keys claimed for the build stream) in the chunk prologue
        const int slot = cache_lookup_wave(cc, Aw, lane, i < n);
        const bool hit = cache_hit(cc, slot, Aw, a_ok, u);
        all_hit = __builtin_amdgcn_readfirstlane(__all(hit) ? 1 : 0);
        if (lane == 0) {
          atomicAdd(cc.ctl + kCtlChunks, 1ull);
          if (all_hit) atomicAdd(cc.ctl + kCtlChunkHits, 1ull);
        }
      }
      DevTabA tc{ta};
      if (all_hit) tc.base = cc.payload + (size_t)u * kTabAGranules;
      good = verify_half_fu<true>(Rw, Aw, Sw, len, msgword, policy, tc, tr, tb0, tb1, wmax, pace, all_hit, a_ok) & act;
    } else if constexpr (!kCache && !kPart) {
      // verify_kernel: nothing comes from a sender cache, so A and R share one joint table (the slot's first 88 granules)
      DevTabJ tj{ta, (int)(tr.stage - ta.stage)};
      good = verify_half_fu_joint(Rw, Aw, Sw, len, msgword, policy, tj, tb0, tb1, wmax, pace) & act;
    } else {
      good = verify_half_fu<false>(Rw, Aw, Sw, len, msgword, policy, ta, tr, tb0, tb1, wmax, pace) & act;
    }
    const uint64_t mask = __ballot(good);
#ifdef AT2V_WAIT_PROBE
    AT2V_WAIT_PROBE_SINK(ta.waited + tr.waited, tb0.waited + tb1.waited, pace.probe[0], pace.probe[1],
                         __builtin_amdgcn_s_memtime() - t_chunk0, ta.lds_waited + tr.lds_waited, pace.probe[2]);
    ta.waited = tr.waited = tb0.waited = tb1.waited = ta.lds_waited = tr.lds_waited = tb0.lds_waited = tb1.lds_waited = 0;
    pace.probe[0] = pace.probe[1] = pace.probe[2] = 0;
#endif
    uint32_t ticket = 0;
    if constexpr (kPart) {  // records in list order
      verdict_or(verdicts, i, good, act, lane);
    } else if (lane == 0) {
      verdicts[2 * c] = (uint32_t)mask;
      if (2 * c + 1 < nwords) verdicts[2 * c + 1] = (uint32_t)(mask >> 32);
    }
    if (lane == 0) {
        ticket = atomicAdd(chunk_queue, 1u);
    }
    ticket = __builtin_amdgcn_readfirstlane(ticket);
    c = ticket < nchunks ? nwaves + ticket : nchunks;  // no wrap: ticket < nchunks <= 2^26
    AT2V_PHASE(6);
  }
}

__global__ __launch_bounds__(kBlock, kVerifyWavesPerSimd) void verify_kernel(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab,
    uint32_t* __restrict__ chunk_queue) {
  __shared__ int4 astage[kWavesPerBlock * 10 * 64];
  __shared__ int4 rstage[kWavesPerBlock * 10 * 64];
  verify_chunks<false>(astage, rstage, pk, sig, msg, msg_total, off, n, cofactorless(policy), verdicts, scratch, btab,
                       chunk_queue, nullptr);
}
__global__ __launch_bounds__(kBlock, kVerifyWavesPerSimd) void verify_kernel_zip215(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab,
    uint32_t* __restrict__ chunk_queue) {
  __shared__ int4 astage[kWavesPerBlock * 10 * 64];
  __shared__ int4 rstage[kWavesPerBlock * 10 * 64];
  verify_chunks<false>(astage, rstage, pk, sig, msg, msg_total, off, n, POLICY_ZIP215, verdicts, scratch, btab,
                       chunk_queue, nullptr);
}

// the same with the per-sender A cache (at2v_opts.sender_cache, tables [j]A)
__global__ __launch_bounds__(kBlock, kVerifyWavesPerSimd) void verify_kernel_cached(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab,
    uint32_t* __restrict__ chunk_queue, CacheArgs c) {
  __shared__ int4 astage[kWavesPerBlock * 10 * 64];
  __shared__ int4 rstage[kWavesPerBlock * 10 * 64];
  verify_chunks<true>(astage, rstage, pk, sig, msg, msg_total, off, n, cofactorless(policy), verdicts, scratch, btab,
                      chunk_queue, &c);
}
__global__ __launch_bounds__(kBlock, kVerifyWavesPerSimd) void verify_kernel_cached_zip215(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab,
    uint32_t* __restrict__ chunk_queue, CacheArgs c) {
  __shared__ int4 astage[kWavesPerBlock * 10 * 64];
  __shared__ int4 rstage[kWavesPerBlock * 10 * 64];
  verify_chunks<true>(astage, rstage, pk, sig, msg, msg_total, off, n, POLICY_ZIP215, verdicts, scratch, btab,
                      chunk_queue, &c);
}

// Partitioned cached launches (at2v_cache.h PartArgs): the ladder over the classify kernel's miss list (sender_comb: the
// comb kernel below takes the hits) or over both lists ([j]A tables: hit chunks skip A's decode and table)
__global__ __launch_bounds__(kBlock, kVerifyWavesPerSimd) void verify_kernel_miss(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab,
    uint32_t* __restrict__ chunk_queue, PartArgs p) {
  __shared__ int4 astage[kWavesPerBlock * 10 * 64];
  __shared__ int4 rstage[kWavesPerBlock * 10 * 64];
  verify_chunks<false, true>(astage, rstage, pk, sig, msg, msg_total, off, n, cofactorless(policy), verdicts, scratch,
                             btab, chunk_queue, nullptr, &p);
}
__global__ __launch_bounds__(kBlock, kVerifyWavesPerSimd) void verify_kernel_miss_zip215(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab,
    uint32_t* __restrict__ chunk_queue, PartArgs p) {
  __shared__ int4 astage[kWavesPerBlock * 10 * 64];
  __shared__ int4 rstage[kWavesPerBlock * 10 * 64];
  verify_chunks<false, true>(astage, rstage, pk, sig, msg, msg_total, off, n, POLICY_ZIP215, verdicts, scratch,
                             btab, chunk_queue, nullptr, &p);
}
__global__ __launch_bounds__(kBlock, kVerifyWavesPerSimd) void verify_kernel_tables_part(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab,
    uint32_t* __restrict__ chunk_queue, CacheArgs c, PartArgs p) {
  __shared__ int4 astage[kWavesPerBlock * 10 * 64];
  __shared__ int4 rstage[kWavesPerBlock * 10 * 64];
  verify_chunks<true, true>(astage, rstage, pk, sig, msg, msg_total, off, n, cofactorless(policy), verdicts, scratch,
                            btab, chunk_queue, &c, &p);
}
__global__ __launch_bounds__(kBlock, kVerifyWavesPerSimd) void verify_kernel_tables_part_zip215(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab,
    uint32_t* __restrict__ chunk_queue, CacheArgs c, PartArgs p) {
  __shared__ int4 astage[kWavesPerBlock * 10 * 64];
  __shared__ int4 rstage[kWavesPerBlock * 10 * 64];
  verify_chunks<true, true>(astage, rstage, pk, sig, msg, msg_total, off, n, POLICY_ZIP215, verdicts, scratch,
                            btab, chunk_queue, &c, &p);
}

// ---------------------------------------------------------------------------------------------------------------
// Low-latency verify for small launches: two lanes per record (lane 2r: A side, lane 2r+1: R side,
// verify_pair_part), 32 records per wave, one wave per SIMD (4-wave blocks, 80 KiB LDS). Each lane decodes one point,
// builds one table and does one addition per window; the partner's cached point comes across by __shfl_xor and both
// lanes evaluate V = P0 + P1 (verify_pair_combine). Chunks c = 32-record groups, grid-strided.
constexpr int kPairBlock = 256;
constexpr int kPairWaves = kPairBlock / 64;
__device__ AT2V_INLINE void verify_pair_chunks(
    int4* pstage, int4* bstage, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig,
    const uint8_t* __restrict__ msg, uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy,
    uint32_t* __restrict__ verdicts, int4* __restrict__ scratch, const int4* __restrict__ btab) {
  const int lane = threadIdx.x & 63;
  const int wib = AT2V_UNIFORM(threadIdx.x >> 6);  // wave-uniform: the LDS stage addresses live in SGPRs
  const int side = lane & 1;
  const uint32_t wave = blockIdx.x * kPairWaves + wib;
  const uint32_t nwaves = gridDim.x * kPairWaves;
  const uint32_t nchunks = (n + 31) / 32;
  int4* slot = scratch + ((size_t)wave * 64 + lane) * kTabAGranules;
  DevTabA tp{slot, pstage + wib * 640, lane, btab + (size_t)kNumBtabs * kBtabEntries * 8};
  const DevTabB tb{btab + (size_t)side * kBtabEntries * 8, bstage + wib * 640, lane};
  auto wmax = [](int v) { return wave_max_i32(v); };
  for (uint32_t c = wave; c < nchunks; c += nwaves) {
    const uint32_t i = c * 32 + (lane >> 1);
    const uint32_t ii = i < n ? i : n - 1;  // tail lanes recompute a real record; their bit is masked
    uint32_t Rw[8], Sw[8], Aw[8];
    load8(Rw, sig + (size_t)ii * 64);
    load8(Sw, sig + (size_t)ii * 64 + 32);
    load8(Aw, pk + (size_t)ii * 32);
    const uint32_t o0 = off[ii];
    const uint32_t len = off[ii + 1] - o0;
    const int msg_fast =
        __builtin_amdgcn_readfirstlane(__all((uint64_t)o0 + len + 8 <= (uint64_t)msg_total) ? 1 : 0);
    const uint32_t* mw = reinterpret_cast<const uint32_t*>(msg) + (o0 >> 2);
    const uint32_t msh = (o0 & 3u) * 8;
    auto msgword = [&](uint32_t j) -> uint32_t {
      if (msg_fast) return __builtin_amdgcn_alignbit(mw[j + 1], mw[j], msh);
      const uint32_t a = o0 + 4 * j;
      const uint32_t a0 = a & ~3u, sh = (a & 3u) * 8;
      const uint32_t lo = load_u32_guarded(msg, a0, msg_total);
      if (sh == 0) return lo;
      const uint32_t hi = load_u32_guarded(msg, a0 + 4, msg_total);
      return __builtin_amdgcn_alignbit(hi, lo, sh);
    };
    gu_p3 Pm;
    int ok = verify_pair_part(side, Rw, Aw, Sw, len, msgword, policy, tp, tb, wmax, Pm);
    gu_cached cm, cp;
    gu_p3_to_cached(cm, Pm);
    const uint32_t* cw = reinterpret_cast<const uint32_t*>(&cm);
    uint32_t* pw = reinterpret_cast<uint32_t*>(&cp);
#pragma unroll
    for (int q = 0; q < 40; ++q) pw[q] = (uint32_t)__shfl_xor((int)cw[q], 1);
    ok &= __shfl_xor(ok, 1);
    const int good = ok & verify_pair_combine(Pm, cp, policy) & (i < n);
    const uint64_t mask = __ballot(good);
    if (lane == 0) {  // record r's verdict is lane 2r's bit: compress the even bits of the ballot
      uint64_t x = mask & 0x5555555555555555ull;
      x = (x | (x >> 1)) & 0x3333333333333333ull;
      x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
      x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull;
      x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
      x = (x | (x >> 16)) & 0x00000000ffffffffull;
      verdicts[c] = (uint32_t)x;
    }
  }
}

__global__ __launch_bounds__(kPairBlock, 1) void verify_pair_kernel(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab) {
  __shared__ int4 pstage[kPairWaves * 10 * 64];
  __shared__ int4 bstage[kPairWaves * 10 * 64];
  verify_pair_chunks(pstage, bstage, pk, sig, msg, msg_total, off, n, cofactorless(policy), verdicts, scratch, btab);
}
__global__ __launch_bounds__(kPairBlock, 1) void verify_pair_kernel_zip215(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab) {
  __shared__ int4 pstage[kPairWaves * 10 * 64];
  __shared__ int4 bstage[kPairWaves * 10 * 64];
  verify_pair_chunks(pstage, bstage, pk, sig, msg, msg_total, off, n, POLICY_ZIP215, verdicts, scratch, btab);
}

size_t cache_entry_bytes() { return (size_t)kCacheEntryGranules * 16; }
size_t cache_payload_bytes(int comb) { return comb ? kCombBytes : (size_t)kTabAGranules * 16; }
size_t bcomb_bytes(int bits) {
  return bits == 24 ? BCombGeom<24>::kBytes : bits == 20 ? BCombGeom<20>::kBytes : BCombGeom<16>::kBytes;
}
int bcomb_lat_bits() { return kBCombLatBits; }
int bcomb_mid_bits() { return kBCombMidBits; }
int bcomb_wide_bits() { return kBCombBits; }

size_t bcomb_scratch_bytes() { return sizeof(gu_cached) * 2 * 16; }

// the comb of B: one table of 2^(bits-1) + 1 entries per position of a 254-bit scalar, table p = [j 2^(bits p)]B
hipError_t launch_build_bcomb(int4* out, int bits, void* scratch, hipStream_t stream) {
  if (bits != 16 && bits != 20 && bits != 24) return hipErrorInvalidValue;
  const int npos = (254 + bits - 1) / bits;  // <= 16
  gu_cached* base = static_cast<gu_cached*>(scratch);
  hipLaunchKernelGGL(bcomb_base_kernel, dim3(1), dim3(64), 0, stream, base, bits, npos);
  hipError_t e = hipGetLastError();
  const uint32_t lanes = ((1u << (bits - 1)) >> kBCombKLog2) * (uint32_t)npos;
  for (uint32_t l0 = 0; l0 < lanes && e == hipSuccess; l0 += kBCombFillLanes) {
    const uint32_t k = lanes - l0 < kBCombFillLanes ? lanes - l0 : kBCombFillLanes;
    hipLaunchKernelGGL(bcomb_fill_kernel, dim3((k + 255) / 256), dim3(256), 0, stream, out, base, bits, npos, l0);
    e = hipGetLastError();
  }
  return e;
}

int cache_ctl_words() { return kCtlWords; }

static uint32_t grid_for(uint64_t items, uint32_t per_block, uint32_t cap_blocks) {
  const uint64_t b = (items + per_block - 1) / per_block;
  return (uint32_t)(b < 1 ? 1 : b > cap_blocks ? cap_blocks : b);
}

hipError_t launch_cache_init(const CacheArgs& c, hipStream_t stream) {
  hipLaunchKernelGGL(cache_init_kernel, dim3(grid_for(c.capacity, 256, 1024)), dim3(256), 0, stream, c);
  return hipGetLastError();
}

hipError_t launch_cache_build(const CacheArgs& c, uint32_t max_claims, hipStream_t stream) {
  if (max_claims == 0) max_claims = 1;
  if (c.comb) {  // a block per claim (few claims) or a wave per claim; the grid loops over more
    hipLaunchKernelGGL(cache_comb_kernel, dim3(max_claims < 512u ? max_claims : 512u), dim3(256), 0, stream, c);
    // (the kernel reads the real claim count: blocks past the keys' blocks (wide) or waves (narrow) exit at once)
  } else {
    hipLaunchKernelGGL(cache_build_kernel, dim3(grid_for(max_claims, 256, 1024)), dim3(256), 0, stream, c);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cache_flip_kernel, dim3(1), dim3(1024), 0, stream, c);
  return hipGetLastError();
}

hipError_t launch_cache_compact(const CacheArgs& c, const CacheCompactArgs& x, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(x.new_tags, 0, (size_t)c.cap * 8, stream);
  if (e == hipSuccess) e = hipMemsetAsync(x.new_entries, 0, (size_t)c.cap * kCacheEntryGranules * 16, stream);
  if (e == hipSuccess) e = hipMemsetAsync(x.used, 0, (size_t)c.capacity * 4, stream);
  static_assert(kCtlHist == kCtlPinned + 1, "the pinned count and the histogram are zeroed as one span");
  if (e == hipSuccess) e = hipMemsetAsync(c.ctl + kCtlPinned, 0, 65 * 8, stream);
  if (e != hipSuccess) return e;
  const uint32_t gs = grid_for(c.cap, 256, 2048), gu = grid_for(c.capacity, 256, 2048);
  hipLaunchKernelGGL(cache_hist_kernel, dim3(gs), dim3(256), 0, stream, c);
  hipLaunchKernelGGL(cache_select_kernel, dim3(1), dim3(1), 0, stream, c, x);
  hipLaunchKernelGGL(cache_compact_kernel, dim3(gs), dim3(256), 0, stream, c, x);
  hipLaunchKernelGGL(cache_freelist_kernel, dim3(gu), dim3(256), 0, stream, c, x);
  return hipGetLastError();
}

hipError_t launch_cache_preload(const CacheArgs& c, const CacheKeyList& l, int pin_op, hipStream_t stream) {
  if (l.n == 0) return hipSuccess;
  hipLaunchKernelGGL(cache_preload_kernel, dim3(grid_for(l.n, 256, 1024)), dim3(256), 0, stream, c, l);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_cache_pin(c, l, pin_op, stream);
}

hipError_t launch_cache_pin(const CacheArgs& c, const CacheKeyList& l, int pin_op, hipStream_t stream) {
  if (l.n == 0) return hipSuccess;
  hipLaunchKernelGGL(cache_pin_kernel, dim3(grid_for(l.n, 256, 1024)), dim3(256), 0, stream, c, l, pin_op);
  return hipGetLastError();
}

hipError_t launch_cache_query(const CacheArgs& c, const CacheKeyList& l, hipStream_t stream) {
  if (l.n == 0) return hipSuccess;
  hipLaunchKernelGGL(cache_query_kernel, dim3(grid_for(l.n, 256, 1024)), dim3(256), 0, stream, c, l);
  return hipGetLastError();
}

// ------------------------------------------------------------------ launchers (host side)

// the B tables, then (kIdentShared) the shared identity entry in cached form: YpX = 1, YmX = 1, Z2 = 2, T2d = 0
size_t btab_bytes() { return (size_t)kNumBtabs * kBtabEntries * 8 * 16 + 160; }

// table t (t = 0: [j]B; t = 1: [j 2^128]B for the half-size path) at out + t * kBtabEntries * 8
hipError_t launch_build_btab(int4* out, hipStream_t stream) {
  for (int t = 0; t < kNumBtabs; ++t) {
    hipLaunchKernelGGL(build_btab_kernel, dim3((kBtabEntries + kBlock - 1) / kBlock), dim3(kBlock), 0, stream,
                       out + (size_t)t * kBtabEntries * 8, 4 * t);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  static const uint32_t ident[40] = {1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0,
                                     0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const hipError_t e = hipMemcpyAsync(out + (size_t)kNumBtabs * kBtabEntries * 8, ident, sizeof ident,
                                      hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(stream);  // `ident` is a host array of this function's lifetime: wait for the copy
}

size_t part_bytes_per_record() { return 12; }  // hidx, hinfo, midx

// a ZIP215 context launches the kernel's cofactored twin (`policy` is launch_verify's)
#define AT2V_LAUNCH_VERIFY(kernel, ...)                                             \
  do {                                                                              \
    if (policy == POLICY_ZIP215) hipLaunchKernelGGL(kernel##_zip215, __VA_ARGS__); \
    else hipLaunchKernelGGL(kernel, __VA_ARGS__);                                  \
  } while (0)

hipError_t launch_verify(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint32_t msg_total,
                         const uint32_t* off, uint32_t n, int policy, uint32_t* verdicts, int4* scratch,
                         const int4* btab, int grid, uint32_t pair_max, hipStream_t stream,
                         const CacheArgs* cache, const PartArgs* part, int dense) {
  if (n == 0) return hipSuccess;
  if (n <= pair_max && !(cache && cache->comb)) {  // (with combs, small batches take the comb kernel: faster still)
    // one wave (32 records) per SIMD: 4-wave blocks; the context's scratch holds grid x 8 waves of (larger) slots
    const uint32_t nchunks = (n + 31) / 32;
    const uint32_t cap_blocks = (uint32_t)grid * kWavesPerBlock / kPairWaves;
    uint32_t g = (nchunks + kPairWaves - 1) / kPairWaves;
    g = g < cap_blocks ? g : cap_blocks;
    AT2V_LAUNCH_VERIFY(verify_pair_kernel, dim3(g), dim3(kPairBlock), 0, stream, pk, sig, msg, msg_total, off, n,
                       policy, verdicts, scratch, btab);
    return hipGetLastError();
  }
  const uint32_t nchunks = (n + 63) / 64;
  // Blocks: a launch below the full grid spreads its chunks over twice as many blocks, half filled (one wave per SIMD:
  // the lowest latency for a lone batch); `dense` (the host-buffer pipeline's chunk launches, at2v_api.hip HostPipe)
  // fills every block, so a small launch takes few whole CUs at full rate and leaves the rest to the launch beside it
  // (1M records as 16 launches of 65,536: 13.3 ms half filled, one stream; profiles/r06/r06i)
  const uint32_t per_block = dense ? kWavesPerBlock : kWavesPerBlock / 2;
  const uint32_t need_blocks = (nchunks + per_block - 1) / per_block;
  const int g = (int)((uint32_t)grid < need_blocks ? (uint32_t)grid : need_blocks);
  // chunk queue counter: the word after the `grid` blocks' lane slots (scratch_bytes(grid)); the four-wave comb kernel of
  // small batches strides over its chunks and needs none (one dependent memset less on the latency path)
  uint32_t* queue =
      reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(scratch) + (size_t)grid * scratch_bytes_per_block());
  const bool lat_comb = cache && cache->comb && n <= pair_max;
  const bool parted = cache && part && n > pair_max;  // (zeroes its control words itself, below)
  if (!lat_comb && !parted) {
    const hipError_t me = hipMemsetAsync(queue, 0, sizeof(uint32_t), stream);
    if (me != hipSuccess) return me;
  }
  if (cache && part && n > pair_max) {
    // partitioned (at2v_cache.h PartArgs): classify -> (combs) hit list by comb additions -> ladder over the rest. The
    // control words after the lane slots: [0] the ladder's chunk queue, [1] the comb kernel's, [4..5] the list sizes.
    PartArgs pa = *part;
    pa.counts = queue + 4;
    hipError_t e = hipMemsetAsync(queue, 0, 8 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint32_t groups = (n + 63) / 64, per_block = kClassifyWaves * kClassifyGroups;
    hipLaunchKernelGGL(cache_classify_kernel, dim3((groups + per_block - 1) / per_block), dim3(64 * kClassifyWaves), 0,
                       stream, pk, n, *cache, pa);
    if (cache->comb) {
      const uint32_t need2 = ((n + 255) / 256 + kWavesPerBlock / 2 - 1) / (kWavesPerBlock / 2);
      const int g2 = (int)((uint32_t)grid < need2 ? (uint32_t)grid : need2);
      AT2V_LAUNCH_VERIFY(verify_kernel_comb_part, dim3(g2), dim3(kBlock), 0, stream, pk, sig, msg, msg_total, off, n,
                         policy, verdicts, scratch, btab, queue + 1, *cache, pa);
      AT2V_LAUNCH_VERIFY(verify_kernel_miss, dim3(g), dim3(kBlock), 0, stream, pk, sig, msg, msg_total, off, n, policy,
                         verdicts, scratch, btab, queue, pa);
    } else {
      AT2V_LAUNCH_VERIFY(verify_kernel_tables_part, dim3(g), dim3(kBlock), 0, stream, pk, sig, msg, msg_total, off, n,
                         policy, verdicts, scratch, btab, queue, *cache, pa);
    }
    return hipGetLastError();
  }
  if (cache) {  // the kernels look their senders up themselves (at2v_cache.h); builds follow on the build stream
    if (cache->comb && n <= pair_max) {  // small batches: the four-wave split, one block per 64 records
      const uint32_t gl = nchunks < (uint32_t)grid ? nchunks : (uint32_t)grid;
      AT2V_LAUNCH_VERIFY(verify_comb_lat_kernel, dim3(gl), dim3(kLatBlock), 0, stream, pk, sig, msg, msg_total, off, n,
                         policy, verdicts, scratch, btab, *cache);
      return hipGetLastError();
    }
    if (cache->comb) {
      const uint32_t crec = 256u;  // records per chunk (verify_chunks_comb4)
      const uint32_t need2 = ((n + crec - 1) / crec + kWavesPerBlock / 2 - 1) / (kWavesPerBlock / 2);
      const int g2 = (int)((uint32_t)grid < need2 ? (uint32_t)grid : need2);
      AT2V_LAUNCH_VERIFY(verify_kernel_comb, dim3(g2), dim3(kBlock), 0, stream, pk, sig, msg, msg_total, off, n, policy,
                         verdicts, scratch, btab, queue, *cache);
      return hipGetLastError();
    }
    AT2V_LAUNCH_VERIFY(verify_kernel_cached, dim3(g), dim3(kBlock), 0, stream, pk, sig, msg, msg_total, off, n, policy,
                       verdicts, scratch, btab, queue, *cache);
    return hipGetLastError();
  }
  AT2V_LAUNCH_VERIFY(verify_kernel, dim3(g), dim3(kBlock), 0, stream, pk, sig, msg, msg_total, off, n, policy,
                     verdicts, scratch, btab, queue);
  return hipGetLastError();
}

hipError_t launch_gen(uint64_t cfg, uint64_t first, uint32_t n, uint32_t msg_len, uint64_t senders,
                      const uint64_t* keys, uint8_t* pk, uint8_t* sig, uint8_t* msg, uint32_t* off, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(gen_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, cfg, first, n, msg_len,
                     senders, keys, pk, sig, msg, off);
  return hipGetLastError();
}

hipError_t launch_sign(const uint8_t* seeds, const uint8_t* msg, uint32_t msg_total, const uint32_t* off, uint32_t n,
                       uint8_t* pk, uint8_t* sig, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(sign_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, seeds, msg, msg_total, off,
                     n, pk, sig);
  return hipGetLastError();
}

hipError_t launch_decode(const uint8_t* pts, uint32_t n, uint32_t* out, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(decode_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, pts, n, out);
  return hipGetLastError();
}

hipError_t verify_occupancy(int* blocks_per_cu, int* vgprs) {
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, verify_kernel, kBlock, 0);
  if (e != hipSuccess) return e;
  hipFuncAttributes attr;
  e = hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(verify_kernel));
  if (e == hipSuccess && vgprs) *vgprs = attr.numRegs;
  return e;
}

size_t scratch_bytes_per_block() { return kScratchPerWave * kWavesPerBlock; }
// device scratch of a context launching `grid` blocks: their lane slots + the chunk queue counter
size_t scratch_bytes(int grid) { return (size_t)grid * scratch_bytes_per_block() + kCtlBytes(grid); }
int block_threads() { return kBlock; }

}  // namespace at2v

#ifdef AT2V_COMB_PROBE
// probe builds only: copy out the comb kernel's probe sums (at2v::kCpN counters) and zero them
extern "C" int at2v_probe_read(unsigned long long* out, int n) {
  if (n < (int)at2v::kCpN) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(at2v::at2v_cprobe_acc), sizeof(unsigned long long) * at2v::kCpN) !=
      hipSuccess)
    return -3;
  unsigned long long z[at2v::kCpN] = {};
  if (hipMemcpyToSymbol(HIP_SYMBOL(at2v::at2v_cprobe_acc), z, sizeof(z)) != hipSuccess) return -4;
  return (int)at2v::kCpN;
}
#endif
