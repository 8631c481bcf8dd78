// at2v_kern_comb.h — verify from per-key combs (at2v_opts.sender_comb): the four-wave low-latency kernel and the
// throughput kernels.
// A piece of the kernels translation unit: at2v_kernels.hip includes the at2v_kern_*.h pieces in order (tables, cache,
// comb, sign, btab) and compiles them with its own kernels and launchers into one object. Each piece uses only the
// shared headers and the pieces before it.
#pragma once
#include <hip/hip_runtime.h>

#include "at2v_cache.h"
#include "at2v_comb.h"
#include "at2v_kern_tables.h"
#include "at2v_kern_cache.h"

namespace at2v {

// LDS words of the four-wave split check (in the kernel's `part` array, word-major: [word][lane])
constexpr int kSplitDig = 0;          // c0 digits (8 words), |c1| digits (8 words)
constexpr int kSplitFlags = 16 * 64;  // bit 0: the lattice / window check, bit 1: c1 < 0
constexpr int kSplitP1 = 40 * 64;     // [c1]R, cached form (40 words)
constexpr int kSplitPb = 80 * 64;     // -[t]B, cached form (40 words)

// Low-latency verify from combs (at2v_opts.sender_comb, launches of <= small_batch_max records): a block of 4 waves (one
// per SIMD) owns a chunk of 64 records. Wave 0 looks the chunk's senders up (claiming new keys for the build stream) and
// hands each record's entry (payload index or -1, decode verdict) to the other waves through LDS, so all four waves take
// the same branch. A chunk whose records all hit splits each record's work by wave (at2v_comb.h, comb_check_split):
//   wave 0: decode R and check its canonicity (one exponentiation), then, after the barrier, R' = Pa0 + Pa1 + Pb and
//           the projective comparison -> verdict words
//   wave 1: s < l, the kBCombPos (11) B-comb additions -> Pb
//   wave 2: SHA-512 -> k, A-comb positions 0..15 -> Pa0;   wave 3: SHA-512 -> k, positions 16..31 -> Pa1
// so a record's latency is the longest part (SHA-512 + 13 additions) instead of SHA-512 + 37 additions + an inversion.
// Any other chunk (a sender seen for the first time: its comb is built on the build stream after this launch and serves
// later launches; a claim without a payload; a probe failure) runs the half-size check V = [c0]A + [c1]R - [t]B = 0
//  split over the four waves: wave 0 decodes A and builds [j]A, wave 1 decodes R and builds [j]R while
// wave 2 hashes (SHA-512 -> k), reduces the lattice (c0, c1, t) and hands the digits over LDS; then wave 0 runs the
// [c0]A ladder, wave 1 the [c1]R ladder (four doublings and one addition per window), wave 2 adds [t]B from the comb of
// B, and wave 0 checks the sum. The chain of a record is then decode + table + one 128-bit ladder, instead of SHA-512,
// the lattice and the fixed-base additions on top (the two-lane split of the pair kernel). A first-seen
// sender costs this instead of waiting for its comb (round 3: 0.82-0.94 ms of device time, profiles/r03zg).
// Verdict words are written by wave 0's lane 0 for every chunk.
constexpr int kLatBlock = 256;
__device__ AT2V_INLINE void verify_comb_lat_chunks(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab, CacheArgs c) {
  __shared__ int4 stage[4 * 2 * 640];        // per wave two 10 KiB LDS-DMA stages
  __shared__ uint32_t part[3 * 40 * 64];      // Pb, Pa0, Pa1 (p3, 40 words) per lane, word-major; or the R side's P1
  __shared__ uint32_t sok[64];                // wave 1's s < l, or the R side's checks
  __shared__ int sent[2 * 64];                // wave 0's cache outcome per record: payload index (-1: miss), A verdict
  __shared__ int snw;                         // split check: the chunk's window count (wave 2)
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int4* st0 = stage + (size_t)w * 2 * 640;
  int4* st1 = st0 + 640;
  const uint32_t nchunks = (n + 63) / 64, nwords = (n + 31) / 32;
  auto wmax = [](int v) { return wave_max_i32(v); };
  for (uint32_t c0 = blockIdx.x; c0 < nchunks; c0 += gridDim.x) {
    const uint32_t i = c0 * 64 + lane;
    const uint32_t ii = i < n ? i : n - 1;
    uint32_t Rw[8], Sw[8], Aw[8];
    load8(Rw, sig + (size_t)ii * 64);
    load8(Sw, sig + (size_t)ii * 64 + 32);
    load8(Aw, pk + (size_t)ii * 32);
    if (w == 0) {
      const int slot = cache_lookup_wave(c, Aw, lane, i < n);
      int a_ok0 = 0, u0 = 0;
      const bool hit0 = cache_hit(c, slot, Aw, a_ok0, u0);
      sent[lane] = hit0 ? u0 : -1;
      sent[64 + lane] = a_ok0;
    }
    __syncthreads();
    const int u = sent[lane], a_ok = sent[64 + lane];
    const int all_hit = __builtin_amdgcn_readfirstlane(__all(u >= 0) ? 1 : 0);  // the same in every wave (LDS)
    if (w == 0 && lane == 0) {
      atomicAdd(c.ctl + kCtlChunks, 1ull);
      if (all_hit) atomicAdd(c.ctl + kCtlChunkHits, 1ull);
    }
    const uint32_t o0 = off[ii];
    const uint32_t len = off[ii + 1] - o0;
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
    gu_p3 R;   // all-hit: wave 0's decoded R;  fallback: wave 0's decoded A, then [c0]A
    int ok0 = 0;
    uint32_t td[kBCombLatDigitWords];  // fallback, wave 2: t's digits for the (low-latency) comb of B
    int4* slot = scratch + (((size_t)blockIdx.x * kWavesPerBlock + w) * 64 + lane) * kLaneGranules;
    const DevTabA tp{slot, st0, lane, btab + (size_t)kNumBtabs * kBtabEntries * 8};
    if (all_hit) {
      if (w == 0) {
        ok0 = comb_decode_r(R, Rw, policy) & comb_prechecks(Rw, Aw, Sw, policy, a_ok);
      } else {
        gu_p3 P;
        gu_p3_identity(P);
        if (w == 1) {
          sok[lane] = (uint32_t)sc_v1_ok(Sw, policy);
          uint32_t sd[kBCombLatDigitWords];
          bcomb_recode<kBCombLatBits>(sd, Sw);
          const DevBCombLat tb{c.bcomb_lat, {st0, st1}, lane};
          comb_sum<false>(P, sd, 0, kBCombLatPos, tb);
        } else {
          uint32_t kd[kCombDigitWords];
          comb_k_digits(kd, Rw, Aw, len, msgword);
          const DevComb tc{c.payload + (size_t)u * (kCombBytes / 16), {st0, st1}, lane};
          comb_sum<true>(P, kd, w == 2 ? 0 : kCombPos / 2, w == 2 ? kCombPos / 2 : kCombPos, tc);
        }
        const uint32_t* pw = reinterpret_cast<const uint32_t*>(&P);
        uint32_t* dst = part + (size_t)(w - 1) * 40 * 64;
#pragma unroll
        for (int q = 0; q < 40; ++q) dst[q * 64 + lane] = pw[q];
      }
    } else if (w == 0) {  // split check, phase 1: V1, the policy pre-checks, A decoded (dalek rules) and [j]A
      ok0 = split_a_side(R, Rw, Aw, Sw, policy, tp);
    } else if (w == 1) {  // R canonical and decoded, [j]R (c1's sign is applied per digit in phase 2)
      sok[lane] = (uint32_t)split_r_side(Rw, tp, policy);
    } else if (w == 2) {  // k = SHA-512(R || A || M) mod l, the lattice (c0, c1), t = c1 s mod l: digits to LDS
      uint32_t c0d[8], c1d[8];
      int c1_neg, nw_lane;
      const int okl = split_scalars(c0d, c1d, td, c1_neg, nw_lane, Rw, Aw, Sw, len, msgword);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        part[kSplitDig + q * 64 + lane] = c0d[q];
        part[kSplitDig + (8 + q) * 64 + lane] = c1d[q];
      }
      part[kSplitFlags + lane] = (uint32_t)okl | ((uint32_t)c1_neg << 1);
      const int nw = wmax(nw_lane);
      if (lane == 0) snw = nw < 1 ? 1 : nw;
    }
    __syncthreads();
    if (!all_hit) {  // split check, phase 2: the two ladders and [t]B
      if (w < 2) {
        uint32_t cd[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) cd[q] = part[kSplitDig + (8 * w + q) * 64 + lane];
        const int flip = w == 1 ? (int)(part[kSplitFlags + lane] >> 1) & 1 : 0;
        gu_p3 P;
        split_side_ladder(P, cd, snw, flip, tp);
        if (w == 0) {
          R = P;
        } else {
          gu_cached cm;
          gu_p3_to_cached(cm, P);
          const uint32_t* cw = reinterpret_cast<const uint32_t*>(&cm);
#pragma unroll
          for (int q = 0; q < 40; ++q) part[kSplitP1 + q * 64 + lane] = cw[q];
        }
      } else if (w == 2) {
        gu_cached cm;
        split_neg_tb(cm, td, DevBCombLat{c.bcomb_lat, {st0, st1}, lane});  // -[t]B
        const uint32_t* cw = reinterpret_cast<const uint32_t*>(&cm);
#pragma unroll
        for (int q = 0; q < 40; ++q) part[kSplitPb + q * 64 + lane] = cw[q];
      }
    }
    __syncthreads();
    if (w == 0) {
      int good;
      if (all_hit) {
        gu_p3 Pb, Pa0, Pa1;
        uint32_t* pb = reinterpret_cast<uint32_t*>(&Pb);
        uint32_t* p0 = reinterpret_cast<uint32_t*>(&Pa0);
        uint32_t* p1 = reinterpret_cast<uint32_t*>(&Pa1);
#pragma unroll
        for (int q = 0; q < 40; ++q) {
          pb[q] = part[q * 64 + lane];
          p0[q] = part[40 * 64 + q * 64 + lane];
          p1[q] = part[80 * 64 + q * 64 + lane];
        }
        good = ok0 & (int)sok[lane] & comb_check_split(R, Pa0, Pa1, Pb, policy) & (i < n);
      } else {  // V = [c0]A + [c1]R - [t]B == identity
        gu_cached c1r, cnb;
        uint32_t* w1 = reinterpret_cast<uint32_t*>(&c1r);
        uint32_t* w2 = reinterpret_cast<uint32_t*>(&cnb);
#pragma unroll
        for (int q = 0; q < 40; ++q) {
          w1[q] = part[kSplitP1 + q * 64 + lane];
          w2[q] = part[kSplitPb + q * 64 + lane];
        }
        good = ok0 & (int)sok[lane] & (int)(part[kSplitFlags + lane] & 1) &
               split_combine(R, c1r, cnb, policy) & (i < n);
      }
      const uint64_t mask = __ballot(good);
      if (lane == 0) {
        verdicts[2 * c0] = (uint32_t)mask;
        if (2 * c0 + 1 < nwords) verdicts[2 * c0 + 1] = (uint32_t)(mask >> 32);
      }
    }
    __syncthreads();  // the LDS parts are reused by the block's next chunk
  }
}

// (two kernels over one body, as every verify kernel: at2v_kernels.hip)
__global__ __launch_bounds__(kLatBlock, 1) void verify_comb_lat_kernel(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab, CacheArgs c) {
  verify_comb_lat_chunks(pk, sig, msg, msg_total, off, n, cofactorless(policy), verdicts, scratch, btab, c);
}
__global__ __launch_bounds__(kLatBlock, 1) void verify_comb_lat_kernel_zip215(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab, CacheArgs c) {
  verify_comb_lat_chunks(pk, sig, msg, msg_total, off, n, POLICY_ZIP215, verdicts, scratch, btab, c);
}

// The message reader of one record (verify_chunks' MsgSplit: the fast form when the wave's messages all end 8 bytes
// before the buffer end), handed to body(msgword). A plain function, so the comb path below inlines it (as lambdas the
// compiler outlined these bodies into calls).
template <class Body>
__device__ AT2V_INLINE int with_msg_reader(const uint8_t* __restrict__ msg, uint32_t msg_total, uint32_t b0, uint32_t bl,
                                           Body&& body) {
  const int msg_fast = __builtin_amdgcn_readfirstlane(__all((uint64_t)b0 + bl + 8 <= (uint64_t)msg_total) ? 1 : 0);
  const uint32_t* mw = reinterpret_cast<const uint32_t*>(msg) + (b0 >> 2);
  const uint32_t msh = (b0 & 3u) * 8;
  auto msg_unguarded = [=](uint32_t j) -> uint32_t { return __builtin_amdgcn_alignbit(mw[j + 1], mw[j], msh); };
  auto msg_guarded = [=](uint32_t j) -> uint32_t {
    const uint32_t a = b0 + 4 * j;
    const uint32_t a0 = a & ~3u, sh = (a & 3u) * 8;
    const uint32_t lo = load_u32_guarded(msg, a0, msg_total);
    if (sh == 0) return lo;
    const uint32_t hi = load_u32_guarded(msg, a0 + 4, msg_total);
    return __builtin_amdgcn_alignbit(hi, lo, sh);
  };
  auto touched = [] {};
  MsgSplit<decltype(msg_unguarded), decltype(msg_guarded), decltype(touched)> msgword{msg_fast, msg_unguarded,
                                                                                      msg_guarded, touched};
  return body(msgword);
}

// R' of record i (clamped to the batch) from its key's comb; returns the checks that need no point arithmetic, and
// under POLICY_ZIP215 the whole verdict (comb_cofactored_ok: the callers then skip the encoding and its inversion)
template <class TabBC>
__device__ AT2V_INLINE int comb2_point(gu_p3& P, uint32_t i, uint32_t n, const uint8_t* __restrict__ pk,
                                       const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
                                       uint32_t msg_total, const uint32_t* __restrict__ off, int policy, int a_ok,
                                       const int4* __restrict__ comb_key, const TabBC& tbc, int4* sa, int4* sr,
                                       int lane
#ifdef AT2V_COMB_PROBE
                                       , CombProbe* pr = nullptr
#endif
) {
  const uint32_t ii = i < n ? i : n - 1;
  uint32_t Rw[8], Sw[8], Aw[8];
  int ok;
  uint32_t o0, len;
#ifdef AT2V_COMB_PROBE
  unsigned long long dummy = 0;
  unsigned long long& p_rec = pr ? pr->v[kCpRecord] : dummy;
  (void)p_rec;
#endif
  AT2V_CPROBE(p_rec, {
    load8(Rw, sig + (size_t)ii * 64);
    load8(Sw, sig + (size_t)ii * 64 + 32);
    load8(Aw, pk + (size_t)ii * 32);
    o0 = off[ii];
    len = off[ii + 1] - o0;
    ok = comb_prechecks(Rw, Aw, Sw, policy, a_ok);
  });
  const DevComb tc{comb_key, {sa, sr}, lane};
  with_msg_reader(msg, msg_total, o0, len, [&](auto& mwd) {
#ifdef AT2V_COMB_PROBE
    if (pr) {  // comb_point with its two phases timed apart
      uint32_t kd[kCombDigitWords], sd[BCombGeom<TabBC::kBits>::kDigitWords];
      AT2V_CPROBE(pr->v[kCpSha], {
        comb_k_digits(kd, Rw, Aw, len, mwd);
        bcomb_recode<TabBC::kBits>(sd, Sw);
      });
      AT2V_CPROBE(pr->v[kCpSums], {
        gu_p3_identity(P);
        comb_sum<true>(P, kd, 0, kCombPos, tc);
        comb_sum<false>(P, sd, 0, BCombGeom<TabBC::kBits>::kPos, tbc);
      });
      return 0;
    }
#endif
    comb_point(P, Rw, Aw, Sw, len, mwd, tc, tbc);
    return 0;
  });
#ifdef AT2V_COMB_PROBE
  if (pr) {
    pr->v[kCpAWait] += tc.waited;
    pr->v[kCpStage] += tc.stage_waited;
    pr->v[kCpLds] += tc.lds_waited;
  }
#endif
  if (policy == POLICY_ZIP215) ok &= comb_cofactored_ok(P, Rw);
  return ok;
}

// comb2_point with the record's offset and length already known (the hit loop loads them with the list) and the message
// staged in LDS: its words go to the wave's second comb stage by LDS-DMA (one global_load_lds_dword per word, issued
// together with the loads of R, S and A), so the record pays one memory latency before SHA-512 instead of one for its
// loads and one per message block. Used when every lane's message (with one word of alignment slack) fits the stage's
// kMsgStageWords words and ends 8 bytes before the buffer end (the unguarded reader's condition); returns -1 without
// doing anything otherwise (the caller falls back to comb2_point).
constexpr int kMsgStageWords = 40;  // the 10 KiB stage: 40 words x 64 lanes x 4 B
template <class TabBC>
__device__ AT2V_INLINE int comb2_point_staged(gu_p3& P, uint32_t ii, uint32_t o0, uint32_t len,
                                              const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig,
                                              const uint8_t* __restrict__ msg, uint32_t msg_total, int policy, int a_ok,
                                              const int4* __restrict__ comb_key, const TabBC& tbc, int4* sa,
                                              int4* sr, int lane
#ifdef AT2V_COMB_PROBE
                                              , CombProbe* pr = nullptr
#endif
) {
  const uint32_t kl = (len >> 2) + 2;  // words 0 .. (len >> 2) + 1 of the aligned window (the reader reads j and j + 1)
  const int fits = __builtin_amdgcn_readfirstlane(
      __all((uint64_t)o0 + len + 8 <= (uint64_t)msg_total && kl <= (uint32_t)kMsgStageWords) ? 1 : 0);
  if (!fits) return -1;
  const int kw = wave_max_i32((int)kl);
  const uint32_t* mw = reinterpret_cast<const uint32_t*>(msg + (o0 & ~3u));
  uint32_t* const ml = reinterpret_cast<uint32_t*>(sr);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the stage's earlier LDS reads are done
#pragma unroll 1
  for (int j = 0; j < kw; ++j)  // word j of every lane's window -> ml[j * 64 + lane] (a lane past its window re-reads
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(mw + ((uint32_t)j < kl ? (uint32_t)j : kl - 1)),
                                     (__attribute__((address_space(3))) void*)(ml + j * 64), 4, 0, 0);  // its last)
  uint32_t Rw[8], Sw[8], Aw[8];
  int ok;
#ifdef AT2V_COMB_PROBE
  unsigned long long dummy = 0;
  unsigned long long& p_rec = pr ? pr->v[kCpRecord] : dummy;
  (void)p_rec;
#endif
  AT2V_CPROBE(p_rec, {
    load8(Rw, sig + (size_t)ii * 64);
    load8(Sw, sig + (size_t)ii * 64 + 32);
    load8(Aw, pk + (size_t)ii * 32);
    ok = comb_prechecks(Rw, Aw, Sw, policy, a_ok);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the staged message words have landed
  });
  const uint32_t msh = (o0 & 3u) * 8;
  auto staged = [=](uint32_t j) -> uint32_t {
    return __builtin_amdgcn_alignbit(ml[(j + 1) * 64 + lane], ml[j * 64 + lane], msh);
  };
  const DevComb tc{comb_key, {sa, sr}, lane};
#ifdef AT2V_COMB_PROBE
  if (pr) {
    uint32_t kd[kCombDigitWords], sd[BCombGeom<TabBC::kBits>::kDigitWords];
    AT2V_CPROBE(pr->v[kCpSha], {
      comb_k_digits(kd, Rw, Aw, len, staged);
      bcomb_recode<TabBC::kBits>(sd, Sw);
    });
    AT2V_CPROBE(pr->v[kCpSums], {
      gu_p3_identity(P);
      comb_sum<true>(P, kd, 0, kCombPos, tc);
      comb_sum<false>(P, sd, 0, BCombGeom<TabBC::kBits>::kPos, tbc);
    });
    pr->v[kCpAWait] += tc.waited;
    pr->v[kCpStage] += tc.stage_waited;
    pr->v[kCpLds] += tc.lds_waited;
    if (policy == POLICY_ZIP215) ok &= comb_cofactored_ok(P, Rw);
    return ok;
  }
#endif
  comb_point(P, Rw, Aw, Sw, len, staged, tc, tbc);
  if (policy == POLICY_ZIP215) ok &= comb_cofactored_ok(P, Rw);
  return ok;
}

// Four records per lane: a chunk is 256 records, lane l verifies 256c + l + 64q, q = 0..3. All-hit
// chunks share ONE inversion among the four R' (Montgomery's trick over Z0 Z1 Z2 Z3): 63.5 S + 5 M per record instead of
// 127 S + 7 M with two records per lane (~9% of the comb path's multiplications). R'0 and R'1 are parked (X, Y, Z) in the
// lane's scratch slot while R'2 and R'3 are summed, and reloaded for their encodings. Other chunks run the four quarters
// through the half-size ladder.
// kPart: the chunks are 256 entries of the classify kernel's hit list (every record cached), verdict bits set by atomic
// OR; no ladder branch.
template <bool kPart = false, bool kZip = false>
__device__ AT2V_INLINE void verify_chunks_comb4(
    int4* astage, int4* rstage, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig,
    const uint8_t* __restrict__ msg, uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy,
    uint32_t* __restrict__ verdicts, int4* __restrict__ scratch, const int4* __restrict__ btab,
    uint32_t* __restrict__ chunk_queue, const CacheArgs& cc, const PartArgs* pp = nullptr) {
  const int lane = threadIdx.x & 63;
  const int wib = AT2V_UNIFORM(threadIdx.x >> 6);
  const uint32_t wave = blockIdx.x * kWavesPerBlock + wib;
  const uint32_t nwaves = gridDim.x * kWavesPerBlock;
  uint32_t nchunks = (n + 255) / 256, nh = 0;
  if constexpr (kPart) {
    nh = __builtin_amdgcn_readfirstlane(pp->counts[0]);
    nchunks = (nh + 255) / 256;
  }
  const int4* __restrict__ comb = cc.payload;
  const uint32_t nwords = (n + 31) / 32;
  int4* slot = scratch + ((size_t)wave * 64 + lane) * kLaneGranules;
  const int4* ident = btab + (size_t)kNumBtabs * kBtabEntries * 8;
  int4* const sa = astage + wib * 640;
  int4* const sr = rstage + wib * 640;
  DevTabA ta{slot, sa, lane, ident};
  DevTabA tr{slot + kTabAGranules, sr, lane, ident};
  const DevTabB tb0{btab, sa, lane};
  const DevTabB tb1{btab + (size_t)kBtabEntries * 8, sr, lane};
  const DevBCombLat tbc{cc.bcomb_lat, {sa, sr}, lane};
  auto wmax = [](int v) { return wave_max_i32(v); };
  constexpr uint32_t kHalf = kWavesPerBlock / 2;
  const uint32_t c_first = wib < (int)kHalf ? blockIdx.x * kHalf + wib
                                            : gridDim.x * kHalf + blockIdx.x * kHalf + (wib - kHalf);
  auto clamp = [n](uint32_t i) { return i < n ? i : n - 1; };
  // kZip: the ZIP215 twin (at2v_kernels.hip). `policy` is captured by reference below (the ladder branch's message
  // reader), so it lives in memory and a value passed in could not be seen through: the policy the two branches use is
  // formed where it is used, from the template argument or with cofactorless() (at2v_kern_tables.h)
  const int pol = kZip ? POLICY_ZIP215 : cofactorless(policy);
#ifdef AT2V_COMB_PROBE
  CombProbe probe;
  CombProbe* const pr = kPart ? &probe : nullptr;
#define AT2V_CP_ARG , pr
#else
#define AT2V_CP_ARG
#endif
  for (uint32_t c = c_first; c < nchunks;) {
#ifdef AT2V_COMB_PROBE
    const unsigned long long t_chunk0 = __builtin_amdgcn_s_memtime();
#endif
    const uint32_t i0 = c * 256 + lane;
    int a_ok[4], cidx[4];
    uint32_t rec[4];  // the four records of the lane
    int all_hit;
    if constexpr (kPart) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t pos = i0 + 64 * q, pc = pos < nh ? pos : nh - 1;
        rec[q] = pp->hidx[pc];
        const uint32_t info = pp->hinfo[pc];
        a_ok[q] = (int)(info & 1u);
        cidx[q] = (int)(info >> 1);
      }
#ifdef AT2V_COMB_PROBE
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the first use waits for them in the product build)
      probe.v[kCpBook] += __builtin_amdgcn_s_memtime() - t_chunk0;
#endif
      all_hit = 1;
    } else {
      int hit = 1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {  // every quarter's sender looked up (new keys claimed for the build stream)
        uint32_t Aw[8];
        rec[q] = clamp(i0 + 64 * q);
        load8(Aw, pk + (size_t)rec[q] * 32);
        hit &= cache_hit(cc, cache_lookup_wave(cc, Aw, lane, i0 + 64 * q < n), Aw, a_ok[q], cidx[q]) ? 1 : 0;
      }
      all_hit = __builtin_amdgcn_readfirstlane(__all(hit) ? 1 : 0);
      if (lane == 0) {
        atomicAdd(cc.ctl + kCtlChunks, 4ull);
        if (all_hit) atomicAdd(cc.ctl + kCtlChunkHits, 4ull);
      }
    }
    const uint32_t lim = kPart ? nh : n;  // list / batch positions below lim are real
    int good[4] = {0, 0, 0, 0};
    if (kPart || all_hit) {
      // ONE inlined copy of the per-record work, run four times: R'_q = comb sums of record q, parked in the slot (X, Y,
      // Z at granules 8q..8q+7). Four unrolled copies made the kernel 400 KB of code, whose hot loops (four copies of
      // SHA-512 and of the A and B comb loops) did not share the instruction cache between waves at different records.
      int okm = 0;
#pragma unroll 1
      for (int q = 0; q < 4; ++q) {
        const uint32_t rq = q == 0 ? rec[0] : q == 1 ? rec[1] : q == 2 ? rec[2] : rec[3];
        const int aq = q == 0 ? a_ok[0] : q == 1 ? a_ok[1] : q == 2 ? a_ok[2] : a_ok[3];
        const int cq = q == 0 ? cidx[0] : q == 1 ? cidx[1] : q == 2 ? cidx[2] : cidx[3];
        gu_p3 P;
        const int okq = comb2_point(P, rq, n, pk, sig, msg, msg_total, off, pol, aq,
                                    comb + (size_t)cq * (kCombBytes / 16), tbc, sa, sr, lane AT2V_CP_ARG);
        okm |= okq << q;
        slot_store(slot + 8 * q, reinterpret_cast<const int32_t*>(&P), 30);  // X, Y, Z (T not needed)
      }
#ifdef AT2V_COMB_PROBE
      const unsigned long long t_fin0 = __builtin_amdgcn_s_memtime();
#endif
      // POLICY_ZIP215 (wave-uniform): comb2_point's verdicts are final, nothing is encoded and nothing inverted
      int goodm = okm;
      if (pol != POLICY_ZIP215) {
        // Montgomery's trick: 1/Z_q = Z_{q^1} / (Z_q Z_{q^1}), and 1/(Z0 Z1), 1/(Z2 Z3) from one inversion
        fu inv01, inv23;
        {
          fu z0, z1, z2, z3, zz01, zz23, zz, inv;
          slot_load(reinterpret_cast<int32_t*>(z0.v), slot + 5, 10);
          slot_load(reinterpret_cast<int32_t*>(z1.v), slot + 8 + 5, 10);
          slot_load(reinterpret_cast<int32_t*>(z2.v), slot + 16 + 5, 10);
          slot_load(reinterpret_cast<int32_t*>(z3.v), slot + 24 + 5, 10);
          fu_mulc(zz01, z0, z1);
          fu_mulc(zz23, z2, z3);
          fu_mulc(zz, zz01, zz23);
          fu_invert(inv, zz);
          fu_mulc(inv01, inv, zz23);
          fu_mulc(inv23, inv, zz01);
        }
        goodm = 0;
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {
          const uint32_t rq = q == 0 ? rec[0] : q == 1 ? rec[1] : q == 2 ? rec[2] : rec[3];
          fu zp, zi;
          gu_p2 Q;
          slot_load(reinterpret_cast<int32_t*>(zp.v), slot + 8 * (q ^ 1) + 5, 10);  // the partner's Z
          slot_load(reinterpret_cast<int32_t*>(&Q), slot + 8 * q, 30);
          uint32_t Rw[8];
          load8(Rw, sig + (size_t)rq * 64);
          fu_mulc(zi, q < 2 ? inv01 : inv23, zp);
          goodm |= (((okm >> q) & 1) & gu_encode_eq_zi(Q, zi, Rw)) << q;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) good[q] = (goodm >> q) & 1;
#ifdef AT2V_COMB_PROBE
      probe.v[kCpFinish] += __builtin_amdgcn_s_memtime() - t_fin0;
#endif
    } else
    {
      // one quarter at a time through ONE inlined copy of the ladder
#pragma unroll 1
      for (int q = 0; q < 4; ++q) {
        const uint32_t ii = clamp(i0 + 64 * q);  // (not kPart: the hit list never takes this branch)
        uint32_t Rw[8], Sw[8], Aw[8];
        load8(Rw, sig + (size_t)ii * 64);
        load8(Sw, sig + (size_t)ii * 64 + 32);
        load8(Aw, pk + (size_t)ii * 32);
        const uint32_t o0 = off[ii], len = off[ii + 1] - o0;
        const int gq = with_msg_reader(msg, msg_total, o0, len, [&](auto& mwd) {
          return verify_half_fu(Rw, Aw, Sw, len, mwd, kZip ? POLICY_ZIP215 : cofactorless(policy), ta, tr, tb0, tb1,
                                wmax);
        });
        good[0] = q == 0 ? gq : good[0];  // (selects, not a runtime index into a register array)
        good[1] = q == 1 ? gq : good[1];
        good[2] = q == 2 ? gq : good[2];
        good[3] = q == 3 ? gq : good[3];
      }
    }
#ifdef AT2V_COMB_PROBE
    const unsigned long long t_book0 = __builtin_amdgcn_s_memtime();
#endif
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if constexpr (kPart) {  // records in list order
        verdict_or(verdicts, rec[q], good[q], i0 + 64 * q < lim, lane);
      } else {
        const uint64_t m = __ballot(good[q] & (i0 + 64 * q < n));
        if (lane == 0) {
          const uint32_t w0 = 8 * c + 2 * q;
          if (w0 < nwords) verdicts[w0] = (uint32_t)m;
          if (w0 + 1 < nwords) verdicts[w0 + 1] = (uint32_t)(m >> 32);
        }
      }
    }
    uint32_t ticket = 0;
    if (lane == 0) ticket = atomicAdd(chunk_queue, 1u);
    ticket = __builtin_amdgcn_readfirstlane(ticket);
    c = ticket < nchunks ? nwaves + ticket : nchunks;
#ifdef AT2V_COMB_PROBE
    if constexpr (kPart) {
      const unsigned long long t_end = __builtin_amdgcn_s_memtime();
      probe.v[kCpBook] += t_end - t_book0;
      probe.v[kCpChunk] += t_end - t_chunk0;
      probe.v[kCpChunks] += 1;
      probe.v[kCpBWait] += tbc.waited;
      probe.v[kCpStage] += tbc.stage_waited;
      tbc.waited = tbc.stage_waited = 0;
    }
#endif
  }
#ifdef AT2V_COMB_PROBE
  if constexpr (kPart) {  // one vector atomic per counter and wave, from lane 0
    if (lane == 0)
#pragma unroll
      for (int k = 0; k < kCpN; ++k) atomicAdd(&at2v_cprobe_acc[k], probe.v[k]);
  }
#endif
#undef AT2V_CP_ARG
}

// the same with per-key combs (at2v_opts.sender_comb): all-hit waves verify by additions only
__global__ __launch_bounds__(kBlock, kVerifyWavesPerSimd) void verify_kernel_comb(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab, uint32_t* __restrict__ chunk_queue, CacheArgs c) {
  __shared__ int4 astage[kWavesPerBlock * 10 * 64];
  __shared__ int4 rstage[kWavesPerBlock * 10 * 64];
  verify_chunks_comb4<false, false>(astage, rstage, pk, sig, msg, msg_total, off, n, policy, verdicts, scratch, btab,
                                    chunk_queue, c);
}
__global__ __launch_bounds__(kBlock, kVerifyWavesPerSimd) void verify_kernel_comb_zip215(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab, uint32_t* __restrict__ chunk_queue, CacheArgs c) {
  __shared__ int4 astage[kWavesPerBlock * 10 * 64];
  __shared__ int4 rstage[kWavesPerBlock * 10 * 64];
  verify_chunks_comb4<false, true>(astage, rstage, pk, sig, msg, msg_total, off, n, policy, verdicts, scratch, btab,
                                   chunk_queue, c);
}

// The classify kernel's hit list by comb additions, kRecs records per lane (chunks of 64 kRecs list positions): each
// record's R' = [k](-A) + [s]B is parked in the lane's slot (X, Y, Z at granules 8q..8q+7), then ONE inversion serves
// all kRecs Z's (Montgomery's trick as a product tree: pair products zp, for 8 records quad products, the inverse of the
// product, back down to 1 / (Z_2k Z_2k+1) at granules 8 kRecs + 3k), and each record is encoded with
// 1 / Z_q = Z_{q^1} / (Z_q Z_{q^1}). Per record: 254/kRecs squarings of the inversion, (3 kRecs - 3)/kRecs + 2
// products. Verdict bits go to the record's place in the bitmap (verdict_or).
template <int kRecs, int kBW>
__device__ AT2V_INLINE void verify_comb_hits(int4* astage, int4* rstage, const uint8_t* __restrict__ pk,
                                             const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
                                             uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n,
                                             int policy, uint32_t* __restrict__ verdicts, int4* __restrict__ scratch,
                                             uint32_t* __restrict__ chunk_queue, const CacheArgs& cc,
                                             const PartArgs& pp, uint32_t nh) {
  static_assert(kRecs == 4 || kRecs == 8, "records per lane");
  static_assert(8 * kRecs + 3 * (kRecs / 2) <= kLaneGranules, "the slot holds the parked points and pair inverses");
  const int lane = threadIdx.x & 63;
  const int wib = AT2V_UNIFORM(threadIdx.x >> 6);
  const uint32_t wave = blockIdx.x * kWavesPerBlock + wib;
  const uint32_t nwaves = gridDim.x * kWavesPerBlock;
  constexpr uint32_t kChunk = 64 * kRecs;
  const uint32_t nchunks = (nh + kChunk - 1) / kChunk;
  const int4* __restrict__ comb = cc.payload;
  int4* slot = scratch + ((size_t)wave * 64 + lane) * kLaneGranules;
  int4* const pinv = slot + 8 * kRecs;  // 1 / (Z_2k Z_2k+1), 3 granules each
  int4* const sa = astage + wib * 640;
  int4* const sr = rstage + wib * 640;
  // the context's wide comb of B (AT2V_CTX_BCOMB_WIDE, 24-bit windows: five additions fewer) or the 16-bit one
  const DevBCombW<kBW> tbc{kBW == kBCombLatBits ? cc.bcomb_lat : cc.bcomb, {sa, sr}, lane};
  constexpr uint32_t kHalf = kWavesPerBlock / 2;
  const uint32_t c_first = wib < (int)kHalf ? blockIdx.x * kHalf + wib
                                            : gridDim.x * kHalf + blockIdx.x * kHalf + (wib - kHalf);
  auto zload = [&](fu& z, int q) { slot_load(reinterpret_cast<int32_t*>(z.v), slot + 8 * q + 5, 10); };
#ifdef AT2V_COMB_PROBE
  CombProbe probe;
  CombProbe* const pr = &probe;
#endif
  for (uint32_t c = c_first; c < nchunks;) {
#ifdef AT2V_COMB_PROBE
    const unsigned long long t_chunk0 = __builtin_amdgcn_s_memtime();
#endif
    const uint32_t i0 = c * kChunk + lane;
    // the chunk's list entries, then their records' offsets: two memory latencies per chunk, not per record
    uint32_t lrec[kRecs], linfo[kRecs], lo0[kRecs], llen[kRecs];
#pragma unroll
    for (int q = 0; q < kRecs; ++q) {
      const uint32_t pos = i0 + 64 * q, pc = pos < nh ? pos : nh - 1;
      lrec[q] = pp.hidx[pc];
      linfo[q] = pp.hinfo[pc];
    }
#pragma unroll
    for (int q = 0; q < kRecs; ++q) {
      lo0[q] = off[lrec[q]];
      llen[q] = off[lrec[q] + 1] - lo0[q];
    }
    int okm = 0;
#pragma unroll 1
    for (int q = 0; q < kRecs; ++q) {
      uint32_t rq = lrec[0], info = linfo[0], o0 = lo0[0], len = llen[0];
#pragma unroll
      for (int k = 1; k < kRecs; ++k)
        if (q == k) {  // (selects: a runtime index into a register array would go to scratch)
          rq = lrec[k];
          info = linfo[k];
          o0 = lo0[k];
          len = llen[k];
        }
      gu_p3 P;
      int okq = -1;
      okq = comb2_point_staged(P, rq, o0, len, pk, sig, msg, msg_total, policy, (int)(info & 1u),
                               comb + (size_t)(info >> 1) * (kCombBytes / 16), tbc, sa, sr, lane
#ifdef AT2V_COMB_PROBE
                               , pr
#endif
      );
      if (okq < 0)
        okq = comb2_point(P, rq, n, pk, sig, msg, msg_total, off, policy, (int)(info & 1u),
                          comb + (size_t)(info >> 1) * (kCombBytes / 16), tbc, sa, sr, lane
#ifdef AT2V_COMB_PROBE
                          , pr
#endif
        );
      okm |= okq << q;
      slot_store(slot + 8 * q, reinterpret_cast<const int32_t*>(&P), 30);  // X, Y, Z (T not needed)
    }
#ifdef AT2V_COMB_PROBE
    const unsigned long long t_fin0 = __builtin_amdgcn_s_memtime();
#endif
    if (policy == POLICY_ZIP215) {  // (wave-uniform) comb2_point's verdicts are final: nothing encoded or inverted
#pragma unroll 1
      for (int q = 0; q < kRecs; ++q) {
        const uint32_t pos = i0 + 64 * q, pc = pos < nh ? pos : nh - 1;
        verdict_or(verdicts, pp.hidx[pc], (okm >> q) & 1, pos < nh, lane);
      }
    } else {
      {
        fu z0, z1, zp0, zp1, inv;
        zload(z0, 0);
        zload(z1, 1);
#ifdef AT2V_COMB_PROBE
        AT2V_CPROBE(probe.v[kCpSlot], asm volatile("s_waitcnt vmcnt(0)" ::: "memory"));
#endif
        fu_mulc(zp0, z0, z1);
        zload(z0, 2);
        zload(z1, 3);
#ifdef AT2V_COMB_PROBE
        AT2V_CPROBE(probe.v[kCpSlot], asm volatile("s_waitcnt vmcnt(0)" ::: "memory"));
#endif
        fu_mulc(zp1, z0, z1);
        if constexpr (kRecs == 4) {
          fu_mulc(z0, zp0, zp1);
          fu_invert(inv, z0);
          fu_mulc(z0, inv, zp1);  // 1 / (Z0 Z1)
          slot_store(pinv, reinterpret_cast<const int32_t*>(z0.v), 10);
          fu_mulc(z0, inv, zp0);  // 1 / (Z2 Z3)
          slot_store(pinv + 3, reinterpret_cast<const int32_t*>(z0.v), 10);
        } else {
          fu zp2, zp3, zq0, zq1;
          zload(z0, 4);
          zload(z1, 5);
          fu_mulc(zp2, z0, z1);
          zload(z0, 6);
          zload(z1, 7);
          fu_mulc(zp3, z0, z1);
          fu_mulc(zq0, zp0, zp1);
          fu_mulc(zq1, zp2, zp3);
          fu_mulc(z0, zq0, zq1);
          fu_invert(inv, z0);
          fu_mulc(z0, inv, zq1);  // 1 / (Z0 Z1 Z2 Z3)
          fu_mulc(z1, z0, zp1);   // 1 / (Z0 Z1)
          slot_store(pinv, reinterpret_cast<const int32_t*>(z1.v), 10);
          fu_mulc(z1, z0, zp0);   // 1 / (Z2 Z3)
          slot_store(pinv + 3, reinterpret_cast<const int32_t*>(z1.v), 10);
          fu_mulc(z0, inv, zq0);  // 1 / (Z4 Z5 Z6 Z7)
          fu_mulc(z1, z0, zp3);   // 1 / (Z4 Z5)
          slot_store(pinv + 6, reinterpret_cast<const int32_t*>(z1.v), 10);
          fu_mulc(z1, z0, zp2);   // 1 / (Z6 Z7)
          slot_store(pinv + 9, reinterpret_cast<const int32_t*>(z1.v), 10);
        }
      }
#pragma unroll 1
      for (int q = 0; q < kRecs; ++q) {
        const uint32_t pos = i0 + 64 * q, pc = pos < nh ? pos : nh - 1;
        const uint32_t rq = pp.hidx[pc];
        fu zp, ip, zi;
        gu_p2 Q;
        zload(zp, q ^ 1);  // the partner's Z
        slot_load(reinterpret_cast<int32_t*>(ip.v), pinv + 3 * (q >> 1), 10);
        slot_load(reinterpret_cast<int32_t*>(&Q), slot + 8 * q, 30);
        uint32_t Rw[8];
        load8(Rw, sig + (size_t)rq * 64);
#ifdef AT2V_COMB_PROBE
        AT2V_CPROBE(probe.v[kCpSlot], asm volatile("s_waitcnt vmcnt(0)" ::: "memory"));
#endif
        fu_mulc(zi, ip, zp);
        const int good = ((okm >> q) & 1) & gu_encode_eq_zi(Q, zi, Rw);
        verdict_or(verdicts, rq, good, pos < nh, lane);
      }
    }
#ifdef AT2V_COMB_PROBE
    const unsigned long long t_book0 = __builtin_amdgcn_s_memtime();
    probe.v[kCpFinish] += t_book0 - t_fin0;
#endif
    uint32_t ticket = 0;
    if (lane == 0) ticket = atomicAdd(chunk_queue, 1u);
    ticket = __builtin_amdgcn_readfirstlane(ticket);
    c = ticket < nchunks ? nwaves + ticket : nchunks;
#ifdef AT2V_COMB_PROBE
    const unsigned long long t_end = __builtin_amdgcn_s_memtime();
    probe.v[kCpBook] += t_end - t_book0;
    probe.v[kCpChunk] += t_end - t_chunk0;
    probe.v[kCpChunks] += 1;
    probe.v[kCpBWait] += tbc.waited;
    probe.v[kCpStage] += tbc.stage_waited;
    probe.v[kCpLds] += tbc.lds_waited;
    tbc.waited = tbc.stage_waited = tbc.lds_waited = 0;
#endif
  }
#ifdef AT2V_COMB_PROBE
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < kCpN; ++k) atomicAdd(&at2v_cprobe_acc[k], probe.v[k]);
#endif
}

// partitioned cached launches: the classify kernel's hit list by comb additions, four records per lane (eight per lane,
// one inversion for eight, measured 1.4% slower on 1M records from 64 senders: one 512-record chunk per wave leaves
// the chunk queue nothing to balance, profiles/r05n/abcomb.txt), [s]B from the context's 20-bit or 24-bit comb of B
__device__ AT2V_INLINE void verify_comb_part_chunks(
    int4* astage, int4* rstage, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig,
    const uint8_t* __restrict__ msg, uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy,
    uint32_t* __restrict__ verdicts, int4* __restrict__ scratch, uint32_t* __restrict__ chunk_queue, const CacheArgs& c,
    const PartArgs& p) {
  const uint32_t nh = __builtin_amdgcn_readfirstlane(p.counts[0]);
  if (c.bcomb_bits == kBCombBits)  // AT2V_CTX_BCOMB_WIDE
    verify_comb_hits<4, kBCombBits>(astage, rstage, pk, sig, msg, msg_total, off, n, policy, verdicts, scratch,
                                    chunk_queue, c, p, nh);
  else
    verify_comb_hits<4, kBCombMidBits>(astage, rstage, pk, sig, msg, msg_total, off, n, policy, verdicts, scratch,
                                       chunk_queue, c, p, nh);
}
__global__ __launch_bounds__(kBlock, kVerifyWavesPerSimd) void verify_kernel_comb_part(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab, uint32_t* __restrict__ chunk_queue, CacheArgs c,
    PartArgs p) {
  __shared__ int4 astage[kWavesPerBlock * 10 * 64];
  __shared__ int4 rstage[kWavesPerBlock * 10 * 64];
  (void)btab;
  verify_comb_part_chunks(astage, rstage, pk, sig, msg, msg_total, off, n, cofactorless(policy), verdicts, scratch,
                          chunk_queue, c, p);
}
__global__ __launch_bounds__(kBlock, kVerifyWavesPerSimd) void verify_kernel_comb_part_zip215(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msg,
    uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n, int policy, uint32_t* __restrict__ verdicts,
    int4* __restrict__ scratch, const int4* __restrict__ btab, uint32_t* __restrict__ chunk_queue, CacheArgs c,
    PartArgs p) {
  __shared__ int4 astage[kWavesPerBlock * 10 * 64];
  __shared__ int4 rstage[kWavesPerBlock * 10 * 64];
  (void)btab;
  verify_comb_part_chunks(astage, rstage, pk, sig, msg, msg_total, off, n, POLICY_ZIP215, verdicts, scratch,
                          chunk_queue, c, p);
}

}  // namespace at2v
