// at2v_kern_sign.h — the record generator, the signer and the point decode kernel.
// A piece of the kernels translation unit: at2v_kernels.hip includes the at2v_kern_*.h pieces in order (tables, cache,
// comb, sign, btab) and compiles them with its own kernels and launchers into one object. Each piece uses only the
// shared headers and the pieces before it.
#pragma once
#include <hip/hip_runtime.h>

#include "at2v_verify.h"
#include "at2v_kern_tables.h"

namespace at2v {

// ------------------------------------------------------------------ signing side

__device__ AT2V_INLINE void sc_muladd(uint32_t out[8], const uint32_t a[8], const uint32_t b[8], const uint32_t c[8]) {
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint64_t t = (uint64_t)a[i] * b[j] + x[i + j] + carry;
      x[i + j] = (uint32_t)t;
      carry = t >> 32;
    }
    x[i + 8] = (uint32_t)carry;
  }
  uint64_t carry = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint64_t t = (uint64_t)x[i] + (i < 8 ? c[i] : 0u) + carry;
    x[i] = (uint32_t)t;
    carry = t >> 32;
  }
  sc_reduce512(out, x);  // a, b, c < 2^253 so the sum < 2^507
}

// RFC 8032 sign of M under `seed` (8 LE words); writes pk (8 words) and R||S (16 words)
template <class TabB, class MsgWord>
__device__ AT2V_INLINE void sign_core(uint32_t pkw[8], uint32_t sigw[16], const uint32_t seed[8], uint32_t len,
                                      MsgWord msgword, const TabB& tb) {
  uint64_t h[8];
  uint32_t hw[16];
  sha512_prefixed<8>(h, seed, 0, [](uint32_t) { return 0u; });
  sha512_digest_words(hw, h);
  uint32_t a[8], prefix[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    a[i] = hw[i];
    prefix[i] = hw[8 + i];
  }
  a[0] &= 0xfffffff8u;
  a[7] = (a[7] & 0x7fffffffu) | 0x40000000u;
  uint32_t a16[16], ared[8];
#pragma unroll
  for (int i = 0; i < 16; ++i) a16[i] = i < 8 ? a[i] : 0u;
  sc_reduce512(ared, a16);
  ge_p2 P;
  ge_scalarmult_base(P, ared, tb);
  ge_p2_tobytes(pkw, P);
  // r = H(prefix || M) mod l ; R = [r]B
  sha512_prefixed<8>(h, prefix, len, msgword);
  sha512_digest_words(hw, h);
  uint32_t r[8];
  sc_reduce512(r, hw);
  ge_scalarmult_base(P, r, tb);
  ge_p2_tobytes(sigw, P);
  // k = H(R || A || M) mod l ; S = r + k a mod l
  uint32_t pre[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    pre[i] = sigw[i];
    pre[8 + i] = pkw[i];
  }
  sha512_prefixed<16>(h, pre, len, msgword);
  sha512_digest_words(hw, h);
  uint32_t k[8];
  sc_reduce512(k, hw);
  sc_muladd(sigw + 8, k, ared, r);
}

// SHA-512 of a short byte string held in registers as LE words (len <= 64)
template <int NW>
__device__ AT2V_INLINE void sha512_words(uint32_t out16[16], const uint32_t (&wds)[NW], uint32_t len) {
  uint64_t h[8];
  sha512_prefixed<0>(h, nullptr, len, [&](uint32_t j) {
    uint32_t v = 0;
#pragma unroll
    for (int m = 0; m < NW; ++m) v = (j == (uint32_t)m) ? wds[m] : v;
    return v;
  });
  sha512_digest_words(out16, h);
}

// seed_i and M_i of the deterministic generator (byte strings "at2v/seed"||u64le||u64le, 25 bytes, and
// "at2v/msg"||u64le cfg||u64le i||u64le ctr, 32 bytes)
__device__ AT2V_INLINE void gen_seed(uint32_t seed[8], uint64_t cfg, uint64_t idx) {
  // bytes: a t 2 v / s e e d | cfg(8) | idx(8)
  uint32_t w[7];
  w[0] = 0x76327461u;                                               // "at2v"
  w[1] = 0x6565732fu;                                               // "/see"
  w[2] = 0x64u | ((uint32_t)(cfg & 0xffffff) << 8);                 // "d" + cfg[0..2]
  w[3] = (uint32_t)(cfg >> 24);                                     // cfg[3..6]
  w[4] = (uint32_t)(cfg >> 56) | ((uint32_t)(idx & 0xffffff) << 8); // cfg[7] + idx[0..2]
  w[5] = (uint32_t)(idx >> 24);                                     // idx[3..6]
  w[6] = (uint32_t)(idx >> 56);                                     // idx[7]
  uint32_t o[16];
  sha512_words<7>(o, w, 25);
#pragma unroll
  for (int i = 0; i < 8; ++i) seed[i] = o[i];
}

__device__ AT2V_INLINE void gen_msg_block(uint32_t out16[16], uint64_t cfg, uint64_t idx, uint64_t ctr) {
  uint32_t w[8];
  w[0] = 0x76327461u;  // "at2v"
  w[1] = 0x67736d2fu;  // "/msg"
  w[2] = (uint32_t)cfg;
  w[3] = (uint32_t)(cfg >> 32);
  w[4] = (uint32_t)idx;
  w[5] = (uint32_t)(idx >> 32);
  w[6] = (uint32_t)ctr;
  w[7] = (uint32_t)(ctr >> 32);
  sha512_words<8>(out16, w, 32);
}

__global__ __launch_bounds__(kBlock) void gen_kernel(uint64_t cfg, uint64_t first, uint32_t n, uint32_t msg_len,
                                                     uint64_t senders, const uint64_t* __restrict__ keys,
                                                     uint8_t* __restrict__ pk,
                                                     uint8_t* __restrict__ sig, uint8_t* __restrict__ msg,
                                                     uint32_t* __restrict__ off) {
  __shared__ int4 btab[AT2V_BTAB_ENTRIES * 8];
  stage_btab(btab);
  LdsTabB tb{btab};
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t idx = first + i;
  uint32_t seed[8];
  // the key of seed index keys[i] (at2v_gen_records_keys_device), or of sender idx % senders; M_i stays per record
  gen_seed(seed, cfg, keys ? keys[i] : senders ? idx % senders : idx);
  // message bytes into the output buffer (byte stores; msg_len arbitrary)
  uint8_t* m = msg + (size_t)i * msg_len;
  for (uint32_t ctr = 0; ctr * 64 < msg_len; ++ctr) {
    uint32_t blk[16];
    gen_msg_block(blk, cfg, idx, ctr);
    for (uint32_t b = 0; b < 64 && ctr * 64 + b < msg_len; ++b) m[ctr * 64 + b] = (uint8_t)(blk[b >> 2] >> (8 * (b & 3)));
  }
  if (off) {
    off[i] = i * msg_len;
    if (i == n - 1) off[n] = n * msg_len;
  }
  const uint32_t mtotal = n * msg_len, o0 = i * msg_len;
  auto msgword = [&](uint32_t j) -> uint32_t {  // this lane's own bytes, written just above
    const uint32_t a = o0 + 4 * j;
    const uint32_t a0 = a & ~3u, sh = (a & 3u) * 8;
    const uint32_t lo = load_u32_guarded(msg, a0, mtotal);
    if (sh == 0) return lo;
    return __builtin_amdgcn_alignbit(load_u32_guarded(msg, a0 + 4, mtotal), lo, sh);
  };
  uint32_t pkw[8], sigw[16];
  sign_core(pkw, sigw, seed, msg_len, msgword, tb);
  uint32_t* pko = reinterpret_cast<uint32_t*>(pk + (size_t)i * 32);
  uint32_t* sgo = reinterpret_cast<uint32_t*>(sig + (size_t)i * 64);
#pragma unroll
  for (int q = 0; q < 8; ++q) pko[q] = pkw[q];
#pragma unroll
  for (int q = 0; q < 16; ++q) sgo[q] = sigw[q];
}

__global__ __launch_bounds__(kBlock) void sign_kernel(const uint8_t* __restrict__ seeds, const uint8_t* __restrict__ msg,
                                                      uint32_t msg_total, const uint32_t* __restrict__ off, uint32_t n,
                                                      uint8_t* __restrict__ pk, uint8_t* __restrict__ sig) {
  __shared__ int4 btab[AT2V_BTAB_ENTRIES * 8];
  stage_btab(btab);
  LdsTabB tb{btab};
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t seed[8];
  load8(seed, seeds + (size_t)i * 32);
  const uint32_t o0 = off[i];
  const uint32_t len = off[i + 1] - o0;
  auto msgword = [&](uint32_t j) -> uint32_t {
    const uint32_t a = o0 + 4 * j;
    const uint32_t a0 = a & ~3u, sh = (a & 3u) * 8;
    const uint32_t lo = load_u32_guarded(msg, a0, msg_total);
    if (sh == 0) return lo;
    return __builtin_amdgcn_alignbit(load_u32_guarded(msg, a0 + 4, msg_total), lo, sh);
  };
  uint32_t pkw[8], sigw[16];
  sign_core(pkw, sigw, seed, len, msgword, tb);
  uint32_t* pko = reinterpret_cast<uint32_t*>(pk + (size_t)i * 32);
  uint32_t* sgo = reinterpret_cast<uint32_t*>(sig + (size_t)i * 64);
#pragma unroll
  for (int q = 0; q < 8; ++q) pko[q] = pkw[q];
#pragma unroll
  for (int q = 0; q < 16; ++q) sgo[q] = sigw[q];
}

// dalek CompressedEdwardsY::decompress success bit per 32-byte point (at2v_decode_points): one lane per
// point, verdict words written per wave like the verify kernel
__global__ __launch_bounds__(kBlock) void decode_kernel(const uint8_t* __restrict__ pts, uint32_t n,
                                                        uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  int ok = 0;
  if (i < n) {
    uint32_t w[8];
    load8(w, pts + (size_t)i * 32);
    ge_p3 P;
    ok = ge_frombytes(P, w);
  }
  const uint64_t mask = __ballot(ok);
  const uint32_t first = i & ~63u, nwords = (n + 31) / 32;
  if ((threadIdx.x & 63) == 0 && first < n) {
    out[first / 32] = (uint32_t)mask;
    if (first / 32 + 1 < nwords) out[first / 32 + 1] = (uint32_t)(mask >> 32);
  }
}

}  // namespace at2v
