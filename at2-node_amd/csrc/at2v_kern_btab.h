// at2v_kern_btab.h — builders of the fixed-base tables and of the combs of B.
// A piece of the kernels translation unit: at2v_kernels.hip includes the at2v_kern_*.h pieces in order (tables, cache,
// comb, sign, btab) and compiles them with its own kernels and launchers into one object. Each piece uses only the
// shared headers and the pieces before it.
#pragma once
#include <hip/hip_runtime.h>

#include "at2v_verify.h"
#include "at2v_verify_fu.h"
#include "at2v_kern_tables.h"

namespace at2v {

// [j]B, j = 0..2^(kBWin-1), affine Niels, 32 words per entry (30 + 2 pad): built once per context
__global__ __launch_bounds__(kBlock) void build_btab_kernel(int4* __restrict__ out, int shift_words) {
  __shared__ int4 btab[AT2V_BTAB_ENTRIES * 8];
  stage_btab(btab);
  LdsTabB tb{btab};
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= (uint32_t)kBtabEntries) return;
  uint32_t sj[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < 8; ++q) sj[q] = q == shift_words ? j : 0u;  // j * 2^(32 shift_words)
  ge_p2 P;
  ge_scalarmult_base(P, sj, tb);
  ge_niels nj;
  ge_p2_to_niels(nj, P);
  int32_t w[32];
  {  // the verify kernel reads the tables on the unsigned field
    gu_niels nu;
    niels_fe_to_fu(nu, nj);
    for (int k = 0; k < 10; ++k) {
      nj.ypx.v[k] = (int32_t)nu.ypx.v[k];
      nj.ymx.v[k] = (int32_t)nu.ymx.v[k];
      nj.xy2d.v[k] = (int32_t)nu.xy2d.v[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    w[k] = nj.ypx.v[k];
    w[10 + k] = nj.ymx.v[k];
    w[20 + k] = nj.xy2d.v[k];
  }
  w[30] = w[31] = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) out[(size_t)j * 8 + q] = make_int4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}

// The combs of B, D[pos][j] = [j 2^(W pos)]B for j = 0..2^(W-1), affine Niels on the unsigned field, built by additions
// (round 6, VERDICT r5 "Next" 3). Round 5 computed every entry by its own fixed-base scalar multiplication (~2,500 field
// multiplications per entry; the 20-bit table took 13 launches of ~28 ms, up to 68 ms, 68% of a profiled bench's GPU
// time). Now:
//   bcomb_base_kernel  one lane per position: P_pos = [2^(W pos)]B (W pos doublings of B, decoded from its encoding)
//                      and D_pos = [K]P_pos, both in cached form;
//   bcomb_fill_kernel  one lane per (pos, h), h < 2^(W-1)/K: S = [K h + 1]P_pos = P_pos + [h]D_pos (binary method),
//                      then its K entries j = K h + 1 .. K h + K by consecutive additions of P_pos, made affine with one
//                      inversion per lane (Montgomery's trick through the entries' own 128-byte slots, as comb_build_lane:
//                      pass 1 stores (X pi', Y pi', Z), pass 2 writes (y+x, y-x, 2dxy)); lane h = 0 also writes j = 0.
// About 30 multiplications per entry; fill launches of at most kBCombFillLanes lanes, so no launch holds the device for
// long (a node that starts beside a serving one no longer stalls it). Any representation of the same point
// gives the same verdicts; the comb paths' parity tests run on these tables.
constexpr int kBCombKLog2 = 6;
constexpr int kBCombK = 1 << kBCombKLog2;       // entries per fill lane
constexpr uint32_t kBCombFillLanes = 1u << 16;  // lanes per fill launch

__global__ __launch_bounds__(64) void bcomb_base_kernel(gu_cached* __restrict__ base, int pos_bits, int npos) {
  const int p = threadIdx.x;
  if (p >= npos) return;
  const uint32_t Bw[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                          0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};  // the base point's encoding (y = 4/5)
  gu_p3 P;
  (void)gu_frombytes(P, Bw);
  gu_p2 Q2;
  gu_p1p1 t;
  const int nd = pos_bits * p;
#pragma unroll 1
  for (int d = 0; d < nd; ++d) {  // P = [2^(pos_bits p)]B
    gu_p3_to_p2(Q2, P);
    gu_p2_dbl(t, Q2);
    gu_p1p1_to_p3(P, t);
  }
  gu_cached c;
  gu_p3_to_cached(c, P);
  base[2 * p] = c;
#pragma unroll 1
  for (int d = 0; d < kBCombKLog2; ++d) {  // D = [K]P
    gu_p3_to_p2(Q2, P);
    gu_p2_dbl(t, Q2);
    gu_p1p1_to_p3(P, t);
  }
  gu_p3_to_cached(c, P);
  base[2 * p + 1] = c;
}

__device__ AT2V_INLINE void bcomb_put3(int4* dst, const fu& a, const fu& b, const fu& c) {
  uint32_t w[32];
#pragma unroll
  for (int q = 0; q < 10; ++q) {
    w[q] = a.v[q];
    w[10 + q] = b.v[q];
    w[20 + q] = c.v[q];
  }
  w[30] = w[31] = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) dst[q] = make_int4((int)w[4 * q], (int)w[4 * q + 1], (int)w[4 * q + 2], (int)w[4 * q + 3]);
}

__device__ AT2V_INLINE void bcomb_get3(const int4* src, fu& a, fu& b, fu& c) {
  uint32_t w[32];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int4 v = src[q];
    w[4 * q] = (uint32_t)v.x;
    w[4 * q + 1] = (uint32_t)v.y;
    w[4 * q + 2] = (uint32_t)v.z;
    w[4 * q + 3] = (uint32_t)v.w;
  }
#pragma unroll
  for (int q = 0; q < 10; ++q) {
    a.v[q] = w[q];
    b.v[q] = w[10 + q];
    c.v[q] = w[20 + q];
  }
}

// lanes [lane0, lane0 + grid) of the fill: lane L = pos * parts + h
__global__ __launch_bounds__(256) void bcomb_fill_kernel(int4* __restrict__ out, const gu_cached* __restrict__ base,
                                                          int bits, int npos, uint32_t lane0) {
  const uint32_t parts = (1u << (bits - 1)) >> kBCombKLog2;
  const uint32_t L = lane0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (L >= parts * (uint32_t)npos) return;
  const int pos = (int)(L / parts);
  const uint32_t h = L % parts;
  const size_t entries = ((size_t)1 << (bits - 1)) + 1;
  int4* tab = out + (size_t)pos * entries * 8;
  const gu_cached P = base[2 * pos], D = base[2 * pos + 1];
  gu_p1p1 t;
  // S = [h]D + P (binary method from the top bit of h; the complete formulas take the identity)
  gu_p3 S;
  gu_p3_identity(S);
  for (int b = 31 - __builtin_clz(h | 1); b >= 0 && h; --b) {
    gu_p2 S2;
    gu_p3_to_p2(S2, S);
    gu_p2_dbl(t, S2);
    gu_p1p1_to_p3(S, t);
    if ((h >> b) & 1u) {
      gu_add(t, S, D);
      gu_p1p1_to_p3(S, t);
    }
  }
  gu_add(t, S, P);
  gu_p1p1_to_p3(S, t);
  const uint32_t j0 = h * kBCombK + 1;
  if (h == 0) {
    fu one, zero;
    fu_1(one);
    fu_0(zero);
    bcomb_put3(tab, one, one, zero);  // j = 0, the identity: y+x = 1, y-x = 1, 2dxy = 0
  }
  fu pi;  // pass 1: pi = Z_0 ... Z_m; entry m holds (X_m pi_(m-1), Y_m pi_(m-1), Z_m)
#pragma unroll 1
  for (int m = 0; m < kBCombK; ++m) {
    int4* e = tab + (size_t)(j0 + m) * 8;
    if (m == 0) {
      bcomb_put3(e, S.X, S.Y, S.Z);
      pi = S.Z;
    } else {
      fu xp, yp;
      fu_mulc(xp, S.X, pi);
      fu_mulc(yp, S.Y, pi);
      bcomb_put3(e, xp, yp, S.Z);
      fu_mulc(pi, pi, S.Z);
    }
    if (m + 1 < kBCombK) {
      gu_add(t, S, P);
      gu_p1p1_to_p3(S, t);
    }
  }
  fu inv;  // 1 / pi_m, m from the last entry down
  fu_invert(inv, pi);
#pragma unroll 1
  for (int m = kBCombK - 1; m >= 0; --m) {
    int4* e = tab + (size_t)(j0 + m) * 8;
    fu xp, yp, z, x, y;
    bcomb_get3(e, xp, yp, z);
    fu_mulc(x, xp, inv);
    fu_mulc(y, yp, inv);
    fu_mulc(inv, inv, z);
    gu_niels n;
    fu_add(n.ypx, y, x);
    fu_carry(n.ypx);
    fu_sub(n.ymx, y, x, FU_KC);
    fu_carry(n.ymx);
    fu xy;
    fu_mulc(xy, x, y);
    fu_mulc(n.xy2d, xy, FU_D2);
    bcomb_put3(e, n.ypx, n.ymx, n.xy2d);
  }
}

}  // namespace at2v
