// at2v_kern_transfer.h — the prep pass of the transfers entry points (a piece of at2v_kernels.hip).
//
// at2v_verify_transfers* take the fields of SendAssetRequest (sender, signature, recipient, amount). The verify kernels
// read messages and offsets in the at2v_verify_batch layout, so this pass expands them on the device, right before the
// verify launch on the same stream: record i's message M_i (at2v_transfer.h) at byte i * L of `msg`, and the n + 1
// offsets i * L. One lane per record; the recipient is two 16-byte loads, the amount one 8-byte load. With
// AT2V_WIRE_BYTES L = 48 and a record's message is 16-byte aligned (three 16-byte stores); with AT2V_WIRE_ARRAY L = 40
// and it is only 8-byte aligned (five 8-byte stores). kDecode: each lane also decodes its recipient (gu_frombytes, the
// verify kernels' own routine: dalek's CompressedEdwardsY::decompress) and the wave's ballot goes out as two words from
// lane 0, as the verify kernels write their verdicts; tail lanes recompute the last record and are masked. No atomics,
// no scratch set, nothing that orders one verify launch against another.
#pragma once
#include "at2v_transfer.h"

namespace at2v {

constexpr int kPrepBlock = 256;

template <bool kDecode>
__global__ __launch_bounds__(kPrepBlock) void transfer_prep_kernel(
    const uint8_t* __restrict__ recipient, const uint64_t* __restrict__ amount, uint32_t n, int wire,
    uint8_t* __restrict__ msg, uint32_t* __restrict__ off, uint32_t* __restrict__ recipient_ok) {
  const uint32_t i = blockIdx.x * kPrepBlock + threadIdx.x;  // (n < 2^31: no wrap)
  const uint32_t ii = i < n ? i : n - 1;  // tail lanes recompute a real record; they store nothing and their bit is masked
  const bool act = i < n;
  uint32_t r[8], w[kTransferMaxWords];
  load8(r, recipient + (size_t)ii * 32);
  const uint64_t a = amount[ii];
  const uint32_t len = transfer_msg_words(w, r, a, wire);
  if (act) {
    uint8_t* m = msg + (size_t)i * len;
    if (wire == kTransferWireBytes) {  // 48-byte stride from a 16-byte-aligned base
      uint4* q = reinterpret_cast<uint4*>(m);
      q[0] = make_uint4(w[0], w[1], w[2], w[3]);
      q[1] = make_uint4(w[4], w[5], w[6], w[7]);
      q[2] = make_uint4(w[8], w[9], w[10], w[11]);
    } else {  // 40-byte stride: 8-byte aligned only
      uint2* q = reinterpret_cast<uint2*>(m);
#pragma unroll
      for (int k = 0; k < 5; ++k) q[k] = make_uint2(w[2 * k], w[2 * k + 1]);
    }
    off[i] = i * len;  // (n * len < 2^32: checked by the launcher)
    if (i == n - 1) off[n] = n * len;
  }
  if constexpr (kDecode) {
    gu_p3 P;
    const int ok = gu_frombytes(P, r) & (act ? 1 : 0);
    const uint64_t mask = __ballot(ok);
    const uint32_t first = i & ~63u, nwords = (n + 31) / 32;
    if ((threadIdx.x & 63) == 0 && first < n) {
      recipient_ok[first / 32] = (uint32_t)mask;
      if (first / 32 + 1 < nwords) recipient_ok[first / 32 + 1] = (uint32_t)(mask >> 32);
    }
  }
}

// msg: 16-byte aligned, n * L bytes (+ the kernels' 16 bytes of slack, not written); off: n + 1 words; recipient_ok:
// ceil(n / 32) words, or nullptr (no decode). The caller has checked wire, n < 2^31 and n * L < 2^32.
hipError_t launch_transfer_prep(const uint8_t* recipient, const uint64_t* amount, uint32_t n, int wire, uint8_t* msg,
                                uint32_t* off, uint32_t* recipient_ok, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t len = transfer_msg_len(wire);
  if (len == 0 || (uint64_t)n * len >= (1ull << 32)) return hipErrorInvalidValue;
  const dim3 grid((n + kPrepBlock - 1) / kPrepBlock), block(kPrepBlock);
  if (recipient_ok)
    hipLaunchKernelGGL(transfer_prep_kernel<true>, grid, block, 0, stream, recipient, amount, n, wire, msg, off,
                       recipient_ok);
  else
    hipLaunchKernelGGL(transfer_prep_kernel<false>, grid, block, 0, stream, recipient, amount, n, wire, msg, off,
                       recipient_ok);
  return hipGetLastError();
}

}  // namespace at2v
