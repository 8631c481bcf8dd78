// at2v_reason.hip — the reject-reasons pass on the device (include/at2v.h at2v_reject_reasons_device): for every record
// whose verdict bit is 0, which check failed (at2v_reason.h reject_reason); and, at the end of the file, the policy-mask
// pass (at2v_policy_mask_device): for every record, which policies accept it. Its own translation unit and code object:
// nothing here is seen by the verify kernels (at2v_kernels.hip), whose object does not depend on this file.
//
// Rejected records are usually few (10 % in the adversarial mix) but spread, so that almost every wave of 64 holds one:
// one lane per record would run the two square-root chains in nearly every wave for a handful of active lanes. So a
// block compacts first:
//   * a block owns a tile of kReasonTile consecutive records (64 verdict words);
//   * it reads the tile's verdict bits (indices >= n masked: pad bits are 0 and are not rejects) and appends the
//     rejected records' tile indices to a list in LDS: ballot + popcount per wave, one LDS counter per block;
//   * after a barrier it walks the list densely (k = tid; k < count; k += blockDim), one reject_reason per entry;
//   * the tile's reason bytes are assembled in LDS (0 for valid records) and written out once, 16 bytes per lane; the
//     last tile's tail goes out byte by byte. No global byte is stored twice, none at or after reasons + n.
#include <hip/hip_runtime.h>

#include "at2v_reason.h"
#include "at2v_reason_launch.h"

namespace at2v {

constexpr int kReasonBlock = 256;
constexpr uint32_t kReasonTile = 2048;  // records per block: 64 verdict words, 2 KB of reason bytes
static_assert(kReasonTile % kReasonBlock == 0 && kReasonTile % 64 == 0, "whole waves of whole verdict words");

__device__ AT2V_INLINE void reason_load8(uint32_t w[8], const uint8_t* p) {  // 32 bytes, 16-byte aligned
  const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
  w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
  w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
}

__global__ __launch_bounds__(kReasonBlock) void reject_reason_kernel(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, uint32_t n,
    const uint32_t* __restrict__ verdict_words, uint8_t* __restrict__ reasons, int policy) {
  __shared__ uint16_t list[kReasonTile];      // tile indices of the rejected records, in no particular order
  __shared__ uint4 bytes16[kReasonTile / 16];  // the tile's reason bytes
  __shared__ uint32_t count;
  uint8_t* const bytes = reinterpret_cast<uint8_t*>(bytes16);
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t tile0 = blockIdx.x * kReasonTile;  // < n < 2^31
  if (tid == 0) count = 0;
  for (uint32_t k = tid; k < kReasonTile / 16; k += kReasonBlock) bytes16[k] = make_uint4(0, 0, 0, 0);
  __syncthreads();
#pragma unroll 1
  for (uint32_t r = tid; r < kReasonTile; r += kReasonBlock) {  // every wave: 64 consecutive records, two words
    const uint32_t i = tile0 + r;
    int rej = 0;
    if (i < n) rej = !((verdict_words[i >> 5] >> (i & 31)) & 1u);
    const uint64_t mask = __ballot(rej);
    uint32_t base = 0;
    if (lane == 0 && mask) base = atomicAdd(&count, (uint32_t)__popcll(mask));
    base = __shfl(base, 0);
    if (rej) list[base + __popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)r;
  }
  __syncthreads();
  const uint32_t c = count;  // <= the tile's records
#pragma unroll 1
  for (uint32_t k = tid; k < c; k += kReasonBlock) {
    const uint32_t r = list[k];
    const size_t i = (size_t)tile0 + r;
    uint32_t Aw[8], Rw[8], Sw[8];
    reason_load8(Aw, pk + i * 32);
    reason_load8(Rw, sig + i * 64);
    reason_load8(Sw, sig + i * 64 + 32);
    bytes[r] = (uint8_t)reject_reason(Aw, Rw, Sw, policy);
  }
  __syncthreads();
  const uint32_t m = n - tile0 < kReasonTile ? n - tile0 : kReasonTile;  // the tile's records
  uint8_t* const out = reasons + tile0;                                 // 16-byte aligned: the tile is 2 KB
  for (uint32_t k = tid; k < m / 16; k += kReasonBlock) reinterpret_cast<uint4*>(out)[k] = bytes16[k];
  for (uint32_t b = (m & ~15u) + tid; b < m; b += kReasonBlock) out[b] = bytes[b];
}

hipError_t launch_reject_reasons(const uint8_t* pk, const uint8_t* sig, uint32_t n, const uint32_t* verdict_words,
                                 uint8_t* reasons, int policy, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(reject_reason_kernel, dim3((n + kReasonTile - 1) / kReasonTile), dim3(kReasonBlock), 0, stream,
                     pk, sig, n, verdict_words, reasons, policy);
  return hipGetLastError();
}

// The policy-mask pass (include/at2v.h at2v_policy_mask_device; at2v_reason.h policy_mask): one lane per record, no
// decode and no field arithmetic, so nothing to compact. A block owns kMaskBlock consecutive records and their bytes,
// assembles them in LDS (0 for a rejected record, whose 96 bytes are not read) and writes them once, 16 bytes per lane;
// the last block's tail goes out byte by byte. No global byte is stored twice, none at or after mask + n.
constexpr int kMaskBlock = 256;
static_assert(kMaskBlock % 64 == 0, "whole waves of whole verdict words; every block's bytes start 16-byte aligned");

__global__ __launch_bounds__(kMaskBlock) void policy_mask_kernel(
    const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, uint32_t n,
    const uint32_t* __restrict__ verdict_words, uint8_t* __restrict__ mask) {
  __shared__ uint4 bytes16[kMaskBlock / 16];
  uint8_t* const bytes = reinterpret_cast<uint8_t*>(bytes16);
  const uint32_t tid = threadIdx.x;
  const uint32_t tile0 = blockIdx.x * kMaskBlock;  // < n < 2^31
  const uint32_t i = tile0 + tid;
  uint8_t b = 0;
  if (i < n && ((verdict_words[i >> 5] >> (i & 31)) & 1u)) {
    uint32_t Aw[8], Rw[8], Sw[8];
    reason_load8(Aw, pk + (size_t)i * 32);
    reason_load8(Rw, sig + (size_t)i * 64);
    reason_load8(Sw, sig + (size_t)i * 64 + 32);
    b = (uint8_t)policy_mask(Aw, Rw, Sw, 1);
  }
  bytes[tid] = b;
  __syncthreads();
  const uint32_t m = n - tile0 < kMaskBlock ? n - tile0 : kMaskBlock;  // the block's records
  uint8_t* const out = mask + tile0;
  if (tid < m / 16) reinterpret_cast<uint4*>(out)[tid] = bytes16[tid];
  const uint32_t t = (m & ~15u) + tid;
  if (t < m) out[t] = bytes[t];
}

hipError_t launch_policy_mask(const uint8_t* pk, const uint8_t* sig, uint32_t n, const uint32_t* verdict_words,
                              uint8_t* mask, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(policy_mask_kernel, dim3((n + kMaskBlock - 1) / kMaskBlock), dim3(kMaskBlock), 0, stream, pk, sig,
                     n, verdict_words, mask);
  return hipGetLastError();
}

}  // namespace at2v
