// at2v_transfer.h — the one definition of the signed message of an AT2 transfer from its fields.
//
// Every SendAssetRequest is signed over M = bincode(ThinTransaction{recipient, amount}) (the reference's src/lib.rs:14-22,
// signed at src/client.rs:77-78). With drop's PublicKey serialised as serde bytes (AT2V_WIRE_BYTES) that is
//   u64le(32) || recipient (32 bytes) || u64le(amount)      48 bytes
// and as a fixed array (AT2V_WIRE_ARRAY)
//   recipient (32 bytes) || u64le(amount)                   40 bytes.
// The transfers entry points (at2v_verify_transfers*, at2v_queue_submit_transfers) take the fields and build M here: the
// device kernel (at2v_kern_transfer.h) from the words, the CPU backend and the ingest queue from the bytes.
// at2v_pack.h's thin_transaction is the packer's own copy and stays as it is; tests/host/transfer_plan_host.cpp checks
// this one against literal bytes. No HIP: plain C++ that also compiles for the device.
#ifndef AT2V_TRANSFER_H  // (a guard, not #pragma once: the header also compiles alone as a main file)
#define AT2V_TRANSFER_H
#include <cstddef>
#include <cstdint>

#ifndef AT2V_HD
#if defined(__HIPCC__)
#define AT2V_HD __host__ __device__
#define AT2V_INLINE __forceinline__
#else
#define AT2V_HD
#define AT2V_INLINE inline __attribute__((always_inline))
#endif
#endif

namespace at2v {

constexpr int kTransferWireBytes = 0;  // include/at2v.h AT2V_WIRE_BYTES
constexpr int kTransferWireArray = 1;  // include/at2v.h AT2V_WIRE_ARRAY
constexpr uint32_t kTransferMaxWords = 12;
constexpr size_t kTransferFieldBytes = 32 + 64 + 32 + 8;  // what a record uploads: sender, signature, recipient, amount

// bytes of M; 0 for a wire that is neither
AT2V_HD AT2V_INLINE uint32_t transfer_msg_len(int wire) {
  return wire == kTransferWireBytes ? 48u : wire == kTransferWireArray ? 40u : 0u;
}

// M as little-endian 32-bit words from the recipient's eight words and the amount: w[0 .. len / 4); returns len
AT2V_HD AT2V_INLINE uint32_t transfer_msg_words(uint32_t w[kTransferMaxWords], const uint32_t recipient[8],
                                                uint64_t amount, int wire) {
  uint32_t o = 0;
  if (wire == kTransferWireBytes) {
    w[0] = 32u;
    w[1] = 0u;
    o = 2;
  }
  for (int k = 0; k < 8; ++k) w[o + k] = recipient[k];
  w[o + 8] = (uint32_t)amount;
  w[o + 9] = (uint32_t)(amount >> 32);
  return (o + 10) * 4;
}

// M as bytes (out: transfer_msg_len(wire) of them, any alignment); returns the length
AT2V_HD AT2V_INLINE uint32_t transfer_msg_bytes(uint8_t* out, const uint8_t recipient[32], uint64_t amount, int wire) {
  uint32_t o = 0;
  if (wire == kTransferWireBytes) {
    out[0] = 32;
    for (int k = 1; k < 8; ++k) out[k] = 0;
    o = 8;
  }
  for (int k = 0; k < 32; ++k) out[o + k] = recipient[k];
  for (int k = 0; k < 8; ++k) out[o + 32 + k] = (uint8_t)(amount >> (8 * k));
  return o + 40;
}

}  // namespace at2v

#endif  // AT2V_TRANSFER_H
