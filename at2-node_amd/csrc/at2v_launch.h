// at2v_launch.h — every host-side entry point of the kernels object (at2v_kernels.hip), declared once: the object
// defines them, the context (at2v_api.hip) calls them, and both include this header, so the compiler checks one against
// the other.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "at2v_cache.h"

namespace at2v {

// ---- verify
// One batch on `stream`: n <= pair_max takes a low-latency kernel, larger launches the persistent grid of `grid` blocks
// (scratch: scratch_bytes(grid); btab: btab_bytes(), built by launch_build_btab). cache: the per-sender A cache is on
// (part: the launch classifies its records first and verifies hits and misses apart); dense: fill every block.
hipError_t launch_verify(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint32_t msg_total,
                         const uint32_t* off, uint32_t n, int policy, uint32_t* verdicts, int4* scratch,
                         const int4* btab, int grid, uint32_t pair_max, hipStream_t stream,
                         const CacheArgs* cache, const PartArgs* part, int dense);
hipError_t verify_occupancy(int* blocks_per_cu, int* vgprs);
int block_threads();
size_t scratch_bytes_per_block();
size_t scratch_bytes(int grid);
size_t part_bytes_per_record();  // PartArgs lists
// the fixed-base tables [j]B and [j 2^128]B, then the shared identity entry; synchronises the stream
size_t btab_bytes();
hipError_t launch_build_btab(int4* out, hipStream_t stream);

// ---- generator, signer, decode
hipError_t launch_gen(uint64_t cfg, uint64_t first, uint32_t n, uint32_t msg_len, uint64_t senders,
                      const uint64_t* keys, uint8_t* pk, uint8_t* sig, uint8_t* msg, uint32_t* off, hipStream_t stream);
hipError_t launch_sign(const uint8_t* seeds, const uint8_t* msg, uint32_t msg_total, const uint32_t* off, uint32_t n,
                       uint8_t* pk, uint8_t* sig, hipStream_t stream);
hipError_t launch_decode(const uint8_t* pts, uint32_t n, uint32_t* out, hipStream_t stream);

// ---- transfers (at2v_kern_transfer.h): the messages and offsets of n transfers from their fields, for the verify launch
// that follows on `stream`. msg: 16-byte aligned, n * L bytes (L = 48 or 40 by wire, n * L < 2^32); off: n + 1 words;
// recipient_ok: ceil(n / 32) words (bit i: recipient i decodes), or nullptr
hipError_t launch_transfer_prep(const uint8_t* recipient, const uint64_t* amount, uint32_t n, int wire, uint8_t* msg,
                                uint32_t* off, uint32_t* recipient_ok, hipStream_t stream);

// ---- combs of B
size_t bcomb_bytes(int bits);  // a comb of B with bits-bit windows (16, 20 or 24)
int bcomb_lat_bits();
int bcomb_mid_bits();
int bcomb_wide_bits();
// build a comb of B into out (bcomb_bytes(bits)), asynchronously on stream; scratch: bcomb_scratch_bytes() of device
// memory the launches use until they complete
size_t bcomb_scratch_bytes();
hipError_t launch_build_bcomb(int4* out, int bits, void* scratch, hipStream_t stream);

// ---- per-sender A cache
size_t cache_entry_bytes();
size_t cache_payload_bytes(int comb);  // one key's payload: table [j]A or comb
int cache_ctl_words();
// initialise a fresh cache: free list 0..capacity-1 (stream order)
hipError_t launch_cache_init(const CacheArgs& c, hipStream_t stream);
// build stream, after the launch that filled claim slot c (c.new_list, count word c.count_word): build the payloads it
// claimed, mark them valid, reset the slot's count
hipError_t launch_cache_build(const CacheArgs& c, uint32_t max_claims, hipStream_t stream);
// compact a full cache into (x.new_tags, x.new_entries) (stream order; no cached launch or build may be in flight)
hipError_t launch_cache_compact(const CacheArgs& c, const CacheCompactArgs& x, hipStream_t stream);
// Known senders (at2v_sender_preload / _unpin / _query; stream order, no cached launch in flight). Preload: claim the
// listed keys into claim slot c (admission bypassed: the caller sets c.admit_first), then give their entries c.epoch and
// apply pin_op (CachePinOp); launch_cache_build follows. Pin: the second step alone. Query: l.status per key, reads only.
hipError_t launch_cache_preload(const CacheArgs& c, const CacheKeyList& l, int pin_op, hipStream_t stream);
hipError_t launch_cache_pin(const CacheArgs& c, const CacheKeyList& l, int pin_op, hipStream_t stream);
hipError_t launch_cache_query(const CacheArgs& c, const CacheKeyList& l, hipStream_t stream);

}  // namespace at2v
