// at2v_stage_plan.h — the arithmetic of the host-buffer pipeline (at2v_api_pipe.h): how a shard's part of a batch is cut
// into chunks, how a chunk is laid out in its staging slot and on the device, how many bytes of device arena a part
// takes, and how a chunk's host copy is cut into pieces for the copy pool. No HIP, HSA or RCCL: plain C++, so
// tests/host/stage_plan_host.cpp checks it under the sanitizers without a GPU. issue_chunk relies on the inequality
// between ChunkPlan, chunk_layout and arena_bytes that the test asserts.
#ifndef AT2V_STAGE_PLAN_H  // (a guard, not #pragma once: the header also compiles alone as a main file)
#define AT2V_STAGE_PLAN_H
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace at2v {

constexpr int kStageSlots = 3;
constexpr size_t kStageMaxRecords = 131072;   // 2,048 wave chunks: one per resident wave of the persistent grid
constexpr size_t kStageFirstRecords = 65536;  // 1,024 wave chunks: half the device in dense blocks
constexpr size_t kCopyPiece = 1 << 20;        // bytes per copy-pool job item
constexpr size_t kCopyPoolMin = 2 << 20;      // chunks below this many bytes are copied by the calling thread alone
constexpr size_t kCopyBatch = 8;              // copy pieces between two polls of the pending chunk's uploads

// A staged chunk of c records with mb message bytes: pk | sig | offsets (c + 1, rebased) | messages (+16 bytes of slack
// for the kernels' last-word reads), every part 16-byte aligned.
struct ChunkLayout {
  size_t sig, off, msg, upload, total;
};
inline ChunkLayout chunk_layout(size_t c, size_t mb) {
  ChunkLayout l;
  l.sig = c * 32;
  l.off = c * 96;
  l.msg = (l.off + (c + 1) * 4 + 15) & ~(size_t)15;
  l.upload = l.msg + mb;
  l.total = l.upload + 16;
  return l;
}

// device bytes a shard's part of a host batch takes in the pipe's arena: every chunk's layout, 256-aligned
inline size_t arena_bytes(size_t m, size_t mb, size_t first) {
  const size_t chunks = m / (first ? first : 1) + 2;
  return m * 100 + mb + chunks * (16 + 4 + 16 + 256) + 256;
}

// A chunk of c transfers (at2v_verify_transfers*; message length L = 48 or 40): pk | sig | recipient | amount, which are
// uploaded (c * 136 bytes in a row, the staging slot's layout too), then the offsets (c + 1) and the messages (c * L, + 16
// bytes of slack) that the prep kernel writes on the device. Every part 16-byte aligned.
struct TransferLayout {
  size_t sig, rcp, amt, upload, off, msg, total;
};
inline TransferLayout transfer_layout(size_t c, size_t L) {
  TransferLayout l;
  l.sig = c * 32;
  l.rcp = c * 96;
  l.amt = c * 128;
  l.upload = c * 136;
  l.off = (l.upload + 15) & ~(size_t)15;
  l.msg = (l.off + (c + 1) * 4 + 15) & ~(size_t)15;
  l.total = l.msg + c * L + 16;
  return l;
}

// device bytes a shard's part of a transfers call takes in the pipe's arena: every chunk's transfer_layout, 256-aligned
// (per chunk: up to 15 + 15 bytes of alignment, the extra offset, the slack, and up to 255 bytes to the next region)
inline size_t transfer_arena_bytes(size_t m, size_t L, size_t first) {
  const size_t chunks = m / (first ? first : 1) + 2;
  return m * (140 + L) + chunks * (15 + 15 + 4 + 16 + 256) + 256;
}

// The chunk schedule of one shard's part of a host batch: a part the low-latency kernel takes whole (<= pair_max, the
// context's small_batch_max, records) is one chunk; a larger one starts with stage_first (kStageFirstRecords: the
// pipeline's fill, nothing runs on the device until it is up), then doubles up to stage_max (kStageMaxRecords), and a
// remainder smaller than the first chunk joins the chunk before it. Those chunks run the throughput kernels with dense
// grids whatever their size (launch_shard `pipeline`). Every chunk but the last is a multiple of 64 records.
struct ChunkPlan {
  size_t first = 0, next = 0, pos = 0, m = 0, cap = 0;
  void init(size_t m_, size_t pair_max, size_t stage_first, size_t stage_max) {
    m = m_;
    pos = 0;
    first = m <= pair_max ? std::max<size_t>(m, 64) : stage_first;
    cap = std::max(stage_max, first);
    next = first;
  }
  bool done() const { return pos >= m; }
  size_t take() {  // the next chunk's record count (its first record is pos before the call)
    size_t c = std::min(next, m - pos);
    if (m - pos - c < first) c = m - pos;
    if (pos > 0 || first >= cap) next = std::min(next * 2, cap);  // (the first size twice: two launches fill the device)
    pos += c;
    return c;
  }
};

// The host copy of one chunk, split into pieces of about kCopyPiece bytes for the copy pool.
struct CopyPiece {
  uint8_t* dst;
  const uint8_t* src;  // bytes, or (offsets piece) the caller's msg_off + first record
  size_t len;          // bytes, or offsets
  uint32_t base;       // offsets piece: subtracted from every offset
  bool offsets;
};
struct CopyJob {
  std::vector<CopyPiece> pieces;
  void add(uint8_t* dst, const uint8_t* src, size_t len) {
    for (size_t o = 0; o < len; o += kCopyPiece)
      pieces.push_back({dst + o, src + o, std::min(kCopyPiece, len - o), 0, false});
  }
  void add_offsets(uint32_t* dst, const uint32_t* src, size_t count, uint32_t base) {
    const size_t step = kCopyPiece / 4;
    for (size_t o = 0; o < count; o += step)
      pieces.push_back({(uint8_t*)(dst + o), (const uint8_t*)(src + o), std::min(step, count - o), base, true});
  }
  size_t base = 0;  // run_copy: the first piece of the batch the pool is running
  static void run_piece(void* a, size_t i) {
    CopyJob* j = static_cast<CopyJob*>(a);
    const CopyPiece& p = j->pieces[j->base + i];
    if (!p.offsets) {
      std::memcpy(p.dst, p.src, p.len);
      return;
    }
    const uint32_t* s = (const uint32_t*)p.src;
    uint32_t* d = (uint32_t*)p.dst;
    for (size_t k = 0; k < p.len; ++k) d[k] = s[k] - p.base;
  }
};

}  // namespace at2v

#endif  // AT2V_STAGE_PLAN_H
