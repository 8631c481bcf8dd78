// at2v_stage_plan.h — the arithmetic of the host-buffer pipeline (at2v_api_pipe.h): how a shard's part of a batch is cut
// into chunks, how a chunk is laid out in its staging slot and on the device, which uploads carry it there, how many bytes
// of device arena a part takes, and how a chunk's host copy is cut into pieces for the copy pool. No HIP, HSA or RCCL:
// plain C++, so tests/host/stage_plan_host.cpp checks it under the sanitizers without a GPU. issue_chunk relies on the
// inequality between ChunkPlan, chunk_layout and arena_bytes that the test asserts, and on upload_plan / walk_uploads
// keeping the slot's signal equal to the uploads in flight.
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

// A chunk of c records in its staging slot and on the device (the same byte positions in both): its uploaded parts, then
// the region the device writes itself, then 16 bytes of slack for the kernels' last-word reads; every part 16-byte aligned.
//   records (at2v_verify_batch*; mb message bytes):                  pk | sig | offsets (c + 1, rebased) | messages | 16
//   transfers (at2v_verify_transfers*; mb = c x the message length): pk | sig | recipient | amount, which are uploaded
//             (c * 136 bytes in a row), | offsets (c + 1) | messages, which the prep kernel writes on the device, | 16
struct ChunkPart {
  size_t at, len;
  // built by the host in the slot (the rebased offsets), never read from the caller's memory by the DMA engine; it joins
  // the previous part's upload when both are staged. Its length is padded to 16, so its upload ends where the next part
  // begins. No other parts merge: a pageable chunk's arrays stay one upload each, each overlapping the next one's copy.
  bool built;
};
constexpr int kChunkParts = 4;
struct ChunkLayout {
  ChunkPart part[kChunkParts];  // the uploaded parts, in upload order (pk at 0)
  size_t sig, rcp, amt, off, msg;  // (rcp, amt: transfers only)
  size_t upload, total;            // the end of the uploaded parts, the end of the slack
};
inline ChunkLayout chunk_layout(size_t c, size_t mb, bool transfers = false) {
  const auto align16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  ChunkLayout l{};
  l.sig = c * 32;
  l.off = align16(transfers ? c * 136 : c * 96);
  l.msg = align16(l.off + (c + 1) * 4);
  l.total = l.msg + mb + 16;
  l.part[0] = {0, c * 32, false};
  l.part[1] = {l.sig, c * 64, false};
  if (transfers) {
    l.rcp = c * 96;
    l.amt = c * 128;
    l.part[2] = {l.rcp, c * 32, false};
    l.part[3] = {l.amt, c * 8, false};
    l.upload = c * 136;
  } else {
    l.part[2] = {l.off, l.msg - l.off, true};
    l.part[3] = {l.msg, mb, false};
    l.upload = l.msg + mb;
  }
  return l;
}

// device bytes a shard's part of a host call (m records, mb message bytes) takes in the pipe's arena: every chunk's
// layout, 256-aligned. Per record its field arrays and an offset; per chunk up to 16 bytes for each alignment that can
// pad (the messages; for transfers also the offsets, after c * 136), the extra offset, the slack, and up to 256 bytes to
// the next region.
inline size_t arena_bytes(size_t m, size_t mb, size_t first, bool transfers = false) {
  const size_t chunks = m / (first ? first : 1) + 2;
  const size_t fields = transfers ? 136 : 96, pads = transfers ? 2 : 1;
  return m * (fields + 4) + mb + chunks * (pads * 16 + 4 + 16 + 256) + 256;
}

// The uploads of one chunk, in order: one per part that has bytes, from the caller's memory where `direct` says the part's
// slice lies in pinned memory the DMA engine can read (never a built part), else from the slot; a built part staged
// behind a staged part shares that part's upload. The slot's completion signal starts at `count`. direct_bytes and
// staged_bytes are the caller's bytes that go either way (at2v_info: built parts are not counted); slot_bytes is how far
// the staged uploads reach into the slot.
struct Upload {
  size_t at, len;
  int part, parts;  // it covers parts [part, part + parts)
  bool direct;
};
struct UploadPlan {
  Upload up[kChunkParts];
  int count = 0;
  size_t direct_bytes = 0, staged_bytes = 0, slot_bytes = 0;
};
inline UploadPlan upload_plan(const ChunkLayout& l, const bool (&direct)[kChunkParts]) {
  UploadPlan p;
  for (int i = 0; i < kChunkParts; ++i) {
    const ChunkPart& pt = l.part[i];
    if (pt.len == 0) continue;
    const bool d = direct[i] && !pt.built;
    if (!pt.built) (d ? p.direct_bytes : p.staged_bytes) += pt.len;
    if (!d) p.slot_bytes = pt.at + pt.len;
    Upload* prev = p.count ? &p.up[p.count - 1] : nullptr;
    if (pt.built && prev && !prev->direct && prev->part + prev->parts == i) {
      prev->len = pt.at + pt.len - prev->at;
      ++prev->parts;
    } else {
      p.up[p.count++] = {pt.at, pt.len, i, 1, d};
    }
  }
  return p;
}

// Walk a plan: per upload, stage(u) fills the slot's bytes of a staged one, then submit(u) hands it to the DMA engine
// (false: the submit failed). Stops at the first failed submit, so nothing after it is staged or submitted; returns how
// many were submitted. The caller then takes count minus that off the signal: exactly the uploads in flight bring it to 0.
template <class Stage, class Submit>
int walk_uploads(const UploadPlan& p, Stage&& stage, Submit&& submit) {
  for (int i = 0; i < p.count; ++i) {
    if (!p.up[i].direct) stage(p.up[i]);
    if (!submit(p.up[i])) return i;
  }
  return p.count;
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
