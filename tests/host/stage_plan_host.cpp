// stage_plan_host.cpp — the arithmetic of the host-buffer pipeline (csrc/at2v_stage_plan.h) on the host, under
// AddressSanitizer + UBSan (tests/test_stage_plan_host.py builds and runs it). No HIP: the header is plain C++.
//   plan    every chunk schedule over a grid of stage sizes, small-batch limits, part sizes and message lengths: the
//           chunks cover the part, keep their size rules, and their layouts fit the arena that arena_bytes sizes
//           (the inequality issue_chunk relies on)
//   layout  chunk_layout: aligned, disjoint parts
//   copy    CopyJob: the pieces cover their ranges exactly once and reproduce a memcpy / the rebased offsets
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "at2v_stage_plan.h"

namespace {

[[noreturn]] void fail(const char* what, size_t a = 0, size_t b = 0, size_t c = 0, size_t d = 0) {
  std::printf("FAIL %s: %zu %zu %zu %zu\n", what, a, b, c, d);
  std::exit(1);
}

constexpr size_t kMsgLens[] = {0, 1, 48, 100, 4097};

int run_plan() {
  const size_t firsts[] = {64, 128, 1024, 65536}, maxes[] = {64, 256, 4096, 131072};
  const size_t pair_maxes[] = {0, 1, 64, 1000, 2048};
  std::vector<size_t> ms;
  for (size_t m = 1; m <= 700; ++m) ms.push_back(m);
  std::mt19937_64 rng(0xA72);
  for (int i = 0; i < 299; ++i) ms.push_back(1 + (size_t)(rng() % 1999999));  // below 2,000,000
  size_t cases = 0, chunks = 0;
  double tightest = 0;
  for (size_t stage_first : firsts)
    for (size_t max_in : maxes) {
      const size_t stage_max = std::max(max_in, stage_first);  // as at2v_create raises it
      for (size_t pair_max : pair_maxes)
        for (size_t m : ms) {
          at2v::ChunkPlan cp;
          cp.init(m, pair_max, stage_first, stage_max);
          const size_t first = cp.first, cap = std::max(stage_max, first);
          size_t sum = 0, count = 0, arena[5] = {0, 0, 0, 0, 0};
          while (!cp.done()) {
            const size_t at = cp.pos, c = cp.take();
            if (c == 0 || at + c > m || cp.pos != at + c) fail("chunk range", m, at, c);
            const bool last = cp.done();
            if (!last && c % 64) fail("a chunk before the last is no multiple of 64", m, at, c);
            if (!last && at % 64) fail("a chunk starts inside a verdict word pair", m, at, c);
            if (c > cap && !(last && c < cap + first)) fail("chunk above the cap", m, at, c, cap);
            for (int k = 0; k < 5; ++k) {
              const at2v::ChunkLayout L = at2v::chunk_layout(c, c * kMsgLens[k]);
              arena[k] += (L.total + 255) & ~(size_t)255;
            }
            sum += c;
            ++count;
            if (count > m) fail("plan does not end", m);
          }
          if (sum != m) fail("chunks do not sum to m", m, sum);
          if (m <= pair_max && count != 1) fail("a small part is not one chunk", m, pair_max, count);
          for (int k = 0; k < 5; ++k) {
            const size_t have = at2v::arena_bytes(m, m * kMsgLens[k], std::min(stage_first, std::max<size_t>(m, 1)));
            if (arena[k] > have) fail("arena too small", m, kMsgLens[k], arena[k], have);
            tightest = std::max(tightest, (double)arena[k] / (double)have);
            ++cases;
          }
          chunks += count;
        }
    }
  std::printf("cases %zu chunks %zu tightest %.7f\n", cases, chunks, tightest);
  return 0;
}

int run_layout() {
  size_t cases = 0;
  std::mt19937_64 rng(0x5EED);
  std::vector<size_t> cs;
  for (size_t c = 1; c <= 300; ++c) cs.push_back(c);
  for (int i = 0; i < 300; ++i) cs.push_back(1 + (size_t)(rng() % 2000000));
  for (size_t c : cs)
    for (size_t len : kMsgLens) {
      const size_t mb = c * len;
      const at2v::ChunkLayout L = at2v::chunk_layout(c, mb);
      if (L.sig % 16 || L.off % 16 || L.msg % 16) fail("part not 16-byte aligned", c, L.sig, L.off, L.msg);
      // pk [0, 32c) | sig [sig, sig + 64c) | offsets [off, off + 4(c + 1)) | messages [msg, msg + mb) | 16 bytes of slack
      if (c * 32 > L.sig || L.sig + c * 64 > L.off || L.off + (c + 1) * 4 > L.msg) fail("parts overlap", c, mb);
      if (L.msg - (L.off + (c + 1) * 4) >= 16) fail("more padding than alignment needs", c, mb);
      if (L.msg + mb != L.upload || L.upload + 16 != L.total) fail("upload / total", c, mb, L.upload, L.total);
      ++cases;
    }
  std::printf("cases %zu\n", cases);
  return 0;
}

// run a job's pieces in a scrambled order (the pool runs them on any thread in any order), batch by batch as run_copy does
void run_job(at2v::CopyJob& job, std::mt19937_64& rng) {
  std::vector<size_t> order(job.pieces.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  std::shuffle(order.begin(), order.end(), rng);
  job.base = 0;
  for (size_t i : order) at2v::CopyJob::run_piece(&job, i);
}

int run_copy() {
  const size_t P = at2v::kCopyPiece;
  std::mt19937_64 rng(0xC0B1);
  size_t cases = 0;
  for (size_t len : {(size_t)0, (size_t)1, (size_t)31, P - 1, P, P + 1, 2 * P, 3 * P + 17}) {
    std::vector<uint8_t> src(len + 1), dst(len + 1, 0xEE), cover(len, 0);
    for (uint8_t& b : src) b = (uint8_t)rng();
    at2v::CopyJob job;
    job.add(dst.data(), src.data(), len);
    if (job.pieces.size() != (len + P - 1) / P) fail("piece count", len, job.pieces.size());
    for (const at2v::CopyPiece& p : job.pieces) {
      if (p.offsets || p.len == 0 || p.len > P) fail("piece size", len, p.len);
      const size_t at = (size_t)(p.dst - dst.data());
      if (at + p.len > len || (size_t)(p.src - src.data()) != at) fail("piece range", len, at, p.len);
      for (size_t i = 0; i < p.len; ++i) ++cover[at + i];
    }
    for (size_t i = 0; i < len; ++i)
      if (cover[i] != 1) fail("byte not covered exactly once", len, i, cover[i]);
    run_job(job, rng);
    if (len && std::memcmp(dst.data(), src.data(), len) != 0) fail("copy differs from memcpy", len);
    if (dst[len] != 0xEE) fail("copy wrote past its range", len);
    ++cases;
  }
  const size_t S = P / 4;  // offsets per piece
  for (size_t count : {(size_t)0, (size_t)1, (size_t)65, S - 1, S, S + 1, 2 * S + 5}) {
    const uint32_t base = (uint32_t)(rng() % 1000000);
    std::vector<uint32_t> src(count + 1), dst(count + 1, 0xEEEEEEEEu);
    std::vector<uint8_t> cover(count, 0);
    uint32_t at = base;
    for (uint32_t& o : src) {
      o = at;
      at += (uint32_t)(rng() % 200);
    }
    at2v::CopyJob job;
    job.add_offsets(dst.data(), src.data(), count, base);
    if (job.pieces.size() != (count + S - 1) / S) fail("offset piece count", count, job.pieces.size());
    for (const at2v::CopyPiece& p : job.pieces) {
      if (!p.offsets || p.base != base || p.len == 0 || p.len * 4 > P) fail("offset piece size", count, p.len);
      const size_t i0 = (size_t)((const uint32_t*)p.dst - dst.data());
      if (i0 + p.len > count || (size_t)((const uint32_t*)p.src - src.data()) != i0) fail("offset piece range", count, i0);
      for (size_t i = 0; i < p.len; ++i) ++cover[i0 + i];
    }
    for (size_t i = 0; i < count; ++i)
      if (cover[i] != 1) fail("offset not covered exactly once", count, i, cover[i]);
    run_job(job, rng);
    for (size_t i = 0; i < count; ++i)
      if (dst[i] != src[i] - base) fail("offset not rebased", count, i, dst[i]);
    if (dst[count] != 0xEEEEEEEEu) fail("offsets wrote past their range", count);
    ++cases;
  }
  std::printf("cases %zu\n", cases);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!std::strcmp(mode, "plan")) return run_plan();
  if (!std::strcmp(mode, "layout")) return run_layout();
  if (!std::strcmp(mode, "copy")) return run_copy();
  std::fprintf(stderr, "usage: %s plan | layout | copy\n", argv[0]);
  return 2;
}
