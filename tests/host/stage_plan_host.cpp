// stage_plan_host.cpp — the arithmetic of the host-buffer pipeline (csrc/at2v_stage_plan.h) on the host, under
// AddressSanitizer + UBSan (tests/test_stage_plan_host.py and tests/test_transfer_plan_host.py build and run it). No HIP:
// the header is plain C++. `records` and `transfers` are the two forms of a chunk (at2v_verify_batch*, at2v_verify_transfers*).
//   plan     records: every chunk schedule over a grid of stage sizes, small-batch limits, part sizes and message lengths:
//   tplan    the chunks cover the part, keep their size rules, have aligned, disjoint parts, and their layouts fit the arena
//            that arena_bytes sizes (the inequality issue_chunk relies on); tplan: the same for transfers
//   layout   chunk_layout of a records chunk: aligned, disjoint parts
//   uploads  upload_plan over every direct / staged combination of a chunk's parts: today's upload sequences, each part
//            covered once, the byte accounting; walk_uploads with a submit that fails at every position: nothing after the
//            failure is staged or submitted, and the signal's count ends at exactly 0
//   copy     CopyJob: the pieces cover their ranges exactly once and reproduce a memcpy / the rebased offsets
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "at2v_stage_plan.h"
#include "at2v_transfer.h"

namespace {

[[noreturn]] void fail(const char* what, size_t a = 0, size_t b = 0, size_t c = 0, size_t d = 0) {
  std::printf("FAIL %s: %zu %zu %zu %zu\n", what, a, b, c, d);
  std::exit(1);
}

// records:   pk [0, 32c) | sig [sig, sig + 64c) | offsets [off, off + 4(c + 1)) | messages [msg, msg + mb) = upload | 16
// transfers: pk [0, 32c) | sig | recipient | amount [amt, amt + 8c) = upload | offsets (c + 1) | messages mb | 16
at2v::ChunkLayout checked_layout(bool transfers, size_t c, size_t mb) {
  const at2v::ChunkLayout L = at2v::chunk_layout(c, mb, transfers);
  if (L.sig % 16 || L.rcp % 16 || L.amt % 16 || L.off % 16 || L.msg % 16)
    fail("part not 16-byte aligned", c, L.amt, L.off, L.msg);
  if (c * 32 > L.sig || L.off + (c + 1) * 4 > L.msg) fail("parts overlap", c, mb);
  if (L.msg - (L.off + (c + 1) * 4) >= 16) fail("more padding than alignment needs", c, mb);
  if (transfers) {
    if (L.sig + c * 64 > L.rcp || L.rcp + c * 32 > L.amt || L.amt + c * 8 > L.upload || L.upload > L.off ||
        L.msg + mb + 16 != L.total)
      fail("parts overlap", c, mb);
    if (L.upload != c * at2v::kTransferFieldBytes) fail("upload is not the four field arrays", c, L.upload);
    if (L.off - L.upload >= 16) fail("more padding than alignment needs", c);
  } else {
    if (L.sig + c * 64 > L.off) fail("parts overlap", c, mb);
    if (L.msg + mb != L.upload || L.upload + 16 != L.total) fail("upload / total", c, mb, L.upload, L.total);
  }
  // the uploaded parts are the named ones, in order (the offsets padded to where the messages begin)
  const size_t at[4] = {0, L.sig, transfers ? L.rcp : L.off, transfers ? L.amt : L.msg};
  const size_t len[4] = {c * 32, c * 64, transfers ? c * 32 : L.msg - L.off, transfers ? c * 8 : mb};
  for (int i = 0; i < 4; ++i)
    if (L.part[i].at != at[i] || L.part[i].len != len[i] || L.part[i].built != (!transfers && i == 2))
      fail("part table", c, mb, (size_t)i);
  return L;
}

int run_plan(bool transfers) {
  const size_t firsts[] = {64, 128, 1024, 65536}, maxes[] = {64, 256, 4096, 131072};
  std::vector<size_t> pair_maxes = {0, 1, 64, 1000, 2048}, ms, lens;
  if (transfers) {
    pair_maxes.push_back(32768);
    ms = {1, 63, 64, 65, 4096, 131073, 1000003};
    lens = {48, 40};
  } else {
    for (size_t m = 1; m <= 700; ++m) ms.push_back(m);
    std::mt19937_64 rng(0xA72);
    for (int i = 0; i < 299; ++i) ms.push_back(1 + (size_t)(rng() % 1999999));  // below 2,000,000
    lens = {0, 1, 48, 100, 4097};
  }
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
          size_t sum = 0, count = 0;
          std::vector<size_t> arena(lens.size(), 0);
          while (!cp.done()) {
            const size_t at = cp.pos, c = cp.take();
            if (c == 0 || at + c > m || cp.pos != at + c) fail("chunk range", m, at, c);
            const bool last = cp.done();
            if (!last && c % 64) fail("a chunk before the last is no multiple of 64", m, at, c);
            if (!last && at % 64) fail("a chunk starts inside a verdict word pair", m, at, c);
            if (c > cap && !(last && c < cap + first)) fail("chunk above the cap", m, at, c, cap);
            for (size_t k = 0; k < lens.size(); ++k) {  // (the records grid is large: its layouts' parts are `layout`'s)
              const at2v::ChunkLayout L =
                  transfers ? checked_layout(true, c, c * lens[k]) : at2v::chunk_layout(c, c * lens[k]);
              arena[k] += (L.total + 255) & ~(size_t)255;
            }
            sum += c;
            ++count;
            if (count > m) fail("plan does not end", m);
          }
          if (sum != m) fail("chunks do not sum to m", m, sum);
          if (m <= pair_max && count != 1) fail("a small part is not one chunk", m, pair_max, count);
          for (size_t k = 0; k < lens.size(); ++k) {
            const size_t have =
                at2v::arena_bytes(m, m * lens[k], std::min(stage_first, std::max<size_t>(m, 1)), transfers);
            if (arena[k] > have) fail("arena too small", m, lens[k], arena[k], have);
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
    for (size_t len : {(size_t)0, (size_t)1, (size_t)48, (size_t)100, (size_t)4097}) {
      checked_layout(false, c, c * len);
      ++cases;
    }
  std::printf("cases %zu\n", cases);
  return 0;
}

// One chunk under one choice of direct parts (bit i of mask: part i lies in pinned memory; for a records chunk bit 2 is
// the offsets part, which must stay staged whatever the caller says).
void check_uploads(bool transfers, size_t c, size_t mb, unsigned mask) {
  const at2v::ChunkLayout L = checked_layout(transfers, c, mb);
  bool direct[at2v::kChunkParts];
  for (int i = 0; i < at2v::kChunkParts; ++i) direct[i] = mask >> i & 1;
  const at2v::UploadPlan P = at2v::upload_plan(L, direct);
  // the order and the ranges the timings rest on, written out
  struct Want {
    size_t at, len;
    bool direct;
  };
  std::vector<Want> want = {{0, c * 32, direct[0]}};
  if (transfers) {
    want.push_back({L.sig, c * 64, direct[1]});
    want.push_back({L.rcp, c * 32, direct[2]});
    want.push_back({L.amt, c * 8, direct[3]});
  } else {
    if (direct[1]) {  // sig from the caller, then the offsets from the slot
      want.push_back({L.sig, c * 64, true});
      want.push_back({L.off, L.msg - L.off, false});
    } else {  // one upload of sig through the end of the offsets
      want.push_back({L.sig, L.msg - L.sig, false});
    }
    if (mb) want.push_back({L.msg, mb, direct[3]});
  }
  const size_t formula = transfers ? 4 : 1 + (direct[1] ? 2 : 1) + (mb ? 1 : 0);
  if ((size_t)P.count != want.size() || (size_t)P.count != formula) fail("upload count", c, mb, mask, (size_t)P.count);
  std::vector<uint8_t> cover(L.upload, 0);
  size_t end = 0, slot = 0;
  for (int i = 0; i < P.count; ++i) {
    const at2v::Upload& u = P.up[i];
    if (u.at != want[i].at || u.len != want[i].len || u.direct != want[i].direct) fail("upload order", c, mb, mask, (size_t)i);
    if (u.at < end || u.at + u.len > L.upload) fail("uploads overlap or leave the uploaded region", c, mb, mask, (size_t)i);
    end = u.at + u.len;
    if (!u.direct) slot = end;
    for (int k = u.part; k < u.part + u.parts; ++k)
      if (L.part[k].built && u.direct) fail("the offsets are sourced from the caller", c, mb, mask);
    if (u.direct && u.parts != 1) fail("a direct upload covers more than its part", c, mb, mask);
    for (size_t o = 0; o < u.len; ++o) ++cover[u.at + o];
  }
  for (const at2v::ChunkPart& pt : L.part)
    for (size_t o = 0; o < pt.len; ++o)
      if (cover[pt.at + o] != 1) fail("a part's byte is not uploaded exactly once", c, mb, mask, pt.at + o);
  if (P.slot_bytes != slot) fail("slot bytes are not the end of the staged uploads", c, mb, P.slot_bytes, slot);
  size_t d = 0;
  for (int i = 0; i < at2v::kChunkParts; ++i)
    if (direct[i] && !L.part[i].built) d += L.part[i].len;
  const size_t all = transfers ? c * 136 : c * 96 + mb;
  if (P.direct_bytes != d || P.direct_bytes + P.staged_bytes != all) fail("byte accounting", c, mb, mask, P.direct_bytes);
  // the walk, with the submit failing at upload k (k == count: never); `signal` stands in for the slot's signal
  for (int k = 0; k <= P.count; ++k) {
    long signal = P.count;
    std::vector<int> log;  // upload i staged: 2i, submitted: 2i + 1
    const int submitted = at2v::walk_uploads(
        P, [&](const at2v::Upload& u) { log.push_back(2 * (int)(&u - P.up)); },
        [&](const at2v::Upload& u) {
          const int i = (int)(&u - P.up);
          if (i == k) return false;
          log.push_back(2 * i + 1);
          return true;
        });
    if (submitted != k) fail("walk: submitted count", c, mb, mask, (size_t)k);
    std::vector<int> expect;  // everything before the failing upload, its own staging, and nothing after
    for (int i = 0; i < P.count && i <= k; ++i) {
      if (!P.up[i].direct) expect.push_back(2 * i);
      if (i < k) expect.push_back(2 * i + 1);
    }
    if (log != expect) fail("walk: staged or submitted out of turn", c, mb, mask, (size_t)k);
    signal -= P.count - submitted;  // issue_chunk's settling
    if (signal != submitted) fail("walk: the signal is not the uploads in flight", c, mb, mask, (size_t)k);
    for (int i = 0; i < submitted; ++i)
      if (--signal < 0) fail("walk: the signal went negative", c, mb, mask, (size_t)k);
    if (signal != 0) fail("walk: the signal does not end at 0", c, mb, mask, (size_t)k);
  }
}

int run_uploads() {
  size_t cases = 0;
  for (bool transfers : {false, true})
    for (size_t c : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)4096})
      for (size_t mb : {(size_t)0, 100 * c})
        for (unsigned mask = 0; mask < 16; ++mask) {
          check_uploads(transfers, c, mb, mask);
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
  if (!std::strcmp(mode, "plan")) return run_plan(false);
  if (!std::strcmp(mode, "tplan")) return run_plan(true);
  if (!std::strcmp(mode, "layout")) return run_layout();
  if (!std::strcmp(mode, "uploads")) return run_uploads();
  if (!std::strcmp(mode, "copy")) return run_copy();
  std::fprintf(stderr, "usage: %s plan | tplan | layout | uploads | copy\n", argv[0]);
  return 2;
}
