// reason_host.cpp — TEST ONLY: the reject-reasons routine on the HOST under AddressSanitizer + UBSan: reject_reason
// (at2-node_amd/csrc/at2v_reason.h, the function the device kernel runs per rejected record) called directly, and
// cpu_reject_reasons (at2v_cpu.cpp, compiled into this program: the CPU backend's pass over a thread pool), over golden
// fixture files. The expected bytes come from the caller (tests/reason_ref.py, Python integers only).
// usage:
//   reason_host <fixture.bin> <expected.bin>   expected.bin: n bytes for DALEK_V1, then n bytes for LIBSODIUM_1_0_18
// prints "<n> <direct != expected, dalek> <pool != expected, dalek> <direct, sodium> <pool, sodium> <guard bytes hit>";
// exit 1 on any mismatch. The verdict bits are the fixture's stored verdicts. The reasons buffer is exactly n + 64 bytes
// of heap, the last 64 a guard pattern that must survive (ASan catches anything past them).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/at2v.h"
#include "at2v_cpu.h"
#include "at2v_reason.h"

static void words8(uint32_t w[8], const uint8_t* b) {
  for (int i = 0; i < 8; ++i) w[i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
}

static bool read_all(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  out.resize((size_t)sz);
  const bool ok = fread(out.data(), 1, out.size(), f) == out.size();
  fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: reason_host <fixture.bin> <expected.bin>\n");
    return 2;
  }
  std::vector<uint8_t> fx, want;
  if (!read_all(argv[1], fx) || !read_all(argv[2], want) || fx.size() < 16) return 2;
  uint32_t hdr[4];
  memcpy(hdr, fx.data(), 16);
  const size_t n = hdr[2], mb = hdr[3];
  if (fx.size() != 16 + 32 * n + 64 * n + 4 * (n + 1) + mb + 3 * n || want.size() != 2 * n) return 2;
  const uint8_t* pk = fx.data() + 16;
  const uint8_t* sig = pk + 32 * n;
  const uint8_t* verdict[2] = {sig + 64 * n + 4 * (n + 1) + mb, sig + 64 * n + 4 * (n + 1) + mb + n};
  at2v::CpuPool* pool = at2v::copy_pool_create(4);  // (a pool without the verify tables: the pass needs none)
  if (!pool) return 2;
  size_t bad[4] = {0, 0, 0, 0}, guard = 0;
  for (int policy = 0; policy < 2; ++policy) {
    std::vector<uint32_t> words((n + 31) / 32, 0u);
    for (size_t i = 0; i < n; ++i) words[i >> 5] |= (uint32_t)(verdict[policy][i] & 1) << (i & 31);
    const uint8_t* exp = want.data() + policy * n;
    for (size_t i = 0; i < n; ++i) {
      int r = AT2V_REASON_VALID;
      if (!verdict[policy][i]) {
        uint32_t A[8], R[8], S[8];
        words8(A, pk + 32 * i);
        words8(R, sig + 64 * i);
        words8(S, sig + 64 * i + 32);
        r = at2v::reject_reason(A, R, S, policy);
      }
      if (r != exp[i]) {
        fprintf(stderr, "%s: record %zu policy %d: reject_reason %d, expected %d\n", argv[1], i, policy, r, exp[i]);
        ++bad[2 * policy];
      }
    }
    uint8_t* out = static_cast<uint8_t*>(malloc(n + 64));
    if (!out) return 2;
    memset(out, 0xA5, n + 64);
    at2v::cpu_reject_reasons(pool, pk, sig, n, words.data(), policy, out);
    for (size_t i = 0; i < n; ++i) bad[2 * policy + 1] += out[i] != exp[i];
    for (size_t i = n; i < n + 64; ++i) guard += out[i] != 0xA5;
    free(out);
  }
  at2v::cpu_pool_destroy(pool);
  printf("%zu %zu %zu %zu %zu %zu\n", n, bad[0], bad[1], bad[2], bad[3], guard);
  return (bad[0] || bad[1] || bad[2] || bad[3] || guard) ? 1 : 0;
}
