// sq_operands_host.cpp — TEST ONLY: every squaring of the unsigned field (at2-node_amd/csrc/at2v_fu_gen.h) on the HOST
// against values computed elsewhere, built with -fsanitize=address,undefined and -DAT2V_FU_CHECK, so every scaled
// operand is checked against 2^32, every column sum against 2^64 and every one-MAD wrap's carry against 2^32 on the way
// (abort on a violation of the bounds tools/gen_fu.py proves for the operand set it chose per function).
// usage:
//   sq_operands_host sq                 stdin, one case per line: <fn> <10 limbs of f0> <10 limbs of f1> <e0> <e1>, limbs
//                                       in hex, e0/e1 the expected canonical results as 64 hex digits (big-endian);
//                                       fn: 0 fu_sq 1 fu_sq2 2 fu_sqc 3 fu_sq_x2 4 fu_sq_sq2 5 fu_sq_sq2_n 6 fu_sqc_x2.
//                                       A one-way function runs on f0 and then on f1. Prints "<cases> <mismatches>",
//                                       exit 1 on any mismatch
//   sq_operands_host verify <fixture.bin>...  every record, both policies, through cpu_verify_one_joint against the
//                                       stored verdicts; prints per file "<n> <bad_dalek> <bad_sodium>", exit 1 on any
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "at2v_cpu.h"
#include "at2v_fu.h"

using namespace at2v;

static bool equals_hex(const fu& h, const char* hex) {  // hex: 64 digits, most significant first
  uint32_t b[8];
  fu_tobytes(b, h);
  for (int w = 0; w < 8; ++w) {
    char d[9];
    memcpy(d, hex + 56 - 8 * w, 8);
    d[8] = 0;
    if (b[w] != (uint32_t)strtoul(d, nullptr, 16)) return false;
  }
  return true;
}

static int run_sq() {
  static char line[1024];
  size_t cases = 0, bad = 0;
  while (fgets(line, sizeof line, stdin)) {
    char* p = line;
    const long fn = strtol(p, &p, 10);
    fu f[2], h[2];
    for (int q = 0; q < 2; ++q)
      for (int i = 0; i < 10; ++i) f[q].v[i] = (uint32_t)strtoul(p, &p, 16);
    char e[2][80];
    if (sscanf(p, "%79s %79s", e[0], e[1]) != 2 || strlen(e[0]) != 64 || strlen(e[1]) != 64) return 2;
    switch (fn) {
      case 0: fu_sq(h[0], f[0]); fu_sq(h[1], f[1]); break;
      case 1: fu_sq2(h[0], f[0]); fu_sq2(h[1], f[1]); break;
      case 2: fu_sqc(h[0], f[0]); fu_sqc(h[1], f[1]); break;
      case 3: fu_sq_x2(h[0], f[0], h[1], f[1]); break;
      case 4: fu_sq_sq2(h[0], f[0], h[1], f[1]); break;
      case 5: fu_sq_sq2_n(h[0], f[0], h[1], f[1]); break;
      case 6: fu_sqc_x2(h[0], f[0], h[1], f[1]); break;
      default: return 2;
    }
    for (int q = 0; q < 2; ++q) {
      bool ok = equals_hex(h[q], e[q]);
      for (int i = 0; i < 10; ++i)  // the result is carried: what the next product's proof assumes
        ok = ok && h[q].v[i] <= ((i & 1) ? (1u << 25) - 1 : (1u << 26) - 1) + (i == 1 ? kFuLimb1Spill : 0);
      if (!ok) {
        if (++bad <= 10) fprintf(stderr, "fn %ld case %zu half %d: wrong result\n", fn, cases, q);
      }
    }
    ++cases;
  }
  printf("%zu %zu\n", cases, bad);
  return bad ? 1 : 0;
}

static int run_verify(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t hdr[4];
  if (fread(hdr, 4, 4, f) != 4) return 2;
  const size_t n = hdr[2], mb = hdr[3];
  std::vector<uint8_t> pk(32 * n), sig(64 * n), msg(mb + 1), vd(n), vs(n);
  std::vector<uint32_t> off(n + 1);
  size_t got = fread(pk.data(), 32, n, f) + fread(sig.data(), 64, n, f) + fread(off.data(), 4, n + 1, f);
  got += fread(msg.data(), 1, mb, f) + fread(vd.data(), 1, n, f) + fread(vs.data(), 1, n, f);
  fclose(f);
  if (got != 2 * n + n + 1 + mb + 2 * n) return 2;
  std::atomic<size_t> next{0}, bad_d{0}, bad_s{0};
  auto work = [&] {
    for (size_t i; (i = next.fetch_add(1)) < n;) {
      const int want[2] = {vd[i], vs[i]};
      for (int policy = 0; policy < 2; ++policy) {
        const int j = cpu_verify_one_joint(&pk[32 * i], &sig[64 * i], &msg[off[i]], off[i + 1] - off[i], policy);
        if (j != want[policy]) {
          fprintf(stderr, "%s: record %zu policy %d: joint %d, expected %d\n", path, i, policy, j, want[policy]);
          ++(policy ? bad_s : bad_d);
        }
      }
    }
  };
  unsigned T = std::thread::hardware_concurrency();
  T = T < 1 ? 1 : T > 8 ? 8 : T;
  std::vector<std::thread> th;
  for (unsigned t = 1; t < T; ++t) th.emplace_back(work);
  work();
  for (auto& x : th) x.join();
  printf("%zu %zu %zu\n", n, bad_d.load(), bad_s.load());
  return (bad_d || bad_s) ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && strcmp(argv[1], "sq") == 0) return run_sq();
  if (argc >= 3 && strcmp(argv[1], "verify") == 0) {
    int rc = 0;
    for (int a = 2; a < argc; ++a) {
      const int r = run_verify(argv[a]);
      if (r) rc = r;
    }
    return rc;
  }
  fprintf(stderr, "usage: sq_operands_host sq | sq_operands_host verify <fixture.bin>...\n");
  return 2;
}
