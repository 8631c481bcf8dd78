// joint_host.cpp — TEST ONLY: the joint-table form of the verify routine (verify_half_fu_joint, at2v_verify_fu.h: what
// the GPU's verify_kernel runs) on the HOST, through the CPU backend's accessor at2v::cpu_verify_one_joint and its host
// tables (at2-node_amd/csrc/at2v_cpu.cpp, compiled into this program). Built with -fsanitize=address,undefined and
// -DAT2V_FU_CHECK, so every scaled operand and column sum of the unsigned field is checked on the way (abort on a
// violation: the joint table build must stay inside the classes tools/gen_fu.py proves).
// usage:
//   joint_host verify <fixture.bin>...  every record, both policies: joint form against the stored verdicts and against
//                                       verify_half_fu (at2v_verify_one_policy); prints per file
//                                       "<n> <bad_dalek> <bad_sodium> <joint != plain>", exit 1 on any mismatch
//   joint_host recode                   stdin: one value per line, 64 hex digits (big-endian, < 2^256); stdout per line:
//                                       sc_recode2's digit count and its 8 output words (hex, word 0 first)
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/at2v.h"
#include "at2v_cpu.h"
#include "at2v_sc.h"

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
  std::atomic<size_t> next{0}, bad_d{0}, bad_s{0}, diff{0};
  auto work = [&] {
    for (size_t i; (i = next.fetch_add(1)) < n;) {
      const uint8_t* m = &msg[off[i]];
      const uint32_t len = off[i + 1] - off[i];
      const int want[2] = {vd[i], vs[i]};
      for (int policy = 0; policy < 2; ++policy) {
        const int j = at2v::cpu_verify_one_joint(&pk[32 * i], &sig[64 * i], m, len, policy);
        const int p = at2v_verify_one_policy(&pk[32 * i], &sig[64 * i], m, len, policy);
        if (j != want[policy]) {
          fprintf(stderr, "%s: record %zu policy %d: joint %d, expected %d\n", path, i, policy, j, want[policy]);
          ++(policy ? bad_s : bad_d);
        }
        if (j != p) ++diff;
      }
    }
  };
  unsigned T = std::thread::hardware_concurrency();
  T = T < 1 ? 1 : T > 8 ? 8 : T;
  std::vector<std::thread> th;
  for (unsigned t = 1; t < T; ++t) th.emplace_back(work);
  work();
  for (auto& x : th) x.join();
  printf("%zu %zu %zu %zu\n", n, bad_d.load(), bad_s.load(), diff.load());
  return (bad_d || bad_s || diff) ? 1 : 0;
}

static int run_recode() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    if (strlen(line) < 64) return 2;
    uint32_t s[8], out[8];
    for (int w = 0; w < 8; ++w) {  // word w: hex digits 56 - 8w .. 63 - 8w
      char h[9];
      memcpy(h, line + 56 - 8 * w, 8);
      h[8] = 0;
      s[w] = (uint32_t)strtoul(h, nullptr, 16);
    }
    const int nd = at2v::sc_recode2(out, s);
    printf("%d", nd);
    for (int w = 0; w < 8; ++w) printf(" %08x", out[w]);
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && strcmp(argv[1], "recode") == 0) return run_recode();
  if (argc >= 3 && strcmp(argv[1], "verify") == 0) {
    int rc = 0;
    for (int a = 2; a < argc; ++a) {
      const int r = run_verify(argv[a]);
      if (r) rc = r;
    }
    return rc;
  }
  fprintf(stderr, "usage: joint_host verify <fixture.bin>... | joint_host recode\n");
  return 2;
}
