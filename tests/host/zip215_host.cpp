// zip215_host.cpp — TEST ONLY: every host-compilable verify route of the shared headers under AT2V_POLICY_ZIP215 (or any
// other policy), in a stand-alone program built with -fsanitize=address,undefined and -DAT2V_FU_CHECK (every scaled
// operand checked against 2^32, every column sum against 2^64: abort on violation). It reads ONE fixture file in the
// tests/golden layout, written by tests/test_zip215_host.py, whose verdict_dalek column holds the verdicts expected under
// the policy asked for (tests/zip215_ref.py's, never the library's), and compares every route's verdicts with it.
// The host table classes are verify_host.cpp's own (one copy: that file is included with its main renamed); the
// per-thread views of them are as in legacy_host.cpp.
// usage: zip215_host <policy> <n_all> <stride> <route>[,<route>...] <fixture.bin>
//   routes: half_fu, joint (verify_half_fu_joint), pair (verify_pair_part + verify_pair_combine), split (split_a_side /
//           split_r_side / split_side_ladder / split_combine), comb16 / comb20 / comb24 (verify_comb_fu: the throughput
//           comb with that recoding of s), comb_lat (comb_decode_r + comb_check_split: the four-wave form)
//   a record is run when its index is below <n_all> or a multiple of <stride>
//   stdout, per route: "<route> <records run> <mismatches> [first mismatching indices]"; exit status 1 on any mismatch
// usage: zip215_host bounds   -> the cofactored tail's new product sites at the extremes of their operand classes (the
//   subtraction of a decoded point, three doublings after the last addition, the completion after the pair combine) and
//   their values on real points; prints "ok <checks>"
#define main verify_host_main
#include "verify_host.cpp"
#undef main

#include <atomic>
#include <string>
#include <thread>

struct HostTabJ {  // the joint table of A and R (verify_half_fu_joint), as the CPU backend's
  gu_cached e[kJointEntries];
  int pending[2] = {0, 0};
  void store(int i, const gu_cached& c) { e[i] = c; }
  void prefetch(int st, int i, bool) { pending[st] = i; }
  void load_prefetched(int st, gu_cached& c) const { c = e[pending[st]]; }
};

struct Fixed {  // the process's fixed-base tables, built before any worker starts
  HostTabB16 tb;
  HostTabB16Hi tb1;
  HostTabBFu<HostTabB16> fb0{tb};
  HostTabBFu<HostTabB16Hi> fb1{tb1};
};

template <class N>
struct View {  // a thread's view of a shared fixed-base table (the pending entry is the thread's own)
  const std::vector<N>* t;
  mutable int pending = 0;
  void prefetch(int e) const { pending = e; }
  void load_prefetched(N& n) const { n = (*t)[pending]; }
};

struct Worker {  // per thread: table views, and the on-demand combs (caches)
  explicit Worker(const Fixed& fx) : tb{&fx.tb.t}, tb1{&fx.tb1.t}, fb0{&fx.fb0.t}, fb1{&fx.fb1.t} {}
  View<ge_niels> tb, tb1;
  View<gu_niels> fb0, fb1;
  std::map<std::vector<uint32_t>, HostComb> combs;
  HostBCombW<16> b16;
  HostBCombW<20> b20;
  HostBCombW<24> b24;
  const HostComb& comb(const uint32_t A[8]) {
    std::vector<uint32_t> key(A, A + 8);
    auto it = combs.find(key);
    if (it == combs.end()) {
      if (combs.size() >= 64) combs.clear();  // 2.1 MB each
      it = combs.try_emplace(key, A).first;
    }
    return it->second;
  }
};


template <class MW>
static int run_zip_route(const std::string& route, int policy, Worker& wk, const uint32_t R[8], const uint32_t A[8],
                         const uint32_t S[8], uint32_t len, MW mw) {
  auto one = [](int v) { return v; };
  if (route == "half_fu") {
    HostTabAFu fa, fr;
    return verify_half_fu(R, A, S, len, mw, policy, fa, fr, wk.fb0, wk.fb1, one);
  }
  if (route == "joint") {
    HostTabJ tj;
    return verify_half_fu_joint(R, A, S, len, mw, policy, tj, wk.fb0, wk.fb1, one);
  }
  if (route == "pair") {
    HostTabAFu f0, f1;
    gu_p3 P0, P1;
    const int ok0 = verify_pair_part(0, R, A, S, len, mw, policy, f0, wk.fb0, one, P0);
    const int ok1 = verify_pair_part(1, R, A, S, len, mw, policy, f1, wk.fb1, one, P1);
    gu_cached c1;
    gu_p3_to_cached(c1, P1);
    return ok0 & ok1 & verify_pair_combine(P0, c1, policy);
  }
  if (route == "split") {
    HostTabAFu fa, fr;
    gu_p3 Ad, P0, P1;
    const int ok0 = split_a_side(Ad, R, A, S, policy, fa);
    const int ok1 = split_r_side(R, fr, policy);
    uint32_t c0d[8], c1d[8], td[kBCombLatDigitWords];
    int c1_neg, nw;
    const int ok2 = split_scalars(c0d, c1d, td, c1_neg, nw, R, A, S, len, mw);
    nw = nw < 1 ? 1 : nw;
    split_side_ladder(P0, c0d, nw, 0, fa);
    split_side_ladder(P1, c1d, nw, c1_neg, fr);
    gu_cached c1, ntb;
    gu_p3_to_cached(c1, P1);
    split_neg_tb(ntb, td, wk.b16);
    return ok0 & ok1 & ok2 & split_combine(P0, c1, ntb, policy);
  }
  const HostComb& c = wk.comb(A);
  if (route == "comb16") return verify_comb_fu(R, A, S, len, mw, policy, c.a_ok, c, wk.b16);
  if (route == "comb20") return verify_comb_fu(R, A, S, len, mw, policy, c.a_ok, c, wk.b20);
  if (route == "comb24") return verify_comb_fu(R, A, S, len, mw, policy, c.a_ok, c, wk.b24);
  if (route == "comb_lat") {
    gu_p3 Rp, Pb, Pa0, Pa1;
    const int ok0 = comb_decode_r(Rp, R, policy) & comb_prechecks(R, A, S, policy, c.a_ok);
    const int sok = sc_v1_ok(S, policy);  // wave 1's share of the verdict (at2v_kern_comb.h sok[])
    uint32_t sd[kBCombLatDigitWords], kd[kCombDigitWords];
    bcomb_recode<kBCombLatBits>(sd, S);
    gu_p3_identity(Pb);
    comb_sum<false>(Pb, sd, 0, kBCombLatPos, wk.b16);
    comb_k_digits(kd, R, A, len, mw);
    gu_p3_identity(Pa0);
    gu_p3_identity(Pa1);
    comb_sum<true>(Pa0, kd, 0, kCombPos / 2, c);
    comb_sum<true>(Pa1, kd, kCombPos / 2, kCombPos, c);
    return ok0 & sok & comb_check_split(Rp, Pa0, Pa1, Pb, policy);
  }
  fprintf(stderr, "unknown route %s\n", route.c_str());
  exit(2);
}

#define EXPECT(c)                                             \
  do {                                                        \
    ++checks;                                                 \
    if (!(c)) {                                               \
      fprintf(stderr, "check failed at line %d\n", __LINE__); \
      return 1;                                               \
    }                                                         \
  } while (0)

// The new product sites of the cofactored tail on all-maximal carried limbs (products are monotonic in their operands,
// so these bound every reachable column; tools/gen_fu.py check_group_law proves the same statically), then on points.
static int bounds() {
  int checks = 0;
  fu C;
  for (int i = 0; i < 10; ++i) C.v[i] = (1u << ((i & 1) ? 25 : 26)) - 1;
  C.v[1] += kFuLimb1Spill;
  const gu_p3 M3{C, C, C, C};
  // three doublings after the last addition / mixed addition, both signs: p1p1 -> p2 -> [8]
  gu_cached ca;
  gu_p3_to_cached(ca, M3);
  gu_niels nb{C, C, C};
  gu_p1p1 t;
  gu_p2 Q2;
  for (int neg = 0; neg < 2; ++neg) {
    gu_cached c2 = ca;
    gu_cached_cneg(c2, neg);
    gu_add(t, M3, c2);
    gu_p1p1_to_p2(Q2, t);
    (void)gu_p2_mul8_is_identity(Q2);
    (void)verify_pair_combine(M3, c2, POLICY_ZIP215);  // the completion after the pair combine
    gu_niels n2 = nb;
    gu_niels_cneg(n2, neg);
    gu_madd(t, M3, n2);
    gu_p1p1_to_p2(Q2, t);
    (void)gu_p2_mul8_is_identity(Q2);
  }
  (void)gu_p2_mul8_is_identity(gu_p2{C, C, C});
  // the subtraction of a decoded point: the largest encodings (y = 2^255 - 1, both signs) and all-maximal limbs
  uint32_t s[8];
  for (int k = 0; k < 8; ++k) s[k] = 0xffffffffu;
  gu_p3 R;
  (void)gu_frombytes(R, s);
  (void)gu_cofactored_eq(M3, R);
  s[7] = 0x7fffffffu;
  (void)gu_frombytes(R, s);
  (void)gu_cofactored_eq(M3, R);
  (void)gu_cofactored_eq(M3, M3);
  (void)comb_cofactored_ok(M3, s);
  // values: B - B is the identity, B - 0 is not; a point of order 8 passes the cofactored test and fails the plain one
  const uint32_t by[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                          0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};  // y = 4/5
  const uint32_t y8[8] = {0x706a17c7u, 0x4fd84d3du, 0x760b3cbau, 0x0f67100du,   // a point of order 8 (c7176a70...037a,
                          0xfa53202au, 0xc6cc392cu, 0x77fdc74eu, 0x7a03ac92u};  // on libsodium's blocklist)
  gu_p3 B, T8, I;
  EXPECT(gu_frombytes(B, by) == 1 && gu_frombytes(T8, y8) == 1);
  gu_p3_identity(I);
  EXPECT(gu_cofactored_eq(B, B) == 1);
  EXPECT(gu_cofactored_eq(B, I) == 0);
  EXPECT(gu_cofactored_eq(I, T8) == 1 && gu_cofactored_eq(T8, I) == 1);
  gu_p2 q;
  gu_p3_to_p2(q, T8);
  EXPECT(gu_p2_is_identity(q) == 0 && gu_p2_mul8_is_identity(q) == 1);
  gu_p2_dbl(t, q);
  gu_p1p1_to_p2(q, t);
  gu_p2_dbl(t, q);
  gu_p1p1_to_p2(q, t);
  EXPECT(gu_p2_is_identity(q) == 0);  // [4]T8 is the point of order 2: two doublings are not enough
  // B + T8 against B: equal up to torsion only
  gu_cached c8;
  gu_p3_to_cached(c8, T8);
  gu_add(t, B, c8);
  gu_p3 BT;
  gu_p1p1_to_p3(BT, t);
  EXPECT(gu_cofactored_eq(BT, B) == 1);
  gu_cached cb;
  gu_p3_to_cached(cb, B);
  gu_cached_cneg(cb, 1);
  EXPECT(verify_pair_combine(BT, cb, POLICY_ZIP215) == 1 && verify_pair_combine(BT, cb, POLICY_DALEK_V1) == 0);
  EXPECT(comb_cofactored_ok(BT, by) == 1 && comb_cofactored_ok(BT, y8) == 0);
  printf("ok %d\n", checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "bounds") return bounds();
  if (argc != 6) {
    fprintf(stderr, "usage: zip215_host <policy> <n_all> <stride> <route>[,...] <fixture.bin> | zip215_host bounds\n");
    return 2;
  }
  const int policy = atoi(argv[1]);
  const size_t n_all = (size_t)atoi(argv[2]);
  const size_t stride = (size_t)atoi(argv[3]) < 1 ? 1 : (size_t)atoi(argv[3]);
  std::vector<std::string> routes;
  for (std::string r = argv[4]; !r.empty();) {
    const size_t c = r.find(',');
    routes.push_back(r.substr(0, c));
    r = c == std::string::npos ? "" : r.substr(c + 1);
  }
  static const Fixed fx;
  FILE* f = fopen(argv[5], "rb");
  if (!f) return 2;
  uint32_t hdr[4];
  if (fread(hdr, 4, 4, f) != 4) return 2;
  const size_t n = hdr[2], mb = hdr[3];
  std::vector<uint8_t> pk(32 * n), sig(64 * n), msg(mb + 8), want(n);
  std::vector<uint32_t> off(n + 1);
  size_t got = fread(pk.data(), 32, n, f) + fread(sig.data(), 64, n, f) + fread(off.data(), 4, n + 1, f);
  got += fread(msg.data(), 1, mb, f) + fread(want.data(), 1, n, f);
  fclose(f);
  if (got != 2 * n + n + 1 + mb + n) return 2;
  int rc = 0;
  for (const std::string& route : routes) {
    std::vector<uint8_t> res(n, 2);  // 2: not run
    std::atomic<size_t> next{0};
    auto work = [&] {
      Worker wk(fx);
      for (size_t i; (i = next.fetch_add(1)) < n;) {
        if (i >= n_all && i % stride != 0) continue;
        uint32_t R[8], A[8], S[8];
        words(R, &sig[64 * i]);
        words(S, &sig[64 * i + 32]);
        words(A, &pk[32 * i]);
        const uint8_t* m = &msg[off[i]];
        const uint32_t len = off[i + 1] - off[i];
        auto mw = [&](uint32_t j) -> uint32_t {
          uint32_t v = 0;
          for (int b = 0; b < 4; ++b)
            if (4 * j + b < len) v |= (uint32_t)m[4 * j + b] << (8 * b);
          return v;
        };
        res[i] = run_zip_route(route, policy, wk, R, A, S, len, mw) ? 1 : 0;
      }
    };
    unsigned T = std::thread::hardware_concurrency();
    T = T < 1 ? 1 : T > 8 ? 8 : T;
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
    size_t ran = 0, bad = 0;
    std::string first;
    for (size_t i = 0; i < n; ++i) {
      if (res[i] == 2) continue;
      ++ran;
      if (res[i] != want[i]) {
        if (bad++ < 8) first += " " + std::to_string(i);
      }
    }
    printf("%s %zu %zu%s\n", route.c_str(), ran, bad, first.c_str());
    fflush(stdout);
    if (bad) rc = 1;
  }
  return rc;
}
