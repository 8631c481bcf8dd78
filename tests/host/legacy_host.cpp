// legacy_host.cpp — TEST ONLY: every host-compilable verify route of the shared headers under one policy (the wrapper,
// tests/test_legacy_host.py, asks for AT2V_POLICY_DALEK_V1_LEGACY = 2), printing the verdicts instead of judging them:
// the expected values are the wrapper's (tests/legacy_ref.py), never the library's. Built with
// -fsanitize=address,undefined like joint_host.cpp.
// The host table classes are verify_host.cpp's own (one copy: that file is included with its main renamed).
// usage: legacy_host <policy> <stride> <route>[,<route>...] <fixture.bin>...
//   routes: core (verify_core<16>), half (verify_half), half_fu, joint (verify_half_fu_joint), pair (verify_pair_part),
//           split (split_a_side ...), comb16 / comb20 / comb24 (verify_comb_fu with that recoding of s),
//           comb_lat (the low-latency kernel's four-way split: the sok[] site's bcomb_recode<16> and comb_prechecks)
//   a record is run when its index is a multiple of <stride> or its s >= l (the class the legacy rule is about)
//   stdout, per file and route: "<file> <route> <one character per record: 0, 1, or - for a record not run>"
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
static int run_route(const std::string& route, int policy, Worker& wk, const uint32_t R[8],
                     const uint32_t A[8], const uint32_t S[8], uint32_t len, MW mw) {
  auto one = [](int v) { return v; };
  if (route == "core") {
    HostTabA ta;
    auto rl = [&](uint32_t r[8]) { for (int q = 0; q < 8; ++q) r[q] = R[q]; };
    return verify_core<16>(R, A, S, len, mw, policy, ta, wk.tb, rl);
  }
  if (route == "half") {
    HostTabA ta, tr;
    return verify_half(R, A, S, len, mw, policy, ta, tr, wk.tb, wk.tb1, one);
  }
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
    return ok0 & ok1 & verify_pair_combine(P0, c1);
  }
  if (route == "split") {
    HostTabAFu fa, fr;
    gu_p3 Ad, P0, P1;
    const int ok0 = split_a_side(Ad, R, A, S, policy, fa);
    const int ok1 = split_r_side(R, fr);
    uint32_t c0d[8], c1d[8], td[kBCombLatDigitWords];
    int c1_neg, nw;
    const int ok2 = split_scalars(c0d, c1d, td, c1_neg, nw, R, A, S, len, mw);
    nw = nw < 1 ? 1 : nw;
    split_side_ladder(P0, c0d, nw, 0, fa);
    split_side_ladder(P1, c1d, nw, c1_neg, fr);
    gu_cached c1, ntb;
    gu_p3_to_cached(c1, P1);
    split_neg_tb(ntb, td, wk.b16);
    return ok0 & ok1 & ok2 & split_combine(P0, c1, ntb);
  }
  const HostComb& c = wk.comb(A);
  if (route == "comb16") return verify_comb_fu(R, A, S, len, mw, policy, c.a_ok, c, wk.b16);
  if (route == "comb20") return verify_comb_fu(R, A, S, len, mw, policy, c.a_ok, c, wk.b20);
  if (route == "comb24") return verify_comb_fu(R, A, S, len, mw, policy, c.a_ok, c, wk.b24);
  if (route == "comb_lat") {
    gu_p3 Rp, Pb, Pa0, Pa1;
    const int ok0 = comb_decode_r(Rp, R) & comb_prechecks(R, A, S, policy, c.a_ok);
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
    return ok0 & sok & comb_check_split(Rp, Pa0, Pa1, Pb);
  }
  fprintf(stderr, "unknown route %s\n", route.c_str());
  exit(2);
}

static bool s_ge_l(const uint32_t S[8]) { return !sc_is_canonical(S); }

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: legacy_host <policy> <stride> <route>[,<route>...] <fixture.bin>...\n");
    return 2;
  }
  const int policy = atoi(argv[1]);
  const size_t stride = (size_t)atoi(argv[2]) < 1 ? 1 : (size_t)atoi(argv[2]);
  std::vector<std::string> routes;
  for (std::string r = argv[3]; !r.empty();) {
    const size_t c = r.find(',');
    routes.push_back(r.substr(0, c));
    r = c == std::string::npos ? "" : r.substr(c + 1);
  }
  static const Fixed fx;
  for (int a = 4; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) return 2;
    uint32_t hdr[4];
    if (fread(hdr, 4, 4, f) != 4) return 2;
    const size_t n = hdr[2], mb = hdr[3];
    std::vector<uint8_t> pk(32 * n), sig(64 * n), msg(mb + 8);
    std::vector<uint32_t> off(n + 1);
    size_t got = fread(pk.data(), 32, n, f) + fread(sig.data(), 64, n, f) + fread(off.data(), 4, n + 1, f);
    got += fread(msg.data(), 1, mb, f);
    fclose(f);
    if (got != 2 * n + n + 1 + mb) return 2;
    for (const std::string& route : routes) {
      std::string out(n, '-');
      std::atomic<size_t> next{0};
      auto work = [&] {
        Worker wk(fx);
        for (size_t i; (i = next.fetch_add(1)) < n;) {
          uint32_t R[8], A[8], S[8];
          words(R, &sig[64 * i]);
          words(S, &sig[64 * i + 32]);
          words(A, &pk[32 * i]);
          if (i % stride != 0 && !s_ge_l(S)) continue;
          const uint8_t* m = &msg[off[i]];
          const uint32_t len = off[i + 1] - off[i];
          auto mw = [&](uint32_t j) -> uint32_t {
            uint32_t v = 0;
            for (int b = 0; b < 4; ++b)
              if (4 * j + b < len) v |= (uint32_t)m[4 * j + b] << (8 * b);
            return v;
          };
          out[i] = run_route(route, policy, wk, R, A, S, len, mw) ? '1' : '0';
        }
      };
      unsigned T = std::thread::hardware_concurrency();
      T = T < 1 ? 1 : T > 8 ? 8 : T;
      std::vector<std::thread> th;
      for (unsigned t = 1; t < T; ++t) th.emplace_back(work);
      work();
      for (auto& x : th) x.join();
      printf("%s %s %s\n", argv[a], route.c_str(), out.c_str());
      fflush(stdout);
    }
  }
  return 0;
}
