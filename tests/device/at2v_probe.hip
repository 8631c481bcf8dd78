// at2v_probe.hip — TEST ONLY: the inline field, group-law and scalar functions of at2-node_amd/csrc, one call per
// function, so a test can compare what they return with Python integers (tests/test_probe_host.py,
// tests/test_gpu_probe.py). Built into its own libat2v_probe.so; nothing here is linked into libat2v.so.
//
//   int at2v_probe_count(void)                                   number of probes
//   int at2v_probe_info(int op, const char** name, int* in_words, int* out_words, int* arg_min, int* arg_max)
//   int at2v_probe_run(int where, int op, int n, const uint32_t* in, uint32_t* out, int arg)
//
// at2v_probe_run is synchronous: `in` holds n cases of in_words host words each, `out` receives n x out_words, one lane
// per case. where = 0 runs the host compile of the functions in this thread; where = 1 copies the cases to device 0,
// runs them one per lane in 256-thread blocks (the device compile: the asm products of at2v_fu_gen.h, the reciprocal
// estimate of lehmer_round32) and copies the results back. Field elements travel as their ten raw limbs, never as
// encodings. Returns 0, -1 for a bad argument, or the hipError_t of the first HIP call that failed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "at2v_gu.h"
#include "at2v_lattice.h"

using namespace at2v;

namespace {

#define PROBE_FN static AT2V_HD AT2V_INLINE

PROBE_FN void ld(fu& f, const uint32_t* p) {
#pragma unroll
  for (int i = 0; i < 10; ++i) f.v[i] = p[i];
}
PROBE_FN void st(uint32_t* p, const fu& f) {
#pragma unroll
  for (int i = 0; i < 10; ++i) p[i] = f.v[i];
}
PROBE_FN void ldw(uint32_t* w, const uint32_t* p, int n) {
  for (int i = 0; i < n; ++i) w[i] = p[i];
}

#define OP_HEAD(NAME, NIN, NOUT, A0, A1)                 \
  struct op_##NAME {                                     \
    static constexpr int IN = NIN, OUT = NOUT, AMIN = A0, AMAX = A1; \
    static const char* name() { return #NAME; }          \
    PROBE_FN void run(const uint32_t* in, uint32_t* out, int arg) {  \
      (void)arg;
#define OP_END \
    }          \
  };

// ---- the fourteen products
#define OP_MUL1(NAME) OP_HEAD(NAME, 20, 10, 0, 0) fu f, g, h; ld(f, in); ld(g, in + 10); NAME(h, f, g); st(out, h); OP_END
#define OP_SQ1(NAME) OP_HEAD(NAME, 10, 10, 0, 0) fu f, h; ld(f, in); NAME(h, f); st(out, h); OP_END
#define OP_MUL2(NAME) OP_HEAD(NAME, 40, 20, 0, 0) fu f0, g0, f1, g1, h0, h1; ld(f0, in); ld(g0, in + 10); \
  ld(f1, in + 20); ld(g1, in + 30); NAME(h0, f0, g0, h1, f1, g1); st(out, h0); st(out + 10, h1); OP_END
#define OP_SQ2(NAME) OP_HEAD(NAME, 20, 20, 0, 0) fu f0, f1, h0, h1; ld(f0, in); ld(f1, in + 10); \
  NAME(h0, f0, h1, f1); st(out, h0); st(out + 10, h1); OP_END

OP_MUL1(fu_mul)
OP_SQ1(fu_sq)
OP_SQ1(fu_sq2)
OP_MUL2(fu_mul_x2)
OP_SQ2(fu_sq_x2)
OP_SQ2(fu_sq_sq2)
OP_MUL1(fu_mulc)
OP_SQ1(fu_sqc)
OP_MUL2(fu_mulc_x2)
OP_MUL1(fu_mul_n)
OP_MUL2(fu_mul_wn)
OP_MUL2(fu_mul_nn)
OP_SQ2(fu_sq_sq2_n)
OP_SQ2(fu_sqc_x2)

// ---- field utilities. arg of fu_sub / fu_neg: 0 = FU_KC, 1 = FU_K2C
OP_HEAD(fu_carry, 10, 10, 0, 0) fu h; ld(h, in); fu_carry(h); st(out, h); OP_END
OP_HEAD(fu_pcarry_even, 10, 10, 0, 0) fu h; ld(h, in); fu_pcarry_even(h); st(out, h); OP_END
OP_HEAD(fu_add, 20, 10, 0, 0) fu f, g, h; ld(f, in); ld(g, in + 10); fu_add(h, f, g); st(out, h); OP_END
OP_HEAD(fu_sub, 20, 10, 0, 1)
  fu f, g, h; ld(f, in); ld(g, in + 10);
  if (arg) fu_sub(h, f, g, FU_K2C); else fu_sub(h, f, g, FU_KC);
  st(out, h);
OP_END
OP_HEAD(fu_neg, 10, 10, 0, 1)
  fu f, h; ld(f, in);
  if (arg) fu_neg(h, f, FU_K2C); else fu_neg(h, f, FU_KC);
  st(out, h);
OP_END
OP_HEAD(fu_frombytes, 8, 10, 0, 0) uint32_t w[8]; ldw(w, in, 8); fu h; fu_frombytes(h, w); st(out, h); OP_END
OP_HEAD(fu_tobytes, 10, 8, 0, 0)
  fu f; ld(f, in); uint32_t w[8]; fu_tobytes(w, f);
  for (int i = 0; i < 8; ++i) out[i] = w[i];
OP_END
OP_HEAD(fu_iszero, 10, 1, 0, 0) fu f; ld(f, in); out[0] = (uint32_t)fu_iszero(f); OP_END
OP_HEAD(fu_isnegative, 10, 1, 0, 0) fu f; ld(f, in); out[0] = (uint32_t)fu_isnegative(f); OP_END
OP_HEAD(fu_sqn, 10, 10, 1, 1024) fu f, h; ld(f, in); fu_sqn(h, f, arg); st(out, h); OP_END
OP_HEAD(fu_sqn_x2, 20, 20, 1, 1024)
  fu f0, f1, h0, h1; ld(f0, in); ld(f1, in + 10); fu_sqn_x2(h0, f0, h1, f1, arg); st(out, h0); st(out + 10, h1);
OP_END
OP_HEAD(fu_invert, 10, 10, 0, 0) fu f, h; ld(f, in); fu_invert(h, f); st(out, h); OP_END
OP_HEAD(fu_pow22523, 10, 10, 0, 0) fu f, h; ld(f, in); fu_pow22523(h, f); st(out, h); OP_END
OP_HEAD(fu_pow22523_x2, 20, 20, 0, 0)
  fu f0, f1, h0, h1; ld(f0, in); ld(f1, in + 10); fu_pow22523_x2(h0, f0, h1, f1); st(out, h0); st(out + 10, h1);
OP_END

// ---- group law. A p2 is (X, Y, Z), a p3 (X, Y, Z, T), a cached point (YpX, YmX, Z2, T2d), a Niels point
// (ypx, ymx, xy2d), ten limbs each. arg of the additions and of the negations: the `neg` of gu_cached_cneg / gu_niels_cneg
PROBE_FN void ld_p3(gu_p3& p, const uint32_t* in) { ld(p.X, in); ld(p.Y, in + 10); ld(p.Z, in + 20); ld(p.T, in + 30); }
PROBE_FN void ld_p2(gu_p2& p, const uint32_t* in) { ld(p.X, in); ld(p.Y, in + 10); ld(p.Z, in + 20); }
PROBE_FN void st_p3(uint32_t* out, const gu_p3& p) { st(out, p.X); st(out + 10, p.Y); st(out + 20, p.Z); st(out + 30, p.T); }
PROBE_FN void ld_niels(gu_niels& q, const uint32_t* in) { ld(q.ypx, in); ld(q.ymx, in + 10); ld(q.xy2d, in + 20); }

OP_HEAD(gu_dbl_p2, 30, 30, 0, 0)   // gu_p2_dbl, gu_p1p1_to_p2
  gu_p2 p, r; ld_p2(p, in); gu_p1p1 t; gu_p2_dbl(t, p); gu_p1p1_to_p2(r, t);
  st(out, r.X); st(out + 10, r.Y); st(out + 20, r.Z);
OP_END
OP_HEAD(gu_dbl_p3, 30, 40, 0, 0)   // gu_p2_dbl, gu_p1p1_to_p3
  gu_p2 p; ld_p2(p, in); gu_p1p1 t; gu_p2_dbl(t, p); gu_p3 r; gu_p1p1_to_p3(r, t); st_p3(out, r);
OP_END
OP_HEAD(gu_p3_to_cached, 40, 40, 0, 1)   // gu_p3_to_cached, gu_cached_cneg
  gu_p3 p; ld_p3(p, in); gu_cached c; gu_p3_to_cached(c, p); gu_cached_cneg(c, arg);
  st(out, c.YpX); st(out + 10, c.YmX); st(out + 20, c.Z2); st(out + 30, c.T2d);
OP_END
OP_HEAD(gu_add, 80, 40, 0, 1)   // P + (neg ? -Q : Q): gu_p3_to_cached(Q), gu_cached_cneg, gu_add, gu_p1p1_to_p3
  gu_p3 p, q, r; ld_p3(p, in); ld_p3(q, in + 40);
  gu_cached c; gu_p3_to_cached(c, q); gu_cached_cneg(c, arg);
  gu_p1p1 t; gu_add(t, p, c); gu_p1p1_to_p3(r, t); st_p3(out, r);
OP_END
OP_HEAD(gu_niels_cneg, 30, 30, 0, 1)
  gu_niels q; ld_niels(q, in); gu_niels_cneg(q, arg); st(out, q.ypx); st(out + 10, q.ymx); st(out + 20, q.xy2d);
OP_END
OP_HEAD(gu_madd, 70, 40, 0, 1)   // P + (neg ? -Q : Q), Q affine Niels: gu_niels_cneg, gu_madd, gu_p1p1_to_p3
  gu_p3 p, r; ld_p3(p, in); gu_niels q; ld_niels(q, in + 40); gu_niels_cneg(q, arg);
  gu_p1p1 t; gu_madd(t, p, q); gu_p1p1_to_p3(r, t); st_p3(out, r);
OP_END
OP_HEAD(gu_p2_is_identity, 30, 1, 0, 0) gu_p2 p; ld_p2(p, in); out[0] = (uint32_t)gu_p2_is_identity(p); OP_END
OP_HEAD(gu_p2_mul8_is_identity, 30, 1, 0, 0)
  gu_p2 p; ld_p2(p, in); out[0] = (uint32_t)gu_p2_mul8_is_identity(p);
OP_END
OP_HEAD(gu_cofactored_eq, 80, 1, 0, 0)
  gu_p3 p, r; ld_p3(p, in); ld_p3(r, in + 40); out[0] = (uint32_t)gu_cofactored_eq(p, r);
OP_END
OP_HEAD(gu_frombytes, 8, 31, 0, 0)   // -> X, Y, T, ok
  uint32_t s[8]; ldw(s, in, 8); gu_p3 h; const int ok = gu_frombytes(h, s);
  st(out, h.X); st(out + 10, h.Y); st(out + 20, h.T); out[30] = (uint32_t)ok;
OP_END
OP_HEAD(gu_frombytes_x2, 16, 62, 0, 0)   // -> X, Y, T, ok of each
  uint32_t s0[8], s1[8]; ldw(s0, in, 8); ldw(s1, in + 8, 8); gu_p3 h0, h1; int ok[2];
  gu_frombytes_x2(h0, s0, h1, s1, ok);
  st(out, h0.X); st(out + 10, h0.Y); st(out + 20, h0.T); out[30] = (uint32_t)ok[0];
  st(out + 31, h1.X); st(out + 41, h1.Y); st(out + 51, h1.T); out[61] = (uint32_t)ok[1];
OP_END

// ---- scalars
OP_HEAD(sc_reduce512, 16, 8, 0, 0)
  uint32_t x[16], k[8]; ldw(x, in, 16); sc_reduce512(k, x);
  for (int i = 0; i < 8; ++i) out[i] = k[i];
OP_END
OP_HEAD(lattice, 16, 26, 0, 0)   // (k, s) -> c0, |c1|, c1_neg, bits, t: the record tests/host/lattice_host.cpp prints
  uint32_t k[8], s[8], t[8]; ldw(k, in, 8); ldw(s, in + 8, 8);
  HalfScalars h; lattice_reduce(h, k); sc_mul_signed(t, h, s);
  for (int i = 0; i < 8; ++i) { out[i] = h.c0[i]; out[8 + i] = h.c1[i]; out[18 + i] = t[i]; }
  out[16] = (uint32_t)h.c1_neg; out[17] = (uint32_t)h.bits;
OP_END
OP_HEAD(sc_recode2_joint, 16, 17, 0, 0)
  uint32_t c0[8], c1[8], d0[8], d1[8]; ldw(c0, in, 8); ldw(c1, in + 8, 8);
  const int nd = sc_recode2_joint(d0, d1, c0, c1);
  for (int i = 0; i < 8; ++i) { out[i] = d0[i]; out[8 + i] = d1[i]; }
  out[16] = (uint32_t)nd;
OP_END
#define OP_RECODE(NAME) OP_HEAD(NAME, 8, 8, 0, 0) uint32_t s[8], d[8]; ldw(s, in, 8); NAME(d, s); \
  for (int i = 0; i < 8; ++i) out[i] = d[i]; OP_END
OP_RECODE(sc_recode4)
OP_RECODE(sc_recode4_hi8)
OP_RECODE(sc_recode8)
OP_RECODE(sc_recode16)
// the sc_recode_w widths the kernels instantiate: the A comb (10), the fixed-base windows and the wide B comb (16, 20, 24)
#define OP_RECODE_W(WB) OP_HEAD(sc_recode_w##WB, 8, ScWin<WB>::ND, 0, 0) uint32_t s[8], d[ScWin<WB>::ND]; ldw(s, in, 8); \
  sc_recode_w<WB>(d, s); for (int i = 0; i < ScWin<WB>::ND; ++i) out[i] = d[i]; OP_END
OP_RECODE_W(10)
OP_RECODE_W(16)
OP_RECODE_W(20)
OP_RECODE_W(24)

// ---- one lane per case
constexpr int kBlock = 256;
constexpr int kMaxCases = 1 << 20;

template <class Op>
__global__ void __launch_bounds__(kBlock) probe_kernel(int n, const uint32_t* in, uint32_t* out, int arg) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (i >= n) return;
  uint32_t a[Op::IN], r[Op::OUT];
  for (int j = 0; j < Op::IN; ++j) a[j] = in[(size_t)i * Op::IN + j];
  Op::run(a, r, arg);
  for (int j = 0; j < Op::OUT; ++j) out[(size_t)i * Op::OUT + j] = r[j];
}

template <class Op>
int run_op(int where, int n, const uint32_t* in, uint32_t* out, int arg) {
  if (where == 0) {
    for (int i = 0; i < n; ++i) Op::run(in + (size_t)i * Op::IN, out + (size_t)i * Op::OUT, arg);
    return 0;
  }
  const size_t ib = (size_t)n * Op::IN * sizeof(uint32_t), ob = (size_t)n * Op::OUT * sizeof(uint32_t);
  uint32_t *din = nullptr, *dout = nullptr;
  int prev = 0;
  hipError_t e = hipGetDevice(&prev);
  if (e != hipSuccess) return (int)e;
  e = hipSetDevice(0);
  if (e != hipSuccess) return (int)e;
  e = hipMalloc((void**)&din, ib);
  if (e == hipSuccess) e = hipMalloc((void**)&dout, ob);
  if (e == hipSuccess) e = hipMemcpy(din, in, ib, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xa5, ob);
  if (e == hipSuccess) {
    probe_kernel<Op><<<dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock)>>>(n, din, dout, arg);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
  hipError_t f = din ? hipFree(din) : hipSuccess;
  if (e == hipSuccess) e = f;
  f = dout ? hipFree(dout) : hipSuccess;
  if (e == hipSuccess) e = f;
  f = hipSetDevice(prev);
  if (e == hipSuccess) e = f;
  return (int)e;
}

struct Entry {
  const char* (*name)();
  int in, out, amin, amax;
  int (*run)(int, int, const uint32_t*, uint32_t*, int);
};
#define ENTRY(NAME) {&op_##NAME::name, op_##NAME::IN, op_##NAME::OUT, op_##NAME::AMIN, op_##NAME::AMAX, &run_op<op_##NAME>}
const Entry kOps[] = {
    // the products keep these numbers (0..13): the order of at2v_fu_gen.h
    ENTRY(fu_mul), ENTRY(fu_sq), ENTRY(fu_sq2), ENTRY(fu_mul_x2), ENTRY(fu_sq_x2), ENTRY(fu_sq_sq2), ENTRY(fu_mulc),
    ENTRY(fu_sqc), ENTRY(fu_mulc_x2), ENTRY(fu_mul_n), ENTRY(fu_mul_wn), ENTRY(fu_mul_nn), ENTRY(fu_sq_sq2_n),
    ENTRY(fu_sqc_x2),
    ENTRY(fu_carry), ENTRY(fu_pcarry_even), ENTRY(fu_add), ENTRY(fu_sub), ENTRY(fu_neg), ENTRY(fu_frombytes),
    ENTRY(fu_tobytes), ENTRY(fu_iszero), ENTRY(fu_isnegative), ENTRY(fu_sqn), ENTRY(fu_sqn_x2), ENTRY(fu_invert),
    ENTRY(fu_pow22523), ENTRY(fu_pow22523_x2),
    ENTRY(gu_dbl_p2), ENTRY(gu_dbl_p3), ENTRY(gu_p3_to_cached), ENTRY(gu_add), ENTRY(gu_niels_cneg), ENTRY(gu_madd),
    ENTRY(gu_p2_is_identity), ENTRY(gu_p2_mul8_is_identity), ENTRY(gu_cofactored_eq), ENTRY(gu_frombytes),
    ENTRY(gu_frombytes_x2),
    ENTRY(sc_reduce512), ENTRY(lattice), ENTRY(sc_recode2_joint), ENTRY(sc_recode4), ENTRY(sc_recode4_hi8),
    ENTRY(sc_recode8), ENTRY(sc_recode16), ENTRY(sc_recode_w10), ENTRY(sc_recode_w16), ENTRY(sc_recode_w20),
    ENTRY(sc_recode_w24),
};
constexpr int kNumOps = (int)(sizeof(kOps) / sizeof(kOps[0]));

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int at2v_probe_count(void) { return kNumOps; }

__attribute__((visibility("default"))) int at2v_probe_info(int op, const char** name, int* in_words, int* out_words,
                                                           int* arg_min, int* arg_max) {
  if (op < 0 || op >= kNumOps || !name || !in_words || !out_words || !arg_min || !arg_max) return -1;
  *name = kOps[op].name();
  *in_words = kOps[op].in;
  *out_words = kOps[op].out;
  *arg_min = kOps[op].amin;
  *arg_max = kOps[op].amax;
  return 0;
}

__attribute__((visibility("default"))) int at2v_probe_run(int where, int op, int n, const uint32_t* in, uint32_t* out,
                                                          int arg) {
  if (op < 0 || op >= kNumOps || (where != 0 && where != 1) || n <= 0 || n > kMaxCases || !in || !out) return -1;
  if (arg < kOps[op].amin || arg > kOps[op].amax) return -1;
  return kOps[op].run(where, n, in, out, arg);
}

}  // extern "C"
