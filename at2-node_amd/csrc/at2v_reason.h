// at2v_reason.h — why a record was rejected (include/at2v.h at2v_reason): one host/device function over the helpers the
// verify routines themselves use (sc_v1_ok, enc_y_canonical, enc_small_order, gu_frombytes), so the reason and
// the verdict can never disagree about a check.
//
// The reference tells these causes apart in two places: an undecodable sender key is InvalidArgument at ingest
// (/root/reference/src/bin/server/rpc.rs:240-243, :265-269), and dalek's Signature::from_bytes refuses s >= l before
// PublicKey::verify ever evaluates the equation. The verify kernels fold all of it into one bit; this is the second,
// cheap pass over the records whose bit is 0 (at2v_reason.hip on the device, cpu_reject_reasons on the host).
#pragma once
#include "at2v_gu.h"
#include "at2v_verify.h"

namespace at2v {

enum {
  REASON_VALID = 0,
  REASON_A_DECODE = 1,
  REASON_S_RANGE = 2,
  REASON_A_POLICY = 3,
  REASON_R_POLICY = 4,
  REASON_R_ENCODING = 5,
  REASON_EQUATION = 6,
  REASON_UNKNOWN = 0xff
};

// The lowest-numbered failing check of a record whose verdict bit is 0, tested in the enum's order: A decodes (dalek
// rules), V1 (s < l; LEGACY policy: s < 2^253), (LIBSODIUM policy) A canonical and not blocklisted, R not blocklisted,
// then R is the canonical encoding of a curve point (the conditions verify_half_fu puts on R_bytes); if all of them
// hold, the equation failed, by elimination. It does not re-verify: a valid record handed in with a 0 bit gets
// REASON_EQUATION. Under POLICY_ZIP215 R is decoded by A's rules, so REASON_R_ENCODING means "R is not on the curve" only
// (a non-canonical y, or x = 0 with the sign bit, is no cause), and the equation is the cofactored one. The cheap checks
// are evaluated for every lane before the decodes, and R is decoded only by lanes
// still undecided, so a wave pays at most two square-root chains.
AT2V_HD AT2V_INLINE int reject_reason(const uint32_t Aw[8], const uint32_t Rw[8], const uint32_t Sw[8], int policy) {
  const int sodium = policy == POLICY_LIBSODIUM_1_0_18, zip = policy == POLICY_ZIP215;
  int cheap = 0;  // the first failing check after A's decode that needs no field arithmetic (0: none)
  if (!zip && !enc_y_canonical(Rw)) cheap = REASON_R_ENCODING;
  if (sodium && enc_small_order(Rw)) cheap = REASON_R_POLICY;
  if (sodium && (!enc_y_canonical(Aw) || enc_small_order(Aw))) cheap = REASON_A_POLICY;
  if (!sc_v1_ok(Sw, policy)) cheap = REASON_S_RANGE;
  int r = 0;
#pragma unroll 1
  for (int q = 0; q < 2 && r == 0; ++q) {  // A, then R: one copy of the decode's code
    uint32_t W[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) W[i] = q ? Rw[i] : Aw[i];
    gu_p3 P;
    const int ok = gu_frombytes(P, W);
    if (q == 0) r = ok ? cheap : REASON_A_DECODE;
    else r = (ok & (zip | !(fu_iszero(P.X) & (int)(Rw[7] >> 31)))) ? REASON_EQUATION : REASON_R_ENCODING;
  }
  return r;
}

// Which policies accept a record (include/at2v.h AT2V_MASK_*), given the verdict bit of a verify over it under
// POLICY_DALEK_V1_LEGACY. The three acceptance sets are nested, LIBSODIUM within DALEK_V1 within LEGACY, and V2..V6 do not
// depend on the policy: for s < l the legacy verdict IS the DALEK_V1 verdict (the same s enters the same equation), and
// the LIBSODIUM verdict is that one AND its pre-rejects. So one accepted bit and three checks without field arithmetic
// give all three verdicts. Like reject_reason it trusts the bit and does not re-verify.
enum { MASK_DALEK_V1 = 1, MASK_LIBSODIUM = 2, MASK_DALEK_V1_LEGACY = 4 };
AT2V_HD AT2V_INLINE int policy_mask(const uint32_t Aw[8], const uint32_t Rw[8], const uint32_t Sw[8], int accepted) {
  const int canon = sc_is_canonical(Sw);
  const int sodium = canon & enc_y_canonical(Aw) & !enc_small_order(Aw) & !enc_small_order(Rw);
  const int m = MASK_DALEK_V1_LEGACY | (canon ? MASK_DALEK_V1 : 0) | (sodium ? MASK_LIBSODIUM : 0);
  return accepted ? m : 0;
}

}  // namespace at2v
