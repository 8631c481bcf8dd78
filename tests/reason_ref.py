"""Expected reject reasons (include/at2v.h at2v_reason) from Python integers alone: the reference of the reasons tests.

It shares no code with the product or the oracle: point decoding by the sqrt-ratio rule of SURVEY Appendix A V2
(curve25519-dalek CompressedEdwardsY::decompress), s < l, y < p, and libsodium 1.0.18's seven blocklisted y values.
The caller supplies the verdict (the reason of a rejected record is a function of A, R, S, the policy and that bit)."""
import numpy as np

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
D = (-121665 * pow(121666, P - 2, P)) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)


def _add(a, b):
    """affine twisted Edwards addition (a = -1), complete on this curve"""
    (x1, y1), (x2, y2) = a, b
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + t, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - t, P - 2, P) % P)


def _order8_y() -> int:
    """y of a point of order 8: [l]T for curve points T until the result has order 8. The four such points are
    (+-x, +-y8), so their encodings' y values are y8 and p - y8."""
    y = 2
    while True:
        u, w = (y * y - 1) % P, (D * y * y + 1) % P
        xx = u * pow(w, P - 2, P) % P
        x = pow(xx, (P + 3) // 8, P)
        if x * x % P != xx:
            x = x * SQRT_M1 % P
        if x * x % P == xx:
            q, t, k = (0, 1), (x, y), L
            while k:  # q = [l]T
                if k & 1:
                    q = _add(q, t)
                t, k = _add(t, t), k >> 1
            q2 = _add(q, q)
            q4 = _add(q2, q2)
            if q4 != (0, 1) and _add(q4, q4) == (0, 1):
                return q[1]
        y += 1


# libsodium 1.0.18's small-order blocklist, as y values (sign bit masked): 0, 1, -1, p, p + 1, y8, -y8
Y8 = _order8_y()
BLOCKLIST_Y = frozenset({0, 1, P - 1, P, P + 1, Y8, P - Y8})

VALID, A_DECODE, S_RANGE, A_POLICY, R_POLICY, R_ENCODING, EQUATION = range(7)
UNKNOWN = 0xFF
DALEK, LIBSODIUM = 0, 1


def decode(enc: bytes):
    """dalek decompress of a 32-byte encoding -> (ok, x): y is taken mod p (no canonicity check); (ok, x) from
    sqrt_ratio_i(y^2 - 1, d y^2 + 1); the sign bit negates x (also x = 0, which stays 0)."""
    v = int.from_bytes(enc, "little")
    sign, y = v >> 255, (v & (2 ** 255 - 1)) % P
    u, w = (y * y - 1) % P, (D * y * y + 1) % P
    x = (u * pow(w, 3, P) * pow(u * pow(w, 7, P), (P - 5) // 8, P)) % P
    chk = (w * x * x) % P
    if chk == u:
        pass
    elif chk == (-u) % P:
        x = (x * SQRT_M1) % P
    else:
        return False, 0
    if x & 1:
        x = P - x
    if sign:
        x = (P - x) % P
    return True, x


def y_of(enc: bytes) -> int:
    return int.from_bytes(enc, "little") & (2 ** 255 - 1)


def reason(pk: bytes, sig: bytes, valid: bool, policy: int = DALEK) -> int:
    """the lowest-numbered failing check, in the header's order; 0 for a record whose verdict bit is set"""
    if valid:
        return VALID
    r_enc, s = sig[:32], int.from_bytes(sig[32:], "little")
    if not decode(pk)[0]:
        return A_DECODE
    if s >= L:
        return S_RANGE
    if policy == LIBSODIUM:
        if y_of(pk) >= P or y_of(pk) in BLOCKLIST_Y:
            return A_POLICY
        if y_of(r_enc) in BLOCKLIST_Y:
            return R_POLICY
    ok, x = decode(r_enc)
    if y_of(r_enc) >= P or not ok or (x == 0 and r_enc[31] >> 7):
        return R_ENCODING
    return EQUATION


def reasons(pk: np.ndarray, sig: np.ndarray, valid, policy: int = DALEK) -> np.ndarray:
    pk = np.ascontiguousarray(pk, np.uint8).reshape(-1, 32)
    sig = np.ascontiguousarray(sig, np.uint8).reshape(-1, 64)
    return np.array([reason(pk[i].tobytes(), sig[i].tobytes(), bool(valid[i]), policy) for i in range(len(pk))],
                    np.uint8)


def counts(r: np.ndarray) -> dict:
    k, c = np.unique(r, return_counts=True)
    return {int(a): int(b) for a, b in zip(k, c)}


def words_of(valid) -> np.ndarray:
    """bool[n] -> the verify calls' verdict words (bit i % 32 of word i / 32, pad bits 0)"""
    b = np.packbits(np.asarray(valid, bool).astype(np.uint8), bitorder="little")
    return np.concatenate([b, np.zeros((-len(b)) % 4, np.uint8)]).view("<u4").copy()


def enc_y(y: int, sign: int = 0) -> bytes:
    return (y | (sign << 255)).to_bytes(32, "little")


def off_curve_y() -> int:
    """the smallest y >= 2 that is no curve point's"""
    y = 2
    while decode(enc_y(y))[0]:
        y += 1
    return y


def constructed(pk_valid: bytes, sig_valid: bytes):
    """From one valid record: the cases no fixture holds (reason 4: wherever a fixture's R is blocklisted, its A is too)
    and the priority cases. -> list of (name, pk, sig, expected under dalek, expected under libsodium). Every record is
    invalid under both policies: a changed R or S breaks the equation's hash, a changed A the key."""
    s_bad = (L + 5).to_bytes(32, "little")
    r_ok, s_ok = sig_valid[:32], sig_valid[32:]
    yoff = off_curve_y()
    out = []
    for y in sorted(BLOCKLIST_Y):
        for sign in (0, 1):
            r = enc_y(y, sign)
            ok, x = decode(r)
            assert ok  # every blocklisted y is a curve point's (mod p)
            d = R_ENCODING if (y >= P or (x == 0 and sign)) else EQUATION
            out.append((f"R=blocklist y={y % P if y >= P else y:#x}{'+p' if y >= P else ''} sign={sign}", pk_valid,
                        r + s_ok, d, R_POLICY))
    out.append(("A off-curve and s >= l", enc_y(yoff), r_ok + s_bad, A_DECODE, A_DECODE))
    out.append(("s >= l and R non-canonical", pk_valid, enc_y(P + 2) + s_bad, S_RANGE, S_RANGE))
    out.append(("A blocklisted and R blocklisted", enc_y(1), enc_y(Y8) + s_ok, EQUATION, A_POLICY))
    out.append(("R canonical y, not on the curve", pk_valid, enc_y(yoff) + s_ok, R_ENCODING, R_ENCODING))
    k = next(k for k in range(2, 19) if decode(enc_y(P + k))[0])  # p + k < 2^255, and k is a curve point's y
    out.append(("A non-canonical y (decodes mod p)", enc_y(P + k), sig_valid, EQUATION, A_POLICY))
    out.append(("one bit of S flipped", pk_valid, r_ok + bytes([s_ok[0] ^ 1]) + s_ok[1:], EQUATION, EQUATION))
    return out
