"""Expected verdicts and reasons under AT2V_POLICY_ZIP215 (include/at2v.h), as Python integers, and the constructed records
no fixture holds. Nothing here comes from the library or from the oracle's verify: the four rule sets are restated on the
full-length equation (decompress, double-and-add, three doublings for the cofactored rule, identity test), which is
independent of the half-size form the kernels evaluate. Hashing is hashlib's SHA-512.

  DALEK_V1         s < l;      A decodes; R canonical and decodes;                       [s]B - [k]A - R == 0
  LIBSODIUM        DALEK_V1, and A's y canonical, A and R not on the small-order blocklist
  DALEK_V1_LEGACY  s < 2^253;  the rest as DALEK_V1 (s enters the equation unreduced)
  ZIP215           s < l;      A and R decode (y mod p, x = 0 with the sign bit accepted); [8]([s]B - [k]A - R) == 0

With R canonical, "[s]B - [k]A - R is the identity" is dalek's enc([s]B - [k]A) == R_bytes."""
import hashlib
import os

import numpy as np

import golden_io
import legacy_ref as lr
import reason_ref as rr

P, L, D = rr.P, rr.L, rr.D
SQRT_M1 = rr.SQRT_M1
DALEK, LIBSODIUM, LEGACY, ZIP215 = 0, 1, 2, 4
POLICIES = (DALEK, LIBSODIUM, LEGACY, ZIP215)
NAMES = {DALEK: "dalek", LIBSODIUM: "libsodium", LEGACY: "dalek-legacy", ZIP215: "zip215"}
IDENT = (0, 1, 1, 0)


def decompress(b: bytes):
    """dalek CompressedEdwardsY::decompress: y = LE255 mod p (no canonicity check), x = 0 with the sign bit accepted, a
    y that is not on the curve -> None. Extended coordinates (X, Y, Z, T)."""
    v = int.from_bytes(b, "little")
    sign, y = v >> 255, (v & ((1 << 255) - 1)) % P
    u, w = (y * y - 1) % P, (D * y * y + 1) % P
    x2 = u * pow(w, P - 2, P) % P
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * SQRT_M1 % P
    if (x * x - x2) % P:
        return None
    if (x & 1) != sign:
        x = (P - x) % P
    return (x, y, 1, x * y % P)


def canonical(b: bytes) -> bool:
    """b is the encoding dalek's compress would produce for the point it decodes to: y < p, not x = 0 with the sign bit"""
    v = int.from_bytes(b, "little")
    if (v & ((1 << 255) - 1)) >= P:
        return False
    pt = decompress(b)
    return not (pt is not None and pt[0] == 0 and (v >> 255))


def add(p1, p2):
    """add-2008-hwcd-3, complete on this curve"""
    X1, Y1, Z1, T1 = p1
    X2, Y2, Z2, T2 = p2
    A = (Y1 - X1) * (Y2 - X2) % P
    B = (Y1 + X1) * (Y2 + X2) % P
    C = T1 * 2 * D * T2 % P
    DD = Z1 * 2 * Z2 % P
    E, F, G, H = B - A, DD - C, DD + C, B + A
    return (E * F % P, G * H % P, F * G % P, E * H % P)


def dbl(p):
    return add(p, p)


def neg(p):
    return ((-p[0]) % P, p[1], p[2], (-p[3]) % P)


def mul(k: int, p):
    """[k]p by double-and-add, k >= 0 of any size"""
    q = IDENT
    for bit in bin(k)[2:]:
        q = dbl(q)
        if bit == "1":
            q = add(q, p)
    return q


def is_identity(p) -> bool:
    return p[0] % P == 0 and (p[1] - p[2]) % P == 0


def same(p, q) -> bool:
    return (p[0] * q[2] - q[0] * p[2]) % P == 0 and (p[1] * q[2] - q[1] * p[2]) % P == 0


def enc(p) -> bytes:
    zi = pow(p[2], P - 2, P)
    x, y = p[0] * zi % P, p[1] * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


BASE = decompress((4 * pow(5, P - 2, P) % P).to_bytes(32, "little"))
_BASE_POW = [BASE]  # [2^i]B: [s]B is then additions only
for _ in range(255):
    _BASE_POW.append(dbl(_BASE_POW[-1]))


def mul_base(s: int):
    q = IDENT
    for i in range(s.bit_length()):
        if (s >> i) & 1:
            q = add(q, _BASE_POW[i])
    return q


def challenge(r_enc: bytes, pk: bytes, msg: bytes) -> int:
    return int.from_bytes(hashlib.sha512(r_enc + pk + msg).digest(), "little") % L


def residual(pk: bytes, sig: bytes, msg: bytes):
    """[s]B - [k]A - R with s as the integer it is, or None when A or R does not decode"""
    A, R = decompress(pk), decompress(sig[:32])
    if A is None or R is None:
        return None
    s = int.from_bytes(sig[32:], "little")
    k = challenge(sig[:32], pk, msg)
    return add(add(mul_base(s), neg(mul(k, A))), neg(R))


def verify(pk: bytes, sig: bytes, msg: bytes, policy: int) -> bool:
    assert policy in POLICIES
    s = int.from_bytes(sig[32:], "little")
    if (sig[63] & 0xE0) if policy == LEGACY else (s >= L):
        return False
    if policy == LIBSODIUM:
        if rr.y_of(pk) >= P or rr.y_of(pk) in rr.BLOCKLIST_Y or rr.y_of(sig[:32]) in rr.BLOCKLIST_Y:
            return False
    if policy != ZIP215 and not canonical(sig[:32]):
        return False
    v = residual(pk, sig, msg)
    if v is None:
        return False
    if policy == ZIP215:
        v = dbl(dbl(dbl(v)))
    return is_identity(v)


def verify_all(pk: bytes, sig: bytes, msg: bytes):
    """the verdicts under (DALEK, LIBSODIUM, LEGACY, ZIP215) from one evaluation of the residual"""
    s = int.from_bytes(sig[32:], "little")
    v = residual(pk, sig, msg)
    if v is None:
        return (False, False, False, False)
    plain = is_identity(v) and canonical(sig[:32])
    sodium = not (rr.y_of(pk) >= P or rr.y_of(pk) in rr.BLOCKLIST_Y or rr.y_of(sig[:32]) in rr.BLOCKLIST_Y)
    return (plain and s < L, plain and s < L and sodium, plain and not (sig[63] & 0xE0),
            s < L and is_identity(dbl(dbl(dbl(v)))))


def expected_set(g, idx=None) -> np.ndarray:
    """bool[len(idx), 4]: verify_all over the records idx (default: all) of a fixture set"""
    idx = range(g.n) if idx is None else idx
    out = np.array([verify_all(g.pk[i].tobytes(), g.sig[i].tobytes(), g.message(i)) for i in idx], bool).reshape(-1, 4)
    out.setflags(write=False)
    return out


def reason(pk: bytes, sig: bytes, valid: bool, policy: int = ZIP215) -> int:
    """the lowest-numbered failing check in the header's order. Under ZIP215 R_ENCODING means "R is not on the curve"
    only and reasons 3 and 4 never occur; the other policies are reason_ref's / legacy_ref's."""
    if policy in (DALEK, LIBSODIUM):
        return rr.reason(pk, sig, valid, policy)
    if valid:
        return rr.VALID
    if decompress(pk) is None:
        return rr.A_DECODE
    if policy == LEGACY:
        return lr.reason_legacy(pk, sig, valid)
    if int.from_bytes(sig[32:], "little") >= L:
        return rr.S_RANGE
    return rr.R_ENCODING if decompress(sig[:32]) is None else rr.EQUATION


def reasons(pk: np.ndarray, sig: np.ndarray, valid, policy: int = ZIP215) -> np.ndarray:
    pk = np.ascontiguousarray(pk, np.uint8).reshape(-1, 32)
    sig = np.ascontiguousarray(sig, np.uint8).reshape(-1, 64)
    return np.array([reason(pk[i].tobytes(), sig[i].tobytes(), bool(valid[i]), policy) for i in range(len(pk))],
                    np.uint8)


# ---- the 8-torsion and its 14 encodings

def torsion_generator():
    """a point of order 8: (x, y8) with reason_ref's y8"""
    t = decompress(rr.enc_y(rr.Y8))
    assert not is_identity(mul(4, t)) and is_identity(mul(8, t))
    return t


T8 = torsion_generator()
TORSION = [mul(j, T8) for j in range(8)]  # [j]T8: order 1, 8, 4, 8, 2, 8, 4, 8


def torsion_encodings():
    """every 32-byte string that decompress maps to a point of the 8-torsion: the 8 canonical encodings and the 6
    non-canonical ones (y = 1 and y = p - 1 with the sign bit set: x = 0; y = p and y = p + 1 with either sign)"""
    out = []
    for t in TORSION:
        y = int.from_bytes(enc(t), "little") & ((1 << 255) - 1)
        for yy in (y, y + P):
            if yy >= 1 << 255:
                continue
            for sign in (0, 1):
                e = rr.enc_y(yy, sign)
                pt = decompress(e)
                if pt is not None and same(pt, t) and e not in out:
                    out.append(e)
    assert len(out) == 14 and sum(canonical(e) for e in out) == 8
    return out


class Case:
    """one constructed record; verdicts and reasons under (DALEK, LIBSODIUM, LEGACY, ZIP215), from verify_all / reason"""

    def __init__(self, name, pk, sig, msg):
        self.name, self.pk, self.sig, self.msg = name, pk, sig, msg
        self.verdicts = tuple(int(v) for v in verify_all(pk, sig, msg))
        self.reasons = tuple(reason(pk, sig, bool(v), p) for v, p in zip(self.verdicts, POLICIES))

    @property
    def zip215(self):
        return bool(self.verdicts[3])

    @property
    def dalek(self):
        return bool(self.verdicts[0])


MATRIX_MSG = b"Zcash"


def small_order_matrix():
    """the 196 ZIP-215 small-order cases: every pair of the 14 torsion encodings as A and as R, S = 0, one message.
    [8](0 - [k]A - R) is the identity whatever k is, so ZIP215 accepts all of them."""
    encs = torsion_encodings()
    return [Case(f"torsion A#{i} R#{j}", a, r + bytes(32), MATRIX_MSG) for i, a in enumerate(encs)
            for j, r in enumerate(encs)]


SECRET_A = int.from_bytes(hashlib.sha512(b"zip215 test secret a").digest(), "little") % L
SECRET_R = int.from_bytes(hashlib.sha512(b"zip215 test nonce r").digest(), "little") % L
SHIFT_MSG = b"torsion-shifted signature"
MIXED = ((1, 3), (2, 5), (7, 4))


def shifted(ja: int, jr: int, msg: bytes = SHIFT_MSG, a: int = SECRET_A, r: int = SECRET_R):
    """(pk, sig) with A = [a]B + [ja]T8, R = [r]B + [jr]T8, s = r + k a mod l, k hashed over the shifted bytes"""
    pk = enc(add(mul_base(a), TORSION[ja]))
    r_enc = enc(add(mul_base(r), TORSION[jr]))
    s = (r + challenge(r_enc, pk, msg) * a) % L
    return pk, r_enc + s.to_bytes(32, "little")


def shifted_cases():
    pairs = [(0, j) for j in range(8)] + [(j, 0) for j in range(1, 8)] + list(MIXED)
    return [Case(f"shift T_A=[{ja}]T8 T_R=[{jr}]T8", *shifted(ja, jr), SHIFT_MSG) for ja, jr in pairs], pairs


def dalek_accepts_shift(ja: int, jr: int) -> bool:
    """[k]T_A + T_R == 0, the condition under which the cofactorless equation still holds"""
    pk, sig = shifted(ja, jr)
    k = challenge(sig[:32], pk, SHIFT_MSG)
    return (k * ja + jr) % 8 == 0


def edge_cases():
    """the negative and boundary records"""
    out = []
    pk, sig = shifted(3, 5)  # both shifts of order 8
    out.append(Case("shifted, one bit of M flipped", pk, sig, bytes([SHIFT_MSG[0] ^ 1]) + SHIFT_MSG[1:]))
    s = int.from_bytes(sig[32:], "little")
    assert s + L < 2 ** 253
    out.append(Case("shifted, S + l", pk, sig[:32] + (s + L).to_bytes(32, "little"), SHIFT_MSG))
    yoff = rr.off_curve_y()
    out.append(Case("R off the curve", pk, rr.enc_y(yoff) + sig[32:], SHIFT_MSG))
    out.append(Case("A off the curve", rr.enc_y(yoff), sig, SHIFT_MSG))
    # R_bytes non-canonical, decoding to the right point: R' = [s]B - [k]A is the identity when s = k a
    pk0 = enc(mul_base(SECRET_A))
    for name, r_enc in (("non-canonical R (y = p + 1) that decodes to R'", rr.enc_y(P + 1)),
                        ("R = (0, 1) with the sign bit set, matching S", rr.enc_y(1, 1))):
        s = challenge(r_enc, pk0, SHIFT_MSG) * SECRET_A % L
        out.append(Case(name, pk0, r_enc + s.to_bytes(32, "little"), SHIFT_MSG))
    pk, sig = shifted(0, 0)
    out.append(Case("plain valid record", pk, sig, SHIFT_MSG))
    return out


def constructed(matrix: bool = True):
    """the matrix (optional), the torsion-shifted signatures, the negative cases"""
    return (small_order_matrix() if matrix else []) + shifted_cases()[0] + edge_cases()


def pack(cases):
    """-> pk (n, 32), sig (n, 64), msg, off as the verify calls take them"""
    pk = np.frombuffer(b"".join(c.pk for c in cases), np.uint8).reshape(-1, 32).copy()
    sig = np.frombuffer(b"".join(c.sig for c in cases), np.uint8).reshape(-1, 64).copy()
    msg = np.frombuffer(b"".join(c.msg for c in cases), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(c.msg) for c in cases])]).astype(np.uint32)
    return pk, sig, msg, off


def transfer_cases():
    """signed transfers (wire BYTES: M = u64le(32) || recipient || u64le(amount)) whose sender is torsion-shifted:
    -> sender (n, 32), sig (n, 64), recipient (n, 32), amount u64[n], and bool[n, 4] expected"""
    recipient = enc(mul_base(12345))
    snd, sig, amt, want = [], [], [], []
    for q, (ja, jr) in enumerate([(0, 0), (1, 0), (4, 0), (0, 3), (5, 2), (3, 7)]):
        amount = 1000 + q
        m = (32).to_bytes(8, "little") + recipient + amount.to_bytes(8, "little")
        pk, sg = shifted(ja, jr, m)
        if q == 5:
            amount += 1  # signed for another amount
            m = (32).to_bytes(8, "little") + recipient + amount.to_bytes(8, "little")
        snd.append(pk), sig.append(sg), amt.append(amount), want.append(verify_all(pk, sg, m))
    n = len(snd)
    return (np.frombuffer(b"".join(snd), np.uint8).reshape(n, 32).copy(),
            np.frombuffer(b"".join(sig), np.uint8).reshape(n, 64).copy(),
            np.frombuffer(recipient * n, np.uint8).reshape(n, 32).copy(), np.array(amt, np.uint64),
            np.array(want, bool))


def stored(name: str, n: int) -> np.ndarray:
    """the ZIP215 column of a fixture set as this module computed it (tests/golden/zip215_<name>.npy, packed bits;
    tests/test_zip215_cpu.py re-derives it)"""
    bits = np.load(os.path.join(golden_io.GOLDEN_DIR, f"zip215_{name}.npy"))
    out = np.unpackbits(bits, bitorder="little")[:n].astype(bool)
    out.setflags(write=False)
    return out


def tile(cases, n):
    """n records cycling through the cases (their order kept)"""
    return [cases[i % len(cases)] for i in range(n)]
