"""Expected verdicts, reasons and policy masks under AT2V_POLICY_DALEK_V1_LEGACY (include/at2v.h), and the constructed
records no fixture holds. Nothing here comes from the library: the rules are Python integers over tests/reason_ref.py, the
verdicts are the fixtures' stored columns (OpenSSL, libsodium) and the oracle's (tests/oracle_py.py).

The legacy rule: V1 is "reject iff S[31] & 0xE0" (s >= 2^253), and s is then used as the integer it is. k is hashed over
R, A and M, not S, and [s]B = [s mod l]B, so the legacy verdict of (A, R || S, M) with the top bits clear is the DALEK_V1
verdict of (A, R || (S mod l), M); 2^253 < 2 l makes "mod l" at most one subtraction."""
import struct

import numpy as np

import reason_ref as rr

L = rr.L
LEGACY = 2
MASK_DALEK_V1, MASK_LIBSODIUM, MASK_DALEK_V1_LEGACY = 1, 2, 4


def s_of(sig: bytes) -> int:
    return int.from_bytes(sig[32:64], "little")


def with_s(sig: bytes, s: int) -> bytes:
    return sig[:32] + s.to_bytes(32, "little")


def legacy_expected(oracle, pk: bytes, sig: bytes, msg: bytes, stored_dalek=None) -> bool:
    """stored_dalek: the fixture's verdict_dalek of this record (None for a record no fixture holds: the oracle's)"""
    if sig[63] & 0xE0:
        return False
    s = s_of(sig)
    if s < L:
        return bool(oracle.verify(pk, sig, msg, rr.DALEK) if stored_dalek is None else stored_dalek)
    return bool(oracle.verify(pk, with_s(sig, s - L), msg, rr.DALEK))


def legacy_expected_set(oracle, g) -> np.ndarray:
    out = np.array([legacy_expected(oracle, g.pk[i].tobytes(), g.sig[i].tobytes(), g.message(i), g.dalek[i])
                    for i in range(g.n)], bool)
    out.setflags(write=False)
    return out


def mask_expected(pk: bytes, sig: bytes, legacy_valid: bool) -> int:
    if not legacy_valid:
        return 0
    m = MASK_DALEK_V1_LEGACY
    if s_of(sig) < L:
        m |= MASK_DALEK_V1
        if rr.y_of(pk) < rr.P and rr.y_of(pk) not in rr.BLOCKLIST_Y and rr.y_of(sig[:32]) not in rr.BLOCKLIST_Y:
            m |= MASK_LIBSODIUM
    return m


def masks_expected(pk: np.ndarray, sig: np.ndarray, legacy_valid) -> np.ndarray:
    pk = np.ascontiguousarray(pk, np.uint8).reshape(-1, 32)
    sig = np.ascontiguousarray(sig, np.uint8).reshape(-1, 64)
    return np.array([mask_expected(pk[i].tobytes(), sig[i].tobytes(), bool(legacy_valid[i])) for i in range(len(pk))],
                    np.uint8)


def reason_legacy(pk: bytes, sig: bytes, valid: bool) -> int:
    """reason_ref.reason with V1 replaced: S_RANGE means S[31] & 0xE0; reasons 3 and 4 never occur"""
    if valid:
        return rr.VALID
    if not rr.decode(pk)[0]:
        return rr.A_DECODE
    if sig[63] & 0xE0:
        return rr.S_RANGE
    return rr.reason(pk, with_s(sig, 0), False, rr.DALEK)  # s = 0 passes V1: the checks on R, else the equation


def reasons_legacy(pk: np.ndarray, sig: np.ndarray, valid) -> np.ndarray:
    pk = np.ascontiguousarray(pk, np.uint8).reshape(-1, 32)
    sig = np.ascontiguousarray(sig, np.uint8).reshape(-1, 64)
    return np.array([reason_legacy(pk[i].tobytes(), sig[i].tobytes(), bool(valid[i])) for i in range(len(pk))], np.uint8)


def in_class(sig: bytes) -> bool:
    """l <= s < 2^253: the records whose verdict depends on the rule"""
    return L <= s_of(sig) < 2 ** 253


class Case:
    """one constructed record and what the issue states about it: verdicts and reasons under (DALEK, LIBSODIUM, LEGACY)
    and the mask"""

    def __init__(self, name, pk, sig, msg, verdicts, reasons, mask):
        self.name, self.pk, self.sig, self.msg = name, pk, sig, msg
        self.verdicts, self.reasons, self.mask = verdicts, reasons, mask


def constructed(oracle, g):
    """g: the at2_cfg1 fixture. A = enc(y = 1) is the identity, so [k]A = 0 and R = enc([s]B) verifies for any s the
    scalar rule lets through; oracle.scalarmult_base takes unreduced scalars."""
    ident = rr.enc_y(1)
    m = b"legacy-scalar policy"
    V, A, S, AP, E = rr.VALID, rr.A_DECODE, rr.S_RANGE, rr.A_POLICY, rr.EQUATION
    out = []
    for s in (L, L + 1, 2 ** 253 - 1):
        r = oracle.scalarmult_base(s.to_bytes(32, "little"))
        out.append(Case(f"identity A, s={s:#x}", ident, r + s.to_bytes(32, "little"), m, (0, 0, 1), (S, S, V), 4))
        out.append(Case(f"identity A, s={s:#x} - l", ident, r + (s - L).to_bytes(32, "little"), m, (1, 0, 1),
                        (V, AP, V), 5))
    s = 2 ** 253
    r = oracle.scalarmult_base(s.to_bytes(32, "little"))
    out.append(Case("identity A, s=2^253", ident, r + s.to_bytes(32, "little"), m, (0, 0, 0), (S, S, S), 0))
    i = next(i for i in range(g.n) if g.dalek[i] and g.sodium[i] and s_of(g.sig[i].tobytes()) + L < 2 ** 253)
    pk, sig, msg = g.pk[i].tobytes(), g.sig[i].tobytes(), g.message(i)
    s = s_of(sig)
    out.append(Case("at2_cfg1 record", pk, sig, msg, (1, 1, 1), (V, V, V), 7))
    out.append(Case("at2_cfg1 record, s + l", pk, with_s(sig, s + L), msg, (0, 0, 1), (S, S, V), 4))
    out.append(Case("at2_cfg1 record, s + 2l", pk, with_s(sig, s + 2 * L), msg, (0, 0, 0), (S, S, S), 0))
    flipped = bytes([msg[0] ^ 1]) + msg[1:]
    out.append(Case("at2_cfg1 record, one bit of M flipped", pk, sig, flipped, (0, 0, 0), (E, E, E), 0))
    # for the GPU shapes: a wave must also hold an undecodable A
    out.append(Case("A off-curve", rr.enc_y(rr.off_curve_y()), sig, msg, (0, 0, 0), (A, A, A), 0))
    return out


def transfer_pair(oracle):
    """one signed transfer (wire BYTES: M = u64le(32) || recipient || u64le(amount)) and the same with s + l"""
    seed = bytes(range(32))
    sender, recipient, amount = oracle.public_key(seed), oracle.public_key(bytes(range(1, 33))), 77
    sig = oracle.sign(seed, (32).to_bytes(8, "little") + recipient + amount.to_bytes(8, "little"))
    s = s_of(sig)
    assert s + L < 2 ** 253
    return (np.frombuffer(sender * 2, np.uint8).reshape(2, 32),
            np.frombuffer(sig + with_s(sig, s + L), np.uint8).reshape(2, 64),
            np.frombuffer(recipient * 2, np.uint8).reshape(2, 32), np.array([amount, amount], np.uint64))


def pack(cases):
    """-> pk (n, 32), sig (n, 64), msg, off as the verify calls take them"""
    pk = np.frombuffer(b"".join(c.pk for c in cases), np.uint8).reshape(-1, 32).copy()
    sig = np.frombuffer(b"".join(c.sig for c in cases), np.uint8).reshape(-1, 64).copy()
    msg = np.frombuffer(b"".join(c.msg for c in cases), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(c.msg) for c in cases])]).astype(np.uint32)
    return pk, sig, msg, off


def tile(cases, n):
    """n records cycling through the cases (their order kept: one wave of 64 holds every kind)"""
    return [cases[i % len(cases)] for i in range(n)]


def write_fixture(path, pk, sig, msg, off):
    """the tests/golden/*.bin layout (tests/golden/README.md) with empty verdict columns: what the host programs read"""
    n = len(pk)
    with open(path, "wb") as f:
        f.write(struct.pack("<4I", 0x56325441, 1, n, len(msg)))
        f.write(np.ascontiguousarray(pk, np.uint8).tobytes() + np.ascontiguousarray(sig, np.uint8).tobytes())
        f.write(np.ascontiguousarray(off, "<u4").tobytes() + np.ascontiguousarray(msg, np.uint8).tobytes())
        f.write(bytes(3 * n))
