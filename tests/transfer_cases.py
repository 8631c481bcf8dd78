"""Inputs and expected bits of the transfers tests (tests/test_transfers_cpu.py, tests/test_gpu_transfers.py): the fields
of SendAssetRequest taken from the golden sets, the messages rebuilt from them in plain numpy (never by the library), and
expected verdicts from the golden verdicts and the oracle. Each set is computed once per process and handed out
read-only."""
import functools
from dataclasses import dataclass

import numpy as np

import golden_io
import oracle_py

WIRE_BYTES, WIRE_ARRAY = 0, 1
POLICIES = {"dalek": 0, "libsodium": 1}


@dataclass(frozen=True)
class Transfers:
    sender: np.ndarray     # (n, 32) u8
    sig: np.ndarray        # (n, 64) u8
    recipient: np.ndarray  # (n, 32) u8
    amount: np.ndarray     # (n,) u64
    wire: int
    want: dict             # policy name -> bool[n]
    mutated: np.ndarray    # bool[n]: records changed after signing

    @property
    def n(self):
        return len(self.amount)

    def head(self, n):
        return Transfers(self.sender[:n], self.sig[:n], self.recipient[:n], self.amount[:n], self.wire,
                         {k: v[:n] for k, v in self.want.items()}, self.mutated[:n])


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def build_messages(recipient, amount, wire):
    """bincode(ThinTransaction{recipient, amount}) per record -> (msg u8[], off u32[n + 1])"""
    n = len(amount)
    amt = np.ascontiguousarray(amount, "<u8").view(np.uint8).reshape(n, 8)
    parts = [recipient.reshape(n, 32), amt]
    if wire == WIRE_BYTES:
        parts.insert(0, np.tile(np.frombuffer((32).to_bytes(8, "little"), np.uint8), (n, 1)))
    m = np.concatenate(parts, axis=1)
    L = m.shape[1]
    assert L == (48 if wire == WIRE_BYTES else 40)
    return np.ascontiguousarray(m).reshape(-1), (np.arange(n + 1, dtype=np.uint64) * L).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def cfg1():
    """at2_cfg1 as fields: 4,096 records, 48-byte messages u64le(32) || recipient || u64le(amount)"""
    g = golden_io.load("at2_cfg1")
    assert g.n == 4096 and np.array_equal(g.off, np.arange(4097, dtype=np.uint32) * 48)
    m = g.msg.reshape(g.n, 48)
    assert (m[:, :8] == np.frombuffer((32).to_bytes(8, "little"), np.uint8)).all()
    recipient = np.ascontiguousarray(m[:, 8:40])
    amount = np.ascontiguousarray(m[:, 40:48]).view("<u8").reshape(-1).astype(np.uint64)
    assert len(np.unique(g.pk, axis=0)) == 64 and len(np.unique(recipient, axis=0)) == 64
    assert amount.min() >= 1 and amount.max() <= 1000
    assert g.dalek.all() and g.sodium.all()
    msg, off = build_messages(recipient, amount, WIRE_BYTES)
    assert np.array_equal(msg, g.msg) and np.array_equal(off, g.off)
    t = Transfers(g.pk.copy(), g.sig.copy(), recipient, amount, WIRE_BYTES,
                  {"dalek": g.dalek.copy(), "libsodium": g.sodium.copy()}, np.zeros(g.n, bool))
    _freeze(t.sender, t.sig, t.recipient, t.amount, t.mutated, *t.want.values())
    return t


@functools.lru_cache(maxsize=None)
def cfg1_mutated():
    """at2_cfg1 with every 10th record changed after signing, cycling over: amount XOR 1, one recipient byte flipped, one
    signature bit flipped. Expected: the golden verdicts for the untouched records, the oracle over the rebuilt messages
    for the mutated ones (the oracle must reject each of them: a condition on the reference, asserted here)."""
    base = cfg1()
    sender, sig = base.sender.copy(), base.sig.copy()
    recipient, amount = base.recipient.copy(), base.amount.copy()
    idx = np.arange(0, base.n, 10)
    for k, i in enumerate(idx):
        if k % 3 == 0:
            amount[i] ^= np.uint64(1)
        elif k % 3 == 1:
            recipient[i, (7 * k) % 32] ^= 0x10
        else:
            sig[i, (5 * k) % 64] ^= np.uint8(1 << (k % 8))
    mutated = np.zeros(base.n, bool)
    mutated[idx] = True
    msg, off = build_messages(recipient[idx], amount[idx], WIRE_BYTES)
    o = oracle_py.Oracle()
    want = {}
    for name, pol in POLICIES.items():
        w = base.want[name].copy()
        sub = o.verify_batch(sender[idx], sig[idx], msg, off, policy=pol)
        assert not sub.any(), "the oracle accepts a mutated record"
        w[idx] = sub
        want[name] = w
    t = Transfers(sender, sig, recipient, amount, WIRE_BYTES, want, mutated)
    _freeze(sender, sig, recipient, amount, mutated, *want.values())
    return t


@functools.lru_cache(maxsize=None)
def array_wire(n=256):
    """n records signed by the oracle (16 keys from fixed seeds) over the 40-byte message of AT2V_WIRE_ARRAY; recipients
    from the at2_cfg1 pool, amounts spread over the u64 range with 0, 1 and 2^64 - 1 among them"""
    o = oracle_py.Oracle()
    base = cfg1()
    rng = np.random.default_rng(0xA77A)
    seeds = rng.integers(0, 256, (16, 32), dtype=np.uint8)
    pks = [o.public_key(s.tobytes()) for s in seeds]
    recipient = np.ascontiguousarray(base.recipient[rng.integers(0, base.n, n)])
    amount = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    amount[:3] = [0, 1, 0xFFFFFFFFFFFFFFFF]
    msg, off = build_messages(recipient, amount, WIRE_ARRAY)
    sender = np.zeros((n, 32), np.uint8)
    sig = np.zeros((n, 64), np.uint8)
    for i in range(n):
        k = i % len(seeds)
        sender[i] = np.frombuffer(pks[k], np.uint8)
        sig[i] = np.frombuffer(o.sign(seeds[k].tobytes(), msg[off[i]:off[i + 1]].tobytes()), np.uint8)
    want = {name: o.verify_batch(sender, sig, msg, off, policy=pol) for name, pol in POLICIES.items()}
    assert want["dalek"].all() and want["libsodium"].all()
    # the same signatures over the 48-byte form: the oracle rejects them all (asked of the reference, not the library)
    msg48, off48 = build_messages(recipient, amount, WIRE_BYTES)
    assert not o.verify_batch(sender, sig, msg48, off48).any()
    t = Transfers(sender, sig, recipient, amount, WIRE_ARRAY, want, np.zeros(n, bool))
    _freeze(sender, sig, recipient, amount, *want.values())
    return t


@functools.lru_cache(maxsize=None)
def recipient_mix():
    """at2_cfg1's first 1,218 records with every second recipient replaced by a pk of the `edge` set (609 keys: off-curve,
    small-order and non-canonical encodings beside good ones). The records are no longer validly signed; expected
    verdicts come from the oracle over the rebuilt messages, expected recipient bits from Oracle.decompress_ok."""
    base = cfg1()
    e = golden_io.load("edge")
    assert e.n == 609
    n = 2 * e.n
    recipient = base.recipient[:n].copy()
    recipient[1::2] = e.pk
    o = oracle_py.Oracle()
    rok = np.array([o.decompress_ok(recipient[i].tobytes()) for i in range(n)], dtype=bool)
    assert 0 < rok.sum() < n
    msg, off = build_messages(recipient, base.amount[:n], WIRE_BYTES)
    want = {name: o.verify_batch(base.sender[:n], base.sig[:n], msg, off, policy=pol) for name, pol in POLICIES.items()}
    t = Transfers(base.sender[:n].copy(), base.sig[:n].copy(), recipient, base.amount[:n].copy(), WIRE_BYTES, want,
                  np.zeros(n, bool))
    _freeze(t.sender, t.sig, t.recipient, t.amount, rok, *want.values())
    return t, rok


@functools.lru_cache(maxsize=None)
def bad_senders():
    """(pk, sig) of the whole `edge` set and of classes 3-7 of `adversarial`, as transfers: recipients from the at2_cfg1
    pool, the amount is the record index. Expected: the oracle over the rebuilt messages, both policies."""
    e, a = golden_io.load("edge"), golden_io.load("adversarial")
    keep = (a.cls >= 3) & (a.cls <= 7)
    sender = np.ascontiguousarray(np.concatenate([e.pk, a.pk[keep]]))
    sig = np.ascontiguousarray(np.concatenate([e.sig, a.sig[keep]]))
    n = len(sender)
    base = cfg1()
    recipient = np.ascontiguousarray(base.recipient[np.arange(n) % base.n])
    amount = np.arange(n, dtype=np.uint64)
    msg, off = build_messages(recipient, amount, WIRE_BYTES)
    o = oracle_py.Oracle()
    want = {name: o.verify_batch(sender, sig, msg, off, policy=pol) for name, pol in POLICIES.items()}
    t = Transfers(sender, sig, recipient, amount, WIRE_BYTES, want, np.zeros(n, bool))
    _freeze(sender, sig, recipient, amount, *want.values())
    return t


@functools.lru_cache(maxsize=None)
def cfg1_mutated_recipient_ok():
    """Oracle.decompress_ok per recipient of cfg1_mutated() (a flipped recipient byte may leave the curve)"""
    t = cfg1_mutated()
    o = oracle_py.Oracle()
    rok = np.array([o.decompress_ok(t.recipient[i].tobytes()) for i in range(t.n)], dtype=bool)
    rok.setflags(write=False)
    return rok
