"""CPU: AT2V_POLICY_ZIP215 (the cofactored rule) through the C ABI without a device: at2v_verify_one_policy / _reason, a CPU
context, a CPU ingest queue and the transfers form. Expected values come from tests/zip215_ref.py (Python integers on the
full-length equation), never from the library; the reference itself is checked here against the stored OpenSSL and
libsodium columns, the oracle, and the counts the policy was specified with."""
import numpy as np
import pytest

import legacy_ref as lr
import reason_ref as rr
import zip215_ref as zr

SENTINEL = 0xA5
ZIP = zr.POLICIES.index(zr.ZIP215)  # the column of verify_all


@pytest.fixture(scope="module")
def at2v_mod():
    import at2v
    at2v.load_library()
    return at2v


@pytest.fixture(scope="module")
def cases():
    return zr.constructed()


class Data:
    """records and what every policy makes of them: valid bool[n, 4] and reasons u8[n, 4] in the order of zr.POLICIES"""

    def __init__(self, pk, sig, msg, off, valid):
        self.pk, self.sig, self.msg, self.off = pk, sig, msg, np.asarray(off, np.uint32)
        self.n = len(pk)
        self.valid = np.asarray(valid, bool).reshape(self.n, 4)
        self.reasons = np.stack([zr.reasons(pk, sig, self.valid[:, c], p) for c, p in enumerate(zr.POLICIES)], axis=1)
        self.valid.setflags(write=False)
        self.reasons.setflags(write=False)

    def message(self, i):
        return self.msg[self.off[i]:self.off[i + 1]].tobytes()


def subset(g, idx, valid):
    idx = np.asarray(idx)
    msg = b"".join(g.message(i) for i in idx)
    off = np.concatenate([[0], np.cumsum([int(g.off[i + 1] - g.off[i]) for i in idx])]).astype(np.uint32)
    return Data(np.ascontiguousarray(g.pk[idx]), np.ascontiguousarray(g.sig[idx]), np.frombuffer(msg, np.uint8), off,
                valid)


@pytest.fixture(scope="module")
def data(golden, oracle, cases):
    """all of edge; the 131 adversarial records on which ZIP215 and dalek differ plus every 16th other; the constructed
    records. Columns 0 and 1 are the fixtures' stored ones, column 2 legacy_ref's, column 3 the stored reference column
    (re-derived below)."""
    out = {}
    for name in ("edge", "adversarial"):
        g = golden[name]
        z = zr.stored(name, g.n)
        valid = np.stack([g.dalek, g.sodium, lr.legacy_expected_set(oracle, g), z], axis=1)
        idx = np.arange(g.n) if name == "edge" else np.nonzero((z != g.dalek) | (np.arange(g.n) % 16 == 0))[0]
        out[name] = subset(g, idx, valid[idx])
    a = out["adversarial"]
    assert out["edge"].n == 609 and a.n == 131 + 512 - 8  # (8 of the 131 are 16th records)
    assert (a.valid[:, ZIP] != a.valid[:, 0]).sum() == 131
    out["constructed"] = Data(*zr.pack(cases), [c.verdicts for c in cases])
    return out


def test_reference_reproduces_the_specified_counts(golden):
    """the table the policy was specified with, re-derived from the Python-integer reference over whole fixture sets;
    its DALEK_V1 and LIBSODIUM columns must be the stored OpenSSL and libsodium ones, and the stored ZIP215 columns the
    other tests read must be what it computes"""
    want = {"adversarial": (8192, 7451, 7582, 131, 88), "edge": (609, 184, 537, 353, 87), "rfc8032": (3, 3, 3, 0, 0)}
    for name, (n, n_dalek, n_zip, n_diff, n_noncanon) in want.items():
        g = golden[name]
        e = zr.expected_set(g)
        assert np.array_equal(e[:, 0], g.dalek) and np.array_equal(e[:, 1], g.sodium), name
        z = e[:, ZIP]
        diff = np.nonzero(z != g.dalek)[0]
        got = (g.n, int(g.dalek.sum()), int(z.sum()), len(diff),
               sum(not zr.canonical(g.sig[i, :32].tobytes()) for i in diff))
        assert got == (n, n_dalek, n_zip, n_diff, n_noncanon), name
        assert not (g.dalek & ~z).any(), name  # a DALEK_V1 accept implies a ZIP215 accept
        if name != "rfc8032":
            assert np.array_equal(zr.stored(name, g.n), z), name
    for name in ("at2_cfg1", "ragged"):  # every 16th record checked: nothing differs
        g = golden[name]
        idx = range(0, g.n, 16)
        e = zr.expected_set(g, idx)
        assert np.array_equal(e[:, ZIP], g.dalek[::16]) and np.array_equal(e[:, 0], g.dalek[::16]), name


def test_constructed_records_are_what_they_claim(cases, oracle):
    matrix = cases[:196]
    assert len(zr.torsion_encodings()) == 14 and all(c.name.startswith("torsion") for c in matrix)
    assert all(c.zip215 for c in matrix)  # ZIP-215 accepts all 196
    for c in cases:  # the reference's cofactorless columns against the oracle, on every constructed record
        assert oracle.verify(c.pk, c.sig, c.msg, rr.DALEK) == bool(c.verdicts[0]), c.name
        assert oracle.verify(c.pk, c.sig, c.msg, rr.LIBSODIUM) == bool(c.verdicts[1]), c.name
        assert lr.legacy_expected(oracle, c.pk, c.sig, c.msg) == bool(c.verdicts[2]), c.name
        assert zr.verify(c.pk, c.sig, c.msg, zr.ZIP215) == c.zip215, c.name
    n_differ = sum(c.zip215 != c.dalek for c in matrix)
    assert n_differ > 98, "the two columns differ on most of the matrix"
    shifted, pairs = zr.shifted_cases()
    assert len(pairs) == 8 + 7 + 3 and {p for p in pairs if p[0] == 0} == {(0, j) for j in range(8)}
    for c, (ja, jr) in zip(shifted, pairs):
        assert c.zip215, c.name
        assert c.dalek == zr.dalek_accepts_shift(ja, jr), c.name  # only where [k]T_A + T_R = 0
    assert any(not c.dalek for c, p in zip(shifted, pairs) if p in ((0, 1), (0, 3), (1, 0), (3, 0)))  # order-8 shifts
    by_name = {c.name: c for c in zr.edge_cases()}
    V, A, S, RE, E = rr.VALID, rr.A_DECODE, rr.S_RANGE, rr.R_ENCODING, rr.EQUATION
    for name, dalek, zip215, why in (("shifted, one bit of M flipped", 0, 0, E), ("shifted, S + l", 0, 0, S),
                                     ("R off the curve", 0, 0, RE), ("A off the curve", 0, 0, A),
                                     ("non-canonical R (y = p + 1) that decodes to R'", 0, 1, V),
                                     ("R = (0, 1) with the sign bit set, matching S", 0, 1, V),
                                     ("plain valid record", 1, 1, V)):
        c = by_name[name]
        assert (c.verdicts[0], c.verdicts[ZIP], c.reasons[ZIP]) == (dalek, zip215, why), name
    assert {r for c in cases for r in (c.reasons[ZIP],)} <= {V, A, S, RE, E}  # reasons 3 and 4 never occur


def test_verify_one_policy_and_reason(at2v_mod, data):
    lib = at2v_mod.load_library()
    for key, d in data.items():
        for i in range(d.n):
            pk, sig, m = d.pk[i].tobytes(), d.sig[i].tobytes(), d.message(i)
            assert at2v_mod.verify_one(pk, sig, m, "zip215") == d.valid[i, ZIP], (key, i)
            assert at2v_mod.verify_one_reason(pk, sig, m, zr.ZIP215) == d.reasons[i, ZIP], (key, i)
    d = data["constructed"]
    for i in range(d.n):  # the old policies on the records built for the new one
        for c, p in enumerate(zr.POLICIES[:3]):
            pk, sig, m = d.pk[i].tobytes(), d.sig[i].tobytes(), d.message(i)
            assert at2v_mod.verify_one(pk, sig, m, zr.NAMES[p]) == d.valid[i, c], (i, p)
            assert at2v_mod.verify_one_reason(pk, sig, m, p) == d.reasons[i, c], (i, p)
    assert lib.at2v_verify_one_policy(bytes(32), bytes(64), None, 0, 4) in (0, 1)
    for bad in (3, 5, -1):
        assert lib.at2v_verify_one_policy(bytes(32), bytes(64), None, 0, bad) == -1
        assert lib.at2v_verify_one_reason(bytes(32), bytes(64), None, 0, bad) == -1


def test_cpu_context_verdicts_and_reasons(at2v_mod, data):
    with at2v_mod.BatchVerifier(num_gpus=0, policy="zip215", cpu_threads=4) as v:
        assert v.policy == 4
        for key, d in data.items():
            ok = v.verify_batch(d.pk, d.sig, d.msg, d.off)
            assert np.array_equal(ok, d.valid[:, ZIP]), (key, np.nonzero(ok != d.valid[:, ZIP])[0][:8])
            assert np.array_equal(v.reject_reasons(d.pk, d.sig, ok), d.reasons[:, ZIP]), key


def test_policy_mask_refuses_a_zip215_context(at2v_mod, data):
    """a cofactored verdict cannot tell the cofactorless rules apart: AT2V_E_INVALID, nothing written"""
    lib = at2v_mod.load_library()
    d = data["edge"]
    n = 70
    pk, sig = np.ascontiguousarray(d.pk[:n]), np.ascontiguousarray(d.sig[:n])
    words = np.full(3, 0xFFFFFFFF, np.uint32)
    with at2v_mod.BatchVerifier(num_gpus=0, policy="zip215", cpu_threads=2) as v:
        buf = np.full(n + 16, SENTINEL, np.uint8)
        assert lib.at2v_policy_mask(v._h, pk.ctypes.data, sig.ctypes.data, n, words.ctypes.data, buf.ctypes.data) == -1
        assert (buf == SENTINEL).all()
        assert lib.at2v_policy_mask_device(v._h, 16, 16, 1, 16, 16, None) == -1


@pytest.mark.parametrize("fallback", [False, True])
def test_old_policies_give_their_columns(at2v_mod, data, fallback):
    for c, p in enumerate(zr.POLICIES[:3]):
        with at2v_mod.BatchVerifier(num_gpus=0, policy=zr.NAMES[p], cpu_threads=4, cpu_fallback=fallback) as v:
            for key, d in data.items():
                ok = v.verify_batch(d.pk, d.sig, d.msg, d.off)
                assert np.array_equal(ok, d.valid[:, c]), (key, p, np.nonzero(ok != d.valid[:, c])[0][:8])
                assert np.array_equal(v.reject_reasons(d.pk, d.sig, ok), d.reasons[:, c]), (key, p)


def test_transfers_on_a_cpu_context(at2v_mod):
    snd, sig, rcp, amt, want = zr.transfer_cases()
    assert want[:, ZIP].tolist() == [True] * 5 + [False] and not want[1:4, 0].any()
    for c, p in enumerate(zr.POLICIES):
        with at2v_mod.BatchVerifier(num_gpus=0, policy=zr.NAMES[p], cpu_threads=2) as v:
            assert v.verify_transfers(snd, sig, rcp, amt).tolist() == want[:, c].tolist(), p


@pytest.mark.parametrize("reasons", [False, True])
def test_cpu_queue(data, reasons):
    from at2v import node
    with node.IngestQueue(cpu=True, policy="zip215", reasons=reasons, max_batch=512, cpu_threads=4) as q:
        want = []
        for d in data.values():
            q.submit(d.pk, d.sig, d.msg, d.off)
            want += (d.reasons[:, ZIP] if reasons else d.valid[:, ZIP].astype(int)).tolist()
        q.flush()
        tickets, got = [], []
        while len(got) < len(want):
            t, r = q.poll_reasons(4096, 2_000_000) if reasons else q.poll(4096, 2_000_000)
            assert len(t), "queue stalled"
            tickets += t.tolist()
            got += r.tolist()
        assert tickets == list(range(tickets[0], tickets[0] + len(want))) and got == want
