"""CPU: AT2V_POLICY_DALEK_V1_LEGACY (dalek's `legacy_compatibility` scalar rule) and the per-record policy mask through the
C ABI without a device: at2v_verify_one_policy / _reason, a CPU context and a CPU ingest queue. Expected values come from
tests/legacy_ref.py: the fixtures' stored columns (OpenSSL, libsodium), the oracle on R || (s - l), and Python integers."""
import numpy as np
import pytest

import legacy_ref as lr
import reason_ref as rr

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def at2v_mod():
    import at2v
    at2v.load_library()
    return at2v


@pytest.fixture(scope="module")
def legacy(golden, oracle):
    """set -> bool[n] expected under the legacy policy, computed once and never modified"""
    return {name: lr.legacy_expected_set(oracle, g) for name, g in golden.items()}


@pytest.fixture(scope="module")
def cases(golden, oracle):
    return lr.constructed(oracle, golden["at2_cfg1"])


def test_fixtures_hold_the_class_the_rule_is_about(golden, legacy):
    """counted with the oracle when the policy was specified: a fixture that lost the class would pass vacuously"""
    n_class, n_acc = {}, {}
    for name, g in golden.items():
        cls = np.array([lr.in_class(g.sig[i].tobytes()) for i in range(g.n)])
        n_class[name], n_acc[name] = int(cls.sum()), int((cls & legacy[name]).sum())
        assert np.array_equal(legacy[name][~cls], g.dalek[~cls])  # outside the class the two rules agree
        assert not (g.dalek & ~legacy[name]).any()  # nested
    assert n_class == {"rfc8032": 0, "at2_cfg1": 0, "adversarial": 109, "edge": 3, "ragged": 1}
    assert n_acc == {"rfc8032": 0, "at2_cfg1": 0, "adversarial": 108, "edge": 0, "ragged": 0}


def test_constructed_records_are_what_they_claim(cases, oracle):
    """the stated verdicts against the oracle and the helper's rules"""
    for c in cases:
        assert oracle.verify(c.pk, c.sig, c.msg, rr.DALEK) == bool(c.verdicts[0]), c.name
        assert oracle.verify(c.pk, c.sig, c.msg, rr.LIBSODIUM) == bool(c.verdicts[1]), c.name
        assert lr.legacy_expected(oracle, c.pk, c.sig, c.msg) == bool(c.verdicts[2]), c.name
        assert lr.mask_expected(c.pk, c.sig, bool(c.verdicts[2])) == c.mask, c.name
        assert c.mask == sum(v << p for p, v in enumerate(c.verdicts)), c.name
        assert rr.reason(c.pk, c.sig, bool(c.verdicts[0]), rr.DALEK) == c.reasons[0], c.name
        assert rr.reason(c.pk, c.sig, bool(c.verdicts[1]), rr.LIBSODIUM) == c.reasons[1], c.name
        assert lr.reason_legacy(c.pk, c.sig, bool(c.verdicts[2])) == c.reasons[2], c.name
    assert {c.mask for c in cases} == {0, 4, 5, 7}


def test_verify_one_policy_and_reason(at2v_mod, golden, legacy, cases):
    for name, g in golden.items():
        want = legacy[name]
        want_r = lr.reasons_legacy(g.pk, g.sig, want)
        got = np.array([at2v_mod.verify_one(g.pk[i].tobytes(), g.sig[i].tobytes(), g.message(i), "dalek-legacy")
                        for i in range(g.n)])
        assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:8])
        got_r = np.array([at2v_mod.verify_one_reason(g.pk[i].tobytes(), g.sig[i].tobytes(), g.message(i), "dalek-legacy")
                          for i in np.nonzero(~want)[0]], np.uint8)
        assert np.array_equal(got_r, want_r[~want]), name
    for c in cases:
        for p, pol in enumerate(("dalek", "libsodium", "dalek-legacy")):
            assert at2v_mod.verify_one(c.pk, c.sig, c.msg, pol) == bool(c.verdicts[p]), (c.name, pol)
            assert at2v_mod.verify_one_reason(c.pk, c.sig, c.msg, pol) == c.reasons[p], (c.name, pol)
    lib = at2v_mod.load_library()
    assert lib.at2v_verify_one_policy(bytes(32), bytes(64), None, 0, 2) in (0, 1)
    for bad in (3, -1):
        assert lib.at2v_verify_one_policy(bytes(32), bytes(64), None, 0, bad) == -1
        assert lib.at2v_verify_one_reason(bytes(32), bytes(64), None, 0, bad) == -1


def test_cpu_context_verdicts_reasons_and_mask(at2v_mod, golden, legacy, cases):
    cpk, csig, cmsg, coff = lr.pack(cases)
    with at2v_mod.BatchVerifier(num_gpus=0, policy="dalek-legacy", cpu_threads=4) as v:
        for name, g in golden.items():
            want = legacy[name]
            ok = v.verify_batch(g.pk, g.sig, g.msg, g.off)
            assert np.array_equal(ok, want), (name, np.nonzero(ok != want)[0][:8])
            assert np.array_equal(v.reject_reasons(g.pk, g.sig, ok), lr.reasons_legacy(g.pk, g.sig, want)), name
            mask = v.policy_mask(g.pk, g.sig, ok)
            # the strong check: bits 0 and 1 reproduce the stored OpenSSL and libsodium columns, bit for bit
            assert np.array_equal((mask & 1).astype(bool), g.dalek), name
            assert np.array_equal((mask & 2).astype(bool), g.sodium), name
            assert np.array_equal((mask & 4).astype(bool), want), name
            assert np.array_equal(mask, lr.masks_expected(g.pk, g.sig, want)), name
        ok = v.verify_batch(cpk, csig, cmsg, coff)
        assert ok.tolist() == [bool(c.verdicts[2]) for c in cases]
        assert v.reject_reasons(cpk, csig, ok).tolist() == [c.reasons[2] for c in cases]
        assert v.policy_mask(cpk, csig, ok).tolist() == [c.mask for c in cases]
        with pytest.raises(at2v_mod.At2vError) as e:  # a device entry point on a CPU context
            v.policy_mask_device(16, 16, 1, 16, 16)
        assert e.value.code == -2


def test_transfers_on_a_cpu_context(at2v_mod, oracle):
    """the transfers form takes the policy unchanged in shape"""
    snd, sig, rcp, amt = lr.transfer_pair(oracle)
    for pname, want in (("dalek-legacy", [True, True]), ("dalek", [True, False]), ("libsodium", [True, False])):
        with at2v_mod.BatchVerifier(num_gpus=0, policy=pname, cpu_threads=2) as v:
            assert v.verify_transfers(snd, sig, rcp, amt).tolist() == want, pname


def test_old_policies_unchanged_and_refuse_the_mask(at2v_mod, golden):
    lib = at2v_mod.load_library()
    for pname, col in (("dalek", "dalek"), ("libsodium", "sodium")):
        with at2v_mod.BatchVerifier(num_gpus=0, policy=pname, cpu_threads=4) as v:
            for name, g in golden.items():
                assert np.array_equal(v.verify_batch(g.pk, g.sig, g.msg, g.off), getattr(g, col)), (name, pname)
            g = golden["edge"]
            n = 70
            pk, sig = np.ascontiguousarray(g.pk[:n]), np.ascontiguousarray(g.sig[:n])
            words = np.full(3, 0xFFFFFFFF, np.uint32)
            buf = np.full(n + 16, SENTINEL, np.uint8)
            assert lib.at2v_policy_mask(v._h, pk.ctypes.data, sig.ctypes.data, n, words.ctypes.data,
                                        buf.ctypes.data) == -1
            assert (buf == SENTINEL).all()
            assert lib.at2v_policy_mask_device(v._h, 16, 16, 1, 16, 16, None) == -1


def test_mask_trusts_the_words_and_fails_closed(at2v_mod, golden):
    g = golden["at2_cfg1"]
    n = 70
    lib = at2v_mod.load_library()
    with at2v_mod.BatchVerifier(num_gpus=0, policy="dalek-legacy", cpu_threads=2) as v:
        buf = np.full(n + 64, SENTINEL, np.uint8)
        words = np.array([0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFF], np.uint32)  # record 0 handed in as rejected; pad bits set
        pk, sig = np.ascontiguousarray(g.pk[:n]), np.ascontiguousarray(g.sig[:n])
        assert lib.at2v_policy_mask(v._h, pk.ctypes.data, sig.ctypes.data, n, words.ctypes.data, buf.ctypes.data) == 0
        assert buf[0] == 0 and (buf[1:n] == 7).all() and (buf[n:] == SENTINEL).all()
        assert lib.at2v_policy_mask(v._h, None, None, 0, None, None) == 0  # n = 0
        assert lib.at2v_policy_mask(v._h, None, sig.ctypes.data, n, words.ctypes.data, buf.ctypes.data) == -1
        assert not buf[:n].any() and (buf[n:] == SENTINEL).all()  # an error: every byte 0
        assert lib.at2v_policy_mask(None, pk.ctypes.data, sig.ctypes.data, n, words.ctypes.data, buf.ctypes.data) == -1


def test_policy_3_is_refused_everywhere(at2v_mod):
    from at2v import node
    lib = at2v_mod.load_library()
    assert 3 not in at2v_mod._POLICIES.values()
    at2v_mod._POLICIES["three"] = 3  # past the binding's own table, to the library
    try:
        with pytest.raises(at2v_mod.At2vError) as e:
            at2v_mod.BatchVerifier(num_gpus=0, policy="three")
        assert e.value.code == -1
        with pytest.raises(at2v_mod.At2vError) as e:
            node.IngestQueue(cpu=True, policy="three")
        assert e.value.code == -1
    finally:
        del at2v_mod._POLICIES["three"]
    assert lib.at2v_verify_one_policy(bytes(32), bytes(64), None, 0, 3) == -1
    assert lib.at2v_verify_one_reason(bytes(32), bytes(64), None, 0, 3) == -1


def test_cpu_queue_under_the_legacy_policy(at2v_mod, golden, legacy, cases):
    from at2v import node
    g = golden["adversarial"]
    n = 2000
    want = legacy["adversarial"][:n]
    want_r = lr.reasons_legacy(g.pk[:n], g.sig[:n], want)
    cpk, csig, cmsg, coff = lr.pack(cases)
    assert (want != g.dalek[:n]).any()  # the slice holds records whose verdict depends on the rule
    for reasons in (False, True):
        with node.IngestQueue(cpu=True, policy="dalek-legacy", reasons=reasons, max_batch=512, cpu_threads=4) as q:
            q.submit(g.pk[:n], g.sig[:n], g.msg[:g.off[n]], g.off[:n + 1])
            q.submit(cpk, csig, cmsg, coff)
            q.flush()
            got = []
            while len(got) < n + len(cases):
                t, r = q.poll_reasons(4096, 2_000_000) if reasons else q.poll(4096, 2_000_000)
                assert len(t), "queue stalled"
                got += r.tolist()
            if reasons:
                assert got == want_r.tolist() + [c.reasons[2] for c in cases]
            else:
                assert got == want.astype(int).tolist() + [c.verdicts[2] for c in cases]
