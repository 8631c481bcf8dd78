"""GPU: the reject-reasons pass (at2v_reject_reasons_device / at2v_reject_reasons / the queue's poll_reasons) through the
C ABI of libat2v.so, behind every verify form. Expected bytes come from tests/reason_ref.py (Python integers only; its
own cross-checks are in tests/test_reasons_cpu.py). Every device launch writes into a buffer pre-filled with 0xA5 that
carries 64 guard bytes after byte n - 1: valid records must come back 0, the guard must survive."""
import numpy as np
import pytest

import reason_ref as rr

pytestmark = pytest.mark.gpu

GUARD = 64
POLICIES = {"dalek": rr.DALEK, "libsodium": rr.LIBSODIUM}


@pytest.fixture(scope="module")
def at2v_mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import at2v
    at2v.load_library()
    return at2v


@pytest.fixture(scope="module")
def verifiers(at2v_mod):
    vs = {p: at2v_mod.BatchVerifier(device=0, policy=p) for p in POLICIES}
    yield vs
    for v in vs.values():
        v.close()


@pytest.fixture(scope="module")
def expected(golden):
    out = {}
    for name in ("adversarial", "edge"):
        g = golden[name]
        for pname, pol in POLICIES.items():
            r = rr.reasons(g.pk, g.sig, g.dalek if pol == rr.DALEK else g.sodium, pol)
            r.setflags(write=False)
            out[(name, pname)] = r
    return out


def device_pass(v, pk, sig, msg, off):
    """one verify_batch_device launch and the reasons pass right behind it on the same stream ->
    (bool[n] verdicts, u8[n] reasons); checks the guard bytes"""
    import torch
    import at2v
    pk = np.ascontiguousarray(pk, np.uint8).reshape(-1, 32)
    sig = np.ascontiguousarray(sig, np.uint8).reshape(-1, 64)
    n = len(pk)
    off = (np.asarray(off[:n + 1]) - off[0]).astype(np.uint32)
    mb = int(off[-1])
    m = np.zeros(mb + 16, np.uint8)
    m[:mb] = np.asarray(msg, np.uint8)[:mb]
    dev = "cuda:0"
    d_pk = torch.from_numpy(pk.reshape(-1).copy()).to(dev)
    d_sig = torch.from_numpy(sig.reshape(-1).copy()).to(dev)
    d_msg = torch.from_numpy(m).to(dev)
    d_off = torch.from_numpy(off.view(np.int32).copy()).to(dev)
    nwords = (n + 31) // 32
    d_ver = torch.zeros(nwords, dtype=torch.int32, device=dev)
    d_rea = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    v.verify_batch_device(d_pk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), mb, d_off.data_ptr(), n,
                          d_ver.data_ptr(), s)
    v.reject_reasons_device(d_pk.data_ptr(), d_sig.data_ptr(), n, d_ver.data_ptr(), d_rea.data_ptr(), s)
    torch.cuda.synchronize()
    ok = at2v.unpack_verdicts(d_ver.cpu().numpy().view(np.uint32), n)
    rea = d_rea.cpu().numpy()
    assert (rea[n:] == 0xA5).all(), "a byte at or after reasons + n was written"
    return ok, rea[:n]


def cut(g, lo, hi):
    return g.pk[lo:hi], g.sig[lo:hi], g.msg[int(g.off[lo]):int(g.off[hi])], g.off[lo:hi + 1]


@pytest.mark.parametrize("policy", ["dalek", "libsodium"])
@pytest.mark.parametrize("name", ["edge", "adversarial"])
def test_device_form_after_verify(verifiers, golden, expected, name, policy):
    g = golden[name]
    ok, rea = device_pass(verifiers[policy], *cut(g, 0, g.n))
    want = expected[(name, policy)]
    assert np.array_equal(ok, want == 0)
    assert np.array_equal(rea, want), np.nonzero(rea != want)[0][:8]


@pytest.mark.parametrize("policy", ["dalek", "libsodium"])
def test_constructed_records(at2v_mod, verifiers, golden, policy):
    """reason 4 (in no fixture) and the priority cases, from one valid record of at2_cfg1"""
    g = golden["at2_cfg1"]
    cases = rr.constructed(g.pk[0].tobytes(), g.sig[0].tobytes())
    pk, sig, msg, off = at2v_mod.pack_records([c[1] for c in cases], [c[2] for c in cases],
                                              [g.message(0)] * len(cases))
    ok, rea = device_pass(verifiers[policy], pk, sig, msg, off)
    assert not ok.any()
    assert rea.tolist() == [c[3 + POLICIES[policy]] for c in cases]
    assert 4 in rea.tolist() if policy == "libsodium" else 4 not in rea.tolist()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4097])
def test_sizes(verifiers, golden, expected, n):
    """the tail word, pad bits, the tile edge (2,048 records) and a last tile of one record"""
    g = golden["adversarial"]
    ok, rea = device_pass(verifiers["dalek"], *cut(g, 0, n))
    want = expected[("adversarial", "dalek")][:n]
    assert np.array_equal(ok, want == 0)
    assert np.array_equal(rea, want), np.nonzero(rea != want)[0][:8]


def test_densities(verifiers, golden):
    """no reject at all, and every record rejected: 2,048 rejects per tile, so the dense walk loops 8 times"""
    g = golden["at2_cfg1"]
    ok, rea = device_pass(verifiers["dalek"], *cut(g, 0, g.n))
    assert ok.all() and not rea.any()
    sig = g.sig.copy()
    i = np.arange(g.n)
    sig[i, (i * 7) % 64] ^= (1 << ((i // 64) % 8)).astype(np.uint8)  # one signature bit per record
    ok, rea = device_pass(verifiers["dalek"], g.pk, sig, g.msg, g.off)
    assert not ok.any()
    want = rr.reasons(g.pk, sig, np.zeros(g.n, bool), rr.DALEK)
    assert set(want.tolist()) == {2, 5, 6}
    assert np.array_equal(rea, want), np.nonzero(rea != want)[0][:8]


@pytest.mark.parametrize("policy", ["dalek", "libsodium"])
def test_host_form_on_a_gpu_context(verifiers, golden, expected, policy):
    v = verifiers[policy]
    for name in ("adversarial", "edge"):
        g = golden[name]
        want = expected[(name, policy)]
        ok = v.verify_batch(g.pk, g.sig, g.msg, g.off)
        assert np.array_equal(ok, want == 0)
        got = v.reject_reasons(g.pk, g.sig, ok)
        assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:8])
    g = golden["adversarial"]
    ones = np.full((g.n + 31) // 32, 0xFFFFFFFF, np.uint32)  # nothing to upload: all zeros back
    assert not v.reject_reasons(g.pk, g.sig, ones).any()
    got = v.reject_reasons(g.pk[:33], g.sig[:33], np.zeros(2, np.uint32))  # every bit 0, one record in the tail word
    assert np.array_equal(got, rr.reasons(g.pk[:33], g.sig[:33], np.zeros(33, bool), POLICIES[policy]))


def test_host_form_device_error(at2v_mod, golden, expected, monkeypatch):
    """the existing hook AT2V_TEST_FAIL_LAUNCH reaches the pass's own launch: without the fallback flag a negative
    code and every byte 0xff; with AT2V_CTX_CPU_FALLBACK AT2V_OK and exact bytes from the CPU pool"""
    g = golden["adversarial"]
    want = expected[("adversarial", "dalek")]
    words = rr.words_of(want == 0)
    lib = at2v_mod.load_library()
    monkeypatch.setenv("AT2V_TEST_FAIL_LAUNCH", "1")
    with at2v_mod.BatchVerifier() as v:
        buf = np.full(g.n + GUARD, 0xA5, np.uint8)
        pk, sig = np.ascontiguousarray(g.pk), np.ascontiguousarray(g.sig)
        rc = lib.at2v_reject_reasons(v._h, pk.ctypes.data, sig.ctypes.data, g.n, words.ctypes.data, buf.ctypes.data)
        assert rc < 0
        assert (buf[:g.n] == 0xFF).all() and (buf[g.n:] == 0xA5).all()
        assert np.array_equal(v.reject_reasons(g.pk, g.sig, words), want)  # the next call runs on the device
    with at2v_mod.BatchVerifier(cpu_fallback=True, cpu_threads=4) as v:
        assert np.array_equal(v.reject_reasons(g.pk, g.sig, words), want)  # on the CPU pool
        assert np.array_equal(v.reject_reasons(g.pk, g.sig, words), want)  # on the device


def test_behind_the_other_verify_forms(at2v_mod, golden):
    """the pass does not care which kernel wrote the bits: the low-latency kernel (a launch of <= small_batch_max), the
    throughput kernel (AT2V_SMALL_BATCH_OFF), and a sender_cache + sender_comb context launched twice, so that the
    second launch verifies by the combs"""
    g = golden["at2_cfg1"]
    rng = np.random.default_rng(11)
    bad = rng.choice(g.n, g.n // 20, replace=False)
    sig = g.sig.copy()
    sig[bad, rng.integers(0, 64, len(bad))] ^= (1 << rng.integers(0, 8, len(bad))).astype(np.uint8)
    valid = np.ones(g.n, bool)
    valid[bad] = False
    want = rr.reasons(g.pk, sig, valid, rr.DALEK)
    OFF = at2v_mod.SMALL_BATCH_OFF
    runs = []
    with at2v_mod.BatchVerifier() as v:
        assert g.n <= at2v_mod.SMALL_BATCH_DEFAULT
        runs.append(("small batch", device_pass(v, g.pk, sig, g.msg, g.off)))
    with at2v_mod.BatchVerifier(small_batch_max=OFF) as v:
        runs.append(("throughput", device_pass(v, g.pk, sig, g.msg, g.off)))
    with at2v_mod.BatchVerifier(small_batch_max=OFF, sender_cache=1024, sender_comb=True, admit_first=True) as v:
        runs.append(("comb, first launch", device_pass(v, g.pk, sig, g.msg, g.off)))
        before = v.info()["cache_record_hits"]
        runs.append(("comb, second launch", device_pass(v, g.pk, sig, g.msg, g.off)))
        assert v.info()["cache_record_hits"] > before  # the second launch did take senders from the cache
    for what, (ok, rea) in runs:
        assert np.array_equal(ok, valid), what
        assert np.array_equal(rea, want), (what, np.nonzero(rea != want)[0][:8])


def poll_all(q, n):
    tickets, reasons = [], []
    while len(tickets) < n:
        t, r = q.poll_reasons(1 << 16, 5_000_000)
        assert len(t), "queue stalled"
        tickets += t.tolist()
        reasons += r.tolist()
    return tickets, np.array(reasons, np.uint8)


def test_queue_poll_reasons(at2v_mod, golden, expected):
    """AT2V_QUEUE_EAGER | AT2V_QUEUE_REASONS on the device: ragged pieces into batches of <= 1,024 (read and written in
    the slot's pinned memory), then one batch of 2,000 in a 4,096-record slot (uploaded)"""
    from at2v.node import IngestQueue
    g = golden["adversarial"]
    n = 2000
    want = expected[("adversarial", "dalek")][:n]
    with IngestQueue(device=0, max_batch=1024, eager=True, reasons=True) as q:
        rng = np.random.default_rng(3)
        at, first = 0, None
        while at < n:
            m = min(n - at, int(rng.integers(1, 400)))
            off = g.off[at:at + m + 1]
            t = q.submit(g.pk[at:at + m], g.sig[at:at + m], g.msg[int(off[0]):int(off[-1])], off - off[0])
            first = t if first is None else first
            at += m
        q.flush()
        tickets, reasons = poll_all(q, n)
        assert tickets == list(range(first, first + n))
        assert np.array_equal(reasons, want), np.nonzero(reasons != want)[0][:8]
        st = q.stats()
        assert st["failed_batches"] == 0 and st["batches"] >= 2
    with IngestQueue(device=0, max_batch=4096, eager=True, reasons=True) as q:
        first = q.submit(g.pk[:n], g.sig[:n], g.msg[:int(g.off[n])], g.off[:n + 1])
        q.flush()
        tickets, reasons = poll_all(q, n)
        assert tickets == list(range(first, first + n))
        assert np.array_equal(reasons, want), np.nonzero(reasons != want)[0][:8]
        assert q.stats()["batches"] == 1  # one batch above the pinned-read threshold
    with IngestQueue(device=0, max_batch=1024, eager=True) as q:  # without the flag
        with pytest.raises(at2v_mod.At2vError) as e:
            q.poll_reasons(16, 0)
        assert e.value.code == -1


def test_queue_reasons_with_cpu_fallback(at2v_mod, golden, expected, monkeypatch):
    """AT2V_QUEUE_CPU_FALLBACK | AT2V_QUEUE_REASONS: the first two batches fail to launch (the existing test hook) and
    get their reasons from the CPU routine, the third from the device; one ticket order, no 0xff"""
    from at2v.node import IngestQueue
    monkeypatch.setenv("AT2V_TEST_FAIL_LAUNCH", "2")
    g = golden["adversarial"]
    n = 3000
    want = expected[("adversarial", "dalek")][:n]
    with IngestQueue(device=0, max_batch=1024, max_delay_us=300, cpu_fallback=True, cpu_threads=4, reasons=True) as q:
        first = q.submit(g.pk[:n], g.sig[:n], g.msg[:int(g.off[n])], g.off[:n + 1])
        q.flush()
        tickets, reasons = poll_all(q, n)
        st = q.stats()
    assert tickets == list(range(first, first + n))
    assert np.array_equal(reasons, want), np.nonzero(reasons != want)[0][:8]
    assert st["cpu_fallbacks"] == 2 and st["failed_batches"] == 0 and st["batches"] == 3, st
