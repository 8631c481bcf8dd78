"""CPU: AT2 transfers verified from their fields (include/at2v.h at2v_verify_transfers*, at2v_queue_submit_transfers) on
the library's CPU backend. A node holds sender, recipient, amount and signature, never the message: the library builds
M = bincode(ThinTransaction{recipient, amount}) itself (csrc/at2v_transfer.h) and the verdict of record i is that of
at2v_verify_batch over (sender_i, sig_i, M_i). Expected bits come from the golden verdicts and the oracle over messages
rebuilt in numpy (tests/transfer_cases.py), and are compared with the library's own records path as well."""
import ctypes
import threading

import numpy as np
import pytest

import transfer_cases as tc


@pytest.fixture(scope="module")
def at2v_mod():
    import at2v
    at2v.load_library()
    return at2v


@pytest.fixture(scope="module")
def cpu_ctx(at2v_mod):
    v = at2v_mod.BatchVerifier(num_gpus=0, cpu_threads=4)
    yield v
    v.close()


@pytest.mark.parametrize("policy", ["dalek", "libsodium"])
def test_cfg1_all_valid_then_mutated(at2v_mod, policy):
    """at2_cfg1 by its fields: all 4,096 valid; with every 10th record mutated the result equals the golden / oracle bits
    and at2v_verify_batch over the explicit messages"""
    with at2v_mod.BatchVerifier(num_gpus=0, cpu_threads=4, policy=policy) as v:
        t = tc.cfg1()
        got = v.verify_transfers(t.sender, t.sig, t.recipient, t.amount)
        assert got.all() and len(got) == 4096
        m = tc.cfg1_mutated()
        assert not m.want[policy][m.mutated].any() and m.want[policy][~m.mutated].all()
        got = v.verify_transfers(m.sender, m.sig, m.recipient, m.amount)
        assert np.array_equal(got, m.want[policy]), np.nonzero(got != m.want[policy])[0][:10]
        msg, off = tc.build_messages(m.recipient, m.amount, tc.WIRE_BYTES)
        assert np.array_equal(got, v.verify_batch(m.sender, m.sig, msg, off))


def test_wire_array(cpu_ctx):
    """256 records signed over the 40-byte message: all valid with wire = ARRAY, all rejected with wire = BYTES"""
    t = tc.array_wire()
    assert t.n == 256
    assert cpu_ctx.verify_transfers(t.sender, t.sig, t.recipient, t.amount, wire=tc.WIRE_ARRAY).all()
    assert not cpu_ctx.verify_transfers(t.sender, t.sig, t.recipient, t.amount, wire=tc.WIRE_BYTES).any()


def test_recipient_ok(cpu_ctx):
    """recipient_ok equals Oracle.decompress_ok and at2v_decode_points over recipients mixed with the edge set's keys, and
    the verdict words are identical with and without the recipient_ok pointer"""
    t, rok = tc.recipient_mix()
    assert 0 < rok.sum() < t.n
    w0 = np.zeros((t.n + 31) // 32, np.uint32)
    w1 = np.zeros_like(w0)
    v0 = cpu_ctx.verify_transfers(t.sender, t.sig, t.recipient, t.amount, words=w0)
    v1, got = cpu_ctx.verify_transfers(t.sender, t.sig, t.recipient, t.amount, recipient_ok=True, words=w1)
    assert np.array_equal(got, rok), np.nonzero(got != rok)[0][:10]
    assert np.array_equal(got, cpu_ctx.decode_points(t.recipient))
    assert np.array_equal(w0, w1) and np.array_equal(v0, v1)
    assert np.array_equal(v0, t.want["dalek"])


@pytest.mark.parametrize("wire", [tc.WIRE_BYTES, tc.WIRE_ARRAY])
@pytest.mark.parametrize("n", [0, 1, 33, 64, 65])
def test_sizes_and_sentinels(at2v_mod, cpu_ctx, oracle, n, wire):
    """a sentinel word after each bitmap is intact and pad bits are 0"""
    t = (tc.cfg1_mutated() if wire == tc.WIRE_BYTES else tc.array_wire()).head(n)
    words = np.full((n + 31) // 32 + 1, 0xDEADBEEF, np.uint32)
    rwords = np.full((n + 31) // 32 + 1, 0xFEEDFACE, np.uint32)
    lib = at2v_mod.load_library()
    p = lambda a: a.ctypes.data if a.size else None
    rc = lib.at2v_verify_transfers(cpu_ctx._h, p(t.sender), p(t.sig), p(t.recipient), p(t.amount), n, wire,
                                   words.ctypes.data, rwords.ctypes.data)
    assert rc == 0
    assert words[-1] == 0xDEADBEEF and rwords[-1] == 0xFEEDFACE
    if n == 0:
        return
    assert np.array_equal(at2v_mod.unpack_verdicts(words[:-1], n), t.want["dalek"])
    rok = np.array([oracle.decompress_ok(t.recipient[i].tobytes()) for i in range(n)], dtype=bool)
    assert np.array_equal(at2v_mod.unpack_verdicts(rwords[:-1], n), rok)
    if n % 32:
        assert words[(n - 1) // 32] >> (n % 32) == 0 and rwords[(n - 1) // 32] >> (n % 32) == 0


def test_argument_errors_leave_outputs_untouched(at2v_mod, cpu_ctx):
    lib = at2v_mod.load_library()
    t = tc.cfg1().head(40)
    words = np.full(3, 0xDEADBEEF, np.uint32)
    rwords = np.full(3, 0xFEEDFACE, np.uint32)
    s, g, r, a = (x.ctypes.data for x in (t.sender, t.sig, t.recipient, t.amount))
    w, rw = words.ctypes.data, rwords.ctypes.data
    tk = ctypes.c_uint64(7)
    assert lib.at2v_verify_transfers(cpu_ctx._h, s, g, r, a, 40, 2, w, rw) == -1   # bad wire
    assert lib.at2v_verify_transfers(cpu_ctx._h, s, g, r, a, 40, -1, w, rw) == -1
    assert lib.at2v_verify_transfers(cpu_ctx._h, s, g, r, a, 0, 7, w, rw) == -1    # ... also with n = 0
    assert lib.at2v_verify_transfers(None, s, g, r, a, 40, 0, w, rw) == -1
    for args in [(None, g, r, a), (s, None, r, a), (s, g, None, a), (s, g, r, None)]:
        assert lib.at2v_verify_transfers(cpu_ctx._h, *args, 40, 0, w, rw) == -1
        assert lib.at2v_verify_transfers_submit(cpu_ctx._h, *args, 40, 0, w, rw, ctypes.byref(tk)) == -1
        assert tk.value == 0
        tk.value = 7
    assert lib.at2v_verify_transfers(cpu_ctx._h, s, g, r, a, 40, 0, None, rw) == -1
    assert lib.at2v_verify_transfers_submit(cpu_ctx._h, s, g, r, a, 40, 0, w, rw, None) == -1
    # the device form on a CPU context: AT2V_E_NODEVICE; a bad wire is AT2V_E_INVALID first
    assert lib.at2v_verify_transfers_device(cpu_ctx._h, s, g, r, a, 40, 0, s, 1 << 20, w, rw, None) == -2
    assert lib.at2v_verify_transfers_device(cpu_ctx._h, s, g, r, a, 40, 5, s, 1 << 20, w, rw, None) == -1
    assert lib.at2v_verify_transfers_device(cpu_ctx._h, s, g, r, a, 0, 0, None, 0, None, None, None) == 0  # n = 0
    assert (words == 0xDEADBEEF).all() and (rwords == 0xFEEDFACE).all()
    with pytest.raises(ValueError):
        cpu_ctx.verify_transfers(t.sender, t.sig, t.recipient[:39], t.amount)


def test_workspace_bytes(at2v_mod):
    ws = at2v_mod.BatchVerifier.transfers_workspace_bytes
    assert ws(0, tc.WIRE_BYTES) == 16 + 16 and ws(1, tc.WIRE_BYTES) == 16 + 48 + 16
    assert ws(3, tc.WIRE_ARRAY) == 16 + 120 + 16 and ws(4, tc.WIRE_ARRAY) == 32 + 160 + 16
    assert ws(10, 2) == 0 and ws(10, -1) == 0
    # n x L < 2^32 and n < 2^31, or the device form refuses (the generated offsets are uint32)
    assert ws((1 << 32) // 48, tc.WIRE_BYTES) > 0 and ws((1 << 32) // 48 + 1, tc.WIRE_BYTES) == 0
    assert ws(-(-(1 << 32) // 40) - 1, tc.WIRE_ARRAY) > 0 and ws(-(-(1 << 32) // 40), tc.WIRE_ARRAY) == 0
    assert ws(1 << 31, tc.WIRE_ARRAY) == 0


def test_submit_wait_with_a_records_call_in_flight(at2v_mod, golden):
    """a records call and a transfers call share the two call slots; at2v_verify_batch_wait serves both"""
    lib = at2v_mod.load_library()
    m = tc.cfg1_mutated()
    t, rok = tc.recipient_mix()
    e = golden["edge"]
    with at2v_mod.BatchVerifier(num_gpus=0, cpu_threads=2) as v:
        a = v.submit_batch(e.pk, e.sig, e.msg, e.off)
        b = v.submit_transfers(m.sender, m.sig, m.recipient, m.amount)
        assert b.ticket == a.ticket + 1
        assert np.array_equal(v.wait_batch(b), m.want["dalek"])
        assert np.array_equal(v.wait_batch(a), e.dalek)
        assert lib.at2v_verify_batch_wait(v._h, b.ticket) == -1  # waited already
        c = v.submit_transfers(t.sender, t.sig, t.recipient, t.amount, recipient_ok=True)
        d = v.submit_batch(e.pk, e.sig, e.msg, e.off)
        assert np.array_equal(v.wait_batch(d), e.dalek)
        assert np.array_equal(v.wait_batch(c), t.want["dalek"]) and np.array_equal(c.recipient_ok(), rok)
        with pytest.raises(ValueError):
            b.recipient_ok()
        assert v.info()["cpu_batches"] == 4


def test_cpu_queue_submit_transfers_from_two_threads(at2v_mod):
    """AT2V_QUEUE_CPU: two producers submit transfers; every call's records have consecutive tickets, verdicts arrive in
    ticket order and equal the expected bits"""
    from at2v import node
    m = tc.cfg1_mutated()
    a = tc.array_wire()
    runs, err = [], []

    def producer(t, step, q):
        try:
            for lo in range(0, t.n, step):
                h = t.head(min(lo + step, t.n))
                first = q.submit_transfers(h.sender[lo:], h.sig[lo:], h.recipient[lo:], h.amount[lo:], wire=t.wire)
                runs.append((first, h.want["dalek"][lo:]))
        except Exception as ex:  # noqa: BLE001 - reported by the main thread
            err.append(ex)

    with node.IngestQueue(cpu=True, cpu_threads=3, max_batch=500, max_delay_us=300) as q:
        th = [threading.Thread(target=producer, args=(m, 333, q)), threading.Thread(target=producer, args=(a, 50, q))]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not err, err
        q.flush()
        total = m.n + a.n
        got_t, got_v = [], []
        while sum(len(x) for x in got_t) < total:
            t, v = q.poll(1 << 16, 5_000_000)
            assert len(t), "queue stalled"
            got_t.append(t)
            got_v.append(v)
        st = q.stats()
    t, v = np.concatenate(got_t), np.concatenate(got_v)
    assert np.array_equal(t, np.arange(t[0], t[0] + total, dtype=np.uint64))
    assert not (v == 0xFF).any() and st["failed_batches"] == 0
    want = np.zeros(total, bool)
    seen = np.zeros(total, bool)
    for first, w in runs:
        lo = first - int(t[0])
        want[lo:lo + len(w)] = w
        assert not seen[lo:lo + len(w)].any()
        seen[lo:lo + len(w)] = True
    assert seen.all()
    assert np.array_equal(v.astype(bool), want)


def test_queue_slot_budget_and_bad_wire(at2v_mod):
    """a slot whose message region cannot take the next message is sealed and the record opens the next batch; a wire
    that is neither is refused. (The refusal of a message above a slot's whole capacity, shared with at2v_queue_submit,
    cannot be reached with L <= 48 through the C ABI: a slot's capacity is never below 64 bytes.)"""
    from at2v import node
    b, a = tc.cfg1().head(1), tc.array_wire().head(1)
    with node.IngestQueue(cpu=True, cpu_threads=1, max_batch=70, max_msg_bytes=1, max_delay_us=100000) as q:  # 70 bytes
        first = q.submit_transfers(b.sender, b.sig, b.recipient, b.amount)
        q.submit_transfers(a.sender, a.sig, a.recipient, a.amount, wire=tc.WIRE_ARRAY)  # 48 + 40 > 70: a new batch
        q.flush()
        t, v = [], []
        while sum(len(x) for x in t) < 2:
            tt, vv = q.poll(16, 5_000_000)
            assert len(tt), "queue stalled"
            t.append(tt)
            v.append(vv)
        assert list(np.concatenate(t)) == [first, first + 1] and list(np.concatenate(v)) == [1, 1]
        assert q.stats()["batches"] == 2
        with pytest.raises(at2v_mod.At2vError):
            q.submit_transfers(b.sender, b.sig, b.recipient, b.amount, wire=3)
