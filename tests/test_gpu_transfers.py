"""GPU: AT2 transfers verified from their fields (include/at2v.h at2v_verify_transfers*, at2v_queue_submit_transfers).

The prep kernel (csrc/at2v_kern_transfer.h) expands recipient and amount into the messages and offsets the verify kernels
read, and decodes the recipients on request; the host forms upload only the four field arrays per chunk. Every route a
context can take must give the verdicts of the records path. Expected bits come from the golden verdicts and the oracle
over messages rebuilt in numpy (tests/transfer_cases.py), never from the library's own records path."""
import numpy as np
import pytest

import transfer_cases as tc

pytestmark = pytest.mark.gpu

OFF = 0xFFFFFFFF  # AT2V_SMALL_BATCH_OFF
PATTERN = 0xA5
V_SENTINEL, R_SENTINEL = 0x5EA7BE17, 0x0DDBA115


@pytest.fixture(scope="module")
def at2v_mod():
    import at2v
    at2v.load_library()
    return at2v


@pytest.fixture(scope="module")
def plain(at2v_mod):
    """the default context: launches of up to 32,768 records run verify_pair_kernel"""
    v = at2v_mod.BatchVerifier()
    yield v
    v.close()


def device_call(at2v_mod, v, t, recipient_ok=True, pad=64):
    """one at2v_verify_transfers_device call over t on the current stream -> (verdicts, recipient bits or None); checks
    the `pad` bytes after the workspace, a sentinel word after each bitmap and the pad bits of both"""
    import torch
    dev = "cuda:0"
    n, words = t.n, (t.n + 31) // 32
    up = lambda a: torch.from_numpy(np.array(a, copy=True).view(np.uint8).reshape(-1)).to(dev)
    d_sender, d_sig, d_recipient, d_amount = up(t.sender), up(t.sig), up(t.recipient), up(t.amount)
    ws = at2v_mod.BatchVerifier.transfers_workspace_bytes(n, t.wire)
    assert ws > 0
    d_work = torch.full((ws + pad,), PATTERN, dtype=torch.uint8, device=dev)
    d_ver = torch.from_numpy(np.full(words + 1, V_SENTINEL, np.uint32).view(np.int32)).to(dev)
    d_rok = torch.from_numpy(np.full(words + 1, R_SENTINEL, np.uint32).view(np.int32)).to(dev)
    v.verify_transfers_device(d_sender.data_ptr(), d_sig.data_ptr(), d_recipient.data_ptr(), d_amount.data_ptr(), n,
                              t.wire, d_work.data_ptr(), ws, d_ver.data_ptr(), d_rok.data_ptr() if recipient_ok else 0,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (d_work[ws:].cpu().numpy() == PATTERN).all(), "written past the workspace"
    ver = d_ver.cpu().numpy().view(np.uint32)
    rok = d_rok.cpu().numpy().view(np.uint32)
    assert ver[-1] == V_SENTINEL and rok[-1] == R_SENTINEL
    if not recipient_ok:
        assert (rok == R_SENTINEL).all()
    if n % 32:
        assert int(ver[words - 1]) >> (n % 32) == 0
        assert not recipient_ok or int(rok[words - 1]) >> (n % 32) == 0
    # the workspace holds what the verify kernels read: offsets i * L, then the messages at a 16-byte boundary
    L = 48 if t.wire == tc.WIRE_BYTES else 40
    work = d_work[:ws].cpu().numpy()
    msg, off = tc.build_messages(t.recipient, t.amount, t.wire)
    assert np.array_equal(work[:4 * (n + 1)].view(np.uint32), off)
    at = (4 * (n + 1) + 15) // 16 * 16
    assert np.array_equal(work[at:at + n * L], msg)
    assert (work[at + n * L:] == PATTERN).all()  # (the 16 bytes of slack are left alone)
    return (at2v_mod.unpack_verdicts(ver[:-1], n),
            at2v_mod.unpack_verdicts(rok[:-1], n) if recipient_ok else None)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 255, 256, 257, 4096])
def test_device_form_sizes(at2v_mod, plain, n):
    """the wave and block tails of the prep kernel and the word tails of both bitmaps"""
    t = tc.cfg1_mutated().head(n)
    got, rok = device_call(at2v_mod, plain, t)
    assert np.array_equal(got, t.want["dalek"]), np.nonzero(got != t.want["dalek"])[0][:10]
    assert np.array_equal(rok, tc.cfg1_mutated_recipient_ok()[:n])


@pytest.mark.parametrize("n", [1, 65, 256])
def test_device_form_wire_array(at2v_mod, plain, n):
    """the 40-byte stride: messages only 8-byte aligned"""
    t = tc.array_wire().head(n)
    got, rok = device_call(at2v_mod, plain, t)
    assert got.all() and rok.all()
    bytes_form = tc.Transfers(t.sender, t.sig, t.recipient, t.amount, tc.WIRE_BYTES, t.want, t.mutated)
    got, _ = device_call(at2v_mod, plain, bytes_form, recipient_ok=False)
    assert not got.any()


ROUTES = {
    "verify_kernel": (dict(small_batch_max=OFF), 1),
    "verify_pair_kernel": (dict(), 1),
    "sender_tables": (dict(small_batch_max=OFF, sender_cache=1024, admit_first=True), 2),
    "combs_small_batch": (dict(sender_cache=1024, sender_comb=True, admit_first=True), 2),
    "combs_throughput": (dict(small_batch_max=512, sender_cache=1024, sender_comb=True, admit_first=True), 2),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route(at2v_mod, route):
    """the mutated at2_cfg1 set through the device form on every kind of context; cached contexts run it cold and then
    warm (the second pass serves the 64 senders from the cache: tables, the partitioned comb launch, the small-batch
    comb kernel)"""
    opts, passes = ROUTES[route]
    t = tc.cfg1_mutated()
    with at2v_mod.BatchVerifier(**opts) as v:
        for k in range(passes):
            got, rok = device_call(at2v_mod, v, t, recipient_ok=(k == 0))
            assert np.array_equal(got, t.want["dalek"]), (route, k, np.nonzero(got != t.want["dalek"])[0][:10])
            if passes > 1:
                assert v.info()["cache_entries"] > 0, route  # (get_info waits for the builds: pass 2 is warm)


@pytest.mark.parametrize("policy", ["dalek", "libsodium"])
def test_bad_senders_and_signatures(at2v_mod, policy):
    """(pk, sig) of the edge set and of the adversarial classes 3-7 over rebuilt transfer messages, bit for bit"""
    t = tc.bad_senders()
    want = t.want[policy]
    with at2v_mod.BatchVerifier(policy=policy, small_batch_max=512) as v:
        got, _ = device_call(at2v_mod, v, t, recipient_ok=False)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        got = v.verify_transfers(t.sender, t.sig, t.recipient, t.amount)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]


def test_recipient_ok_on_the_device(at2v_mod, plain):
    t, want_rok = tc.recipient_mix()
    v1, rok = device_call(at2v_mod, plain, t, recipient_ok=True)
    v0, _ = device_call(at2v_mod, plain, t, recipient_ok=False)
    assert np.array_equal(rok, want_rok), np.nonzero(rok != want_rok)[0][:10]
    assert np.array_equal(rok, plain.decode_points(t.recipient))
    assert np.array_equal(v0, v1) and np.array_equal(v0, t.want["dalek"])


def test_device_form_argument_errors(at2v_mod, plain):
    import torch
    lib = at2v_mod.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    ws = at2v_mod.BatchVerifier.transfers_workspace_bytes(64, 0)
    args = lambda **kw: [kw.get(k, d) for k, d in (("h", plain._h), ("s", p), ("g", p), ("r", p), ("a", p), ("n", 64),
                                                   ("wire", 0), ("work", p), ("wb", ws), ("v", p), ("rok", p),
                                                   ("st", None))]
    f = lib.at2v_verify_transfers_device
    assert f(*args(wire=2)) == -1 and f(*args(wb=ws - 1)) == -1 and f(*args(work=None)) == -1
    assert f(*args(r=None)) == -1 and f(*args(v=None)) == -1
    assert f(*args(n=(1 << 32) // 48 + 1, wb=1 << 40)) == -1  # n x L >= 2^32
    assert f(*args(s=p + 8)) == -5 and f(*args(r=p + 8)) == -5 and f(*args(a=p + 4)) == -5
    assert f(*args(work=p + 8)) == -5 and f(*args(v=p + 2)) == -5 and f(*args(rok=p + 2)) == -5
    assert f(*args(n=0)) == 0
    torch.cuda.synchronize()
    assert not buf.any()  # nothing ran


@pytest.mark.parametrize("n", [1, 63, 513, 4096])
def test_host_form_eight_shards(at2v_mod, monkeypatch, n):
    monkeypatch.setenv("AT2V_TEST_DEVICE_ALIAS", "1")
    t = tc.cfg1_mutated().head(n)
    words = np.full((n + 31) // 32 + 1, V_SENTINEL, np.uint32)
    rwords = np.full((n + 31) // 32 + 1, R_SENTINEL, np.uint32)
    with at2v_mod.BatchVerifier(num_gpus=8, small_batch_max=OFF) as v:
        got, rok = v.verify_transfers(t.sender, t.sig, t.recipient, t.amount, words=words[:-1],
                                      recipient_words=rwords[:-1])
        assert v.info()["num_gpus"] == 8
    assert np.array_equal(got, t.want["dalek"]), np.nonzero(got != t.want["dalek"])[0][:10]
    assert np.array_equal(rok, tc.cfg1_mutated_recipient_ok()[:n])
    assert words[-1] == V_SENTINEL and rwords[-1] == R_SENTINEL
    if n % 32:
        assert int(words[-2]) >> (n % 32) == 0 and int(rwords[-2]) >> (n % 32) == 0


def carve(block, t):
    """t's four field arrays and two bitmaps (+ a sentinel word each) inside one host_alloc block, 64-byte aligned"""
    out, at = [], 0
    for a in (t.sender, t.sig, t.recipient, t.amount, np.full((t.n + 31) // 32 + 1, V_SENTINEL, np.uint32),
              np.full((t.n + 31) // 32 + 1, R_SENTINEL, np.uint32)):
        view = block[at:at + a.nbytes].view(a.dtype).reshape(a.shape)
        view[...] = a
        out.append(view)
        at += (a.nbytes + 63) // 64 * 64
    return out


def test_host_form_chunks_pinned_and_pageable(at2v_mod, monkeypatch):
    """4,096 records in three chunks (1,024 / 1,024 / 2,048): from host_alloc memory every byte of the four field arrays
    goes direct (n x 136) and nothing is staged; from pageable arrays the same bytes are staged"""
    monkeypatch.setenv("AT2V_TEST_STAGE_FIRST", "1024")
    monkeypatch.setenv("AT2V_TEST_STAGE_MAX", "2048")
    t = tc.cfg1_mutated()
    n = t.n
    with at2v_mod.BatchVerifier(small_batch_max=512) as v:
        block = v.host_alloc(n * 136 + 2 * (n // 32 + 1) * 4 + 6 * 64)
        sender, sig, recipient, amount, words, rwords = carve(block, t)
        i0 = v.info()
        got, rok = v.verify_transfers(sender, sig, recipient, amount, words=words[:-1], recipient_words=rwords[:-1])
        i1 = v.info()
        assert i1["host_chunks"] - i0["host_chunks"] == 3
        assert i1["host_direct_bytes"] - i0["host_direct_bytes"] == n * 136
        assert i1["host_staged_bytes"] - i0["host_staged_bytes"] == 0
        assert np.array_equal(got, t.want["dalek"]), np.nonzero(got != t.want["dalek"])[0][:10]
        assert np.array_equal(rok, tc.cfg1_mutated_recipient_ok())
        assert words[-1] == V_SENTINEL and rwords[-1] == R_SENTINEL
        got, rok = v.verify_transfers(t.sender, t.sig, t.recipient, t.amount, recipient_ok=True)  # pageable
        i2 = v.info()
        assert i2["host_chunks"] - i1["host_chunks"] == 3
        assert i2["host_direct_bytes"] - i1["host_direct_bytes"] == 0
        assert i2["host_staged_bytes"] - i1["host_staged_bytes"] == n * 136
        assert np.array_equal(got, t.want["dalek"]) and np.array_equal(rok, tc.cfg1_mutated_recipient_ok())
        # mixed: recipients and amounts pinned, senders and signatures pageable
        got = v.verify_transfers(t.sender, t.sig, recipient, amount)
        i3 = v.info()
        assert i3["host_direct_bytes"] - i2["host_direct_bytes"] == n * 40
        assert i3["host_staged_bytes"] - i2["host_staged_bytes"] == n * 96
        assert np.array_equal(got, t.want["dalek"])
        v.host_free(block)


def test_two_transfers_calls_in_flight(at2v_mod, monkeypatch):
    monkeypatch.setenv("AT2V_TEST_STAGE_FIRST", "1024")
    monkeypatch.setenv("AT2V_TEST_STAGE_MAX", "2048")
    m = tc.cfg1_mutated()
    t, want_rok = tc.recipient_mix()
    with at2v_mod.BatchVerifier(small_batch_max=512) as v:
        a = v.submit_transfers(m.sender, m.sig, m.recipient, m.amount, recipient_ok=True)
        b = v.submit_transfers(t.sender, t.sig, t.recipient, t.amount, recipient_ok=True)
        assert b.ticket == a.ticket + 1
        got_a, got_b = v.wait_batch(a), v.wait_batch(b)
        assert np.array_equal(got_a, m.want["dalek"]) and np.array_equal(a.recipient_ok(), tc.cfg1_mutated_recipient_ok())
        assert np.array_equal(got_b, t.want["dalek"]) and np.array_equal(b.recipient_ok(), want_rok)
        # a records call and a transfers call together
        msg, off = tc.build_messages(t.recipient, t.amount, tc.WIRE_BYTES)
        c = v.submit_batch(t.sender, t.sig, msg, off)
        d = v.submit_transfers(m.sender, m.sig, m.recipient, m.amount)
        assert np.array_equal(v.wait_batch(d), m.want["dalek"]) and np.array_equal(v.wait_batch(c), t.want["dalek"])


def test_launch_failure_falls_back_or_fails_closed(at2v_mod, monkeypatch):
    """AT2V_TEST_FAIL_LAUNCH fails the first verify launch on the host side, before any kernel of it runs. With
    AT2V_CTX_CPU_FALLBACK the call is verified on the CPU from the caller's fields, recipient_ok included; without it the
    call returns its error and every word of both outputs is 0"""
    monkeypatch.setenv("AT2V_TEST_FAIL_LAUNCH", "1")
    t, want_rok = tc.recipient_mix()
    with at2v_mod.BatchVerifier(cpu_fallback=True, cpu_threads=8) as v:
        got, rok = v.verify_transfers(t.sender, t.sig, t.recipient, t.amount, recipient_ok=True)
        assert np.array_equal(got, t.want["dalek"]) and np.array_equal(rok, want_rok)
        inf = v.info()
        assert inf["cpu_fallbacks"] == 1 and inf["cpu_batches"] == 1
        got, rok = v.verify_transfers(t.sender, t.sig, t.recipient, t.amount, recipient_ok=True)  # on the GPU again
        assert np.array_equal(got, t.want["dalek"]) and np.array_equal(rok, want_rok)
        assert v.info()["cpu_fallbacks"] == 1
    words = np.full((t.n + 31) // 32, 0xFFFFFFFF, np.uint32)
    rwords = np.full((t.n + 31) // 32, 0xFFFFFFFF, np.uint32)
    with at2v_mod.BatchVerifier() as v:
        with pytest.raises(at2v_mod.At2vError) as ei:
            v.verify_transfers(t.sender, t.sig, t.recipient, t.amount, words=words, recipient_words=rwords)
        assert ei.value.code < 0
        assert not words.any() and not rwords.any()
        # ... also when the failed call is submitted and a later submit completes it
    monkeypatch.setenv("AT2V_TEST_FAIL_LAUNCH", "1")
    with at2v_mod.BatchVerifier() as v:
        words[:] = 0xFFFFFFFF
        rwords[:] = 0xFFFFFFFF
        a = v.submit_transfers(t.sender, t.sig, t.recipient, t.amount, words=words, recipient_words=rwords)
        b = v.submit_transfers(t.sender, t.sig, t.recipient, t.amount, recipient_ok=True)
        c = v.submit_transfers(t.sender, t.sig, t.recipient, t.amount, recipient_ok=True)  # completes a
        assert not words.any() and not rwords.any()
        assert at2v_mod.load_library().at2v_verify_batch_wait(v._h, a.ticket) == -1  # its result is gone
        assert np.array_equal(v.wait_batch(b), t.want["dalek"]) and np.array_equal(b.recipient_ok(), want_rok)
        assert np.array_equal(v.wait_batch(c), t.want["dalek"]) and np.array_equal(c.recipient_ok(), want_rok)


def test_eager_gpu_queue_submit_transfers(at2v_mod):
    from at2v.node import IngestQueue
    m = tc.cfg1_mutated()
    a = tc.array_wire()
    with IngestQueue(device=0, max_batch=1024, max_delay_us=300, max_msg_bytes=64, eager=True) as q:
        first = q.submit_transfers(m.sender[:1500], m.sig[:1500], m.recipient[:1500], m.amount[:1500])
        mid = q.submit_transfers(a.sender, a.sig, a.recipient, a.amount, wire=tc.WIRE_ARRAY)
        last = q.submit_transfers(m.sender[1500:], m.sig[1500:], m.recipient[1500:], m.amount[1500:])
        assert mid == first + 1500 and last == mid + a.n
        q.flush()
        total = m.n + a.n
        ts, vs = [], []
        while sum(len(t) for t in ts) < total:
            t, v = q.poll(1 << 16, 5_000_000)
            assert len(t), "queue stalled"
            ts.append(t)
            vs.append(v)
        st = q.stats()
    t, v = np.concatenate(ts), np.concatenate(vs)
    want = np.concatenate([m.want["dalek"][:1500], a.want["dalek"], m.want["dalek"][1500:]])
    assert np.array_equal(t, np.arange(first, first + total, dtype=np.uint64))
    assert not (v == 0xFF).any() and np.array_equal(v.astype(bool), want)
    assert st["failed_batches"] == 0
