"""GPU: host-buffer calls on pinned caller memory (ABI 9: at2v_host_alloc / at2v_host_register, include/at2v.h). A
slice of pk, sig or msg that lies wholly inside one range the context knows is uploaded straight from the caller's memory
(csrc/at2v_api_pipe.h issue_chunk); everything else takes the staging slot as before. Every test compares record by record
with the stored golden verdicts or with the oracle, and checks at2v_info.host_direct_bytes / host_staged_bytes exactly:
a slice that silently took the other path fails the test even where the verdicts agree.

Sizes: the golden sets (one chunk each), and 8,003 adversarial records with the schedule hooks AT2V_TEST_STAGE_FIRST=1024 /
AT2V_TEST_STAGE_MAX=2048 and small_batch_max = 512, which gives five chunks of 1,024 / 1,024 / 2,048 / 2,048 / 1,859
records: all three staging slots are reused and the last chunk has a ragged tail."""
import numpy as np
import pytest

import golden_io
import pinned_layout

pytestmark = pytest.mark.gpu

N = 8003
MSG_LEN = 60
CHUNKS = (1024, 1024, 2048, 2048, 1859)


@pytest.fixture(scope="module")
def at2v_mod():
    import at2v
    at2v.load_library()
    return at2v


@pytest.fixture(scope="module")
def records(oracle):
    """(pk, sig, msg, off, want) of the two adversarial batches, computed once and never written to"""
    out = []
    for seed in (0x9137, 0x9138):
        pk, sig, msg, off, cls = oracle.gen_adversarial(seed, 0, N, MSG_LEN)
        want = oracle.verify_batch(pk, sig, msg, off)
        assert 0 < want.sum() < N
        for a in (pk, sig, msg, off, want):
            a.setflags(write=False)
        out.append((pk, sig, msg, off, want))
    return out


@pytest.fixture()
def chunked(monkeypatch):
    monkeypatch.setenv("AT2V_TEST_STAGE_FIRST", "1024")
    monkeypatch.setenv("AT2V_TEST_STAGE_MAX", "2048")


def record_bytes(off, n):
    return 96 * n + int(off[n]) - int(off[0])


class Counters:
    """the growth of (host_direct_bytes, host_staged_bytes) since the last look"""

    def __init__(self, v):
        self.v = v
        self.last = self._now()

    def _now(self):
        inf = self.v.info()
        return inf["host_direct_bytes"], inf["host_staged_bytes"]

    def delta(self):
        now = self._now()
        d = (now[0] - self.last[0], now[1] - self.last[1])
        self.last = now
        return d


def off_page(a: np.ndarray) -> np.ndarray:
    """a copy of `a` at an address that is 24 bytes past a page boundary (plain pageable numpy memory)"""
    buf = np.empty(a.nbytes + 8192, np.uint8)
    start = (-buf.ctypes.data) % 4096 + 24
    out = buf[start:start + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    assert out.ctypes.data % 4096 == 24
    return out


def carved_call(at2v_mod, v, c, want, what=""):
    got = v.verify_batch(c.pk, c.sig, c.msg, c.off, words=c.verdict_words())
    assert np.array_equal(got, want), (what, np.nonzero(got != want)[0][:10])
    assert np.array_equal(at2v_mod.unpack_verdicts(c.verdict_words(), c.n), want), what
    pinned_layout.check_words(c)


@pytest.mark.parametrize("policy", ["dalek", "libsodium"])
def test_golden_sets_allocated_memory(at2v_mod, golden, policy):
    """each golden set with the whole batch in one host_alloc range (messages at an odd address, msg_off[0] > 0, the
    verdict words pinned too): stored verdicts, pad bits 0, sentinel untouched, every pk/sig/msg byte direct"""
    with at2v_mod.BatchVerifier(policy=policy) as v:
        cnt = Counters(v)
        for name in golden_io.SETS:
            g = golden[name]
            block = v.host_alloc(pinned_layout.carved_bytes(g.n, len(g.msg)))
            c = pinned_layout.carve(block, g.pk, g.sig, g.msg, g.off)
            carved_call(at2v_mod, v, c, g.dalek if policy == "dalek" else g.sodium, name)
            assert cnt.delta() == (record_bytes(g.off, g.n), 0), name
            v.host_free(block)
        assert v.info()["num_gpus"] == 1


@pytest.mark.parametrize("policy", ["dalek", "libsodium"])
def test_golden_sets_registered_memory(at2v_mod, golden, policy):
    """the same from plain numpy arrays, not page-aligned, passed to host_register; after host_unregister a further call
    over the same arrays is staged and gives the same verdicts"""
    with at2v_mod.BatchVerifier(policy=policy) as v:
        cnt = Counters(v)
        for name in golden_io.SETS:
            g = golden[name]
            want = g.dalek if policy == "dalek" else g.sodium
            pk, sig = off_page(g.pk), off_page(g.sig)
            msg = off_page(np.concatenate([np.full(5, 0x5A, np.uint8), g.msg]))  # msg_off[0] = 5
            off = g.off + np.uint32(5)
            words = np.full((g.n + 31) // 32 + 1, pinned_layout.SENTINEL, np.uint32)
            arrays = (pk, sig, msg, words)
            for a in arrays:
                v.host_register(a)
            got = v.verify_batch(pk, sig, msg, off, words=words[:-1])
            assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:10])
            assert words[-1] == pinned_layout.SENTINEL
            if g.n % 32:
                assert int(words[(g.n - 1) // 32]) >> (g.n % 32) == 0
            assert cnt.delta() == (record_bytes(off, g.n), 0), name
            for a in arrays:
                v.host_unregister(a)
            got = v.verify_batch(pk, sig, msg, off)
            assert np.array_equal(got, want), (name, "staged", np.nonzero(got != want)[0][:10])
            assert cnt.delta() == (0, record_bytes(off, g.n)), name


def test_several_chunks_sync_and_two_in_flight(at2v_mod, records, chunked):
    """five chunks per call (1,024 / 1,024 / 2,048 / 2,048 / 1,859): twice synchronously through one context, then two
    batches in flight through submit / submit / wait / wait; record by record against the oracle, counters exact"""
    (pk, sig, msg, off, want), (pk2, sig2, msg2, off2, want2) = records
    with at2v_mod.BatchVerifier(small_batch_max=512) as v:
        a = pinned_layout.carve(v.host_alloc(pinned_layout.carved_bytes(N, len(msg))), pk, sig, msg, off)
        b = pinned_layout.carve(v.host_alloc(pinned_layout.carved_bytes(N, len(msg2))), pk2, sig2, msg2, off2)
        cnt = Counters(v)
        chunks0 = v.info()["host_chunks"]
        for rep in range(2):
            carved_call(at2v_mod, v, a, want, rep)
            assert cnt.delta() == (record_bytes(off, N), 0), rep
        assert v.info()["host_chunks"] - chunks0 == 2 * len(CHUNKS)
        pa = v.submit_batch(a.pk, a.sig, a.msg, a.off, words=a.verdict_words())
        pb = v.submit_batch(b.pk, b.sig, b.msg, b.off, words=b.verdict_words())
        got_a, got_b = v.wait_batch(pa), v.wait_batch(pb)
        assert np.array_equal(got_a, want), np.nonzero(got_a != want)[0][:10]
        assert np.array_equal(got_b, want2), np.nonzero(got_b != want2)[0][:10]
        pinned_layout.check_words(a)
        pinned_layout.check_words(b)
        assert cnt.delta() == (record_bytes(off, N) + record_bytes(off2, N), 0)


def test_mixed_arrays(at2v_mod, records, chunked):
    """pk pinned, sig and msg pageable: 32 n bytes direct, the rest staged; then a wholly pageable call through the same
    context (it shares the slots and the device arena with the direct one before it)"""
    pk, sig, msg, off, want = records[0]
    with at2v_mod.BatchVerifier(small_batch_max=512) as v:
        block = v.host_alloc(32 * N)
        p_pk = block.reshape(N, 32)
        p_pk[:] = pk
        cnt = Counters(v)
        got = v.verify_batch(p_pk, sig, msg, off)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        assert cnt.delta() == (32 * N, 64 * N + int(off[N]) - int(off[0]))
        # a fully direct call, then a pageable one right after it
        c = pinned_layout.carve(v.host_alloc(pinned_layout.carved_bytes(N, len(msg))), pk, sig, msg, off)
        carved_call(at2v_mod, v, c, want, "direct")
        assert cnt.delta() == (record_bytes(off, N), 0)
        got = v.verify_batch(pk, sig, msg, off)
        assert np.array_equal(got, want), ("pageable", np.nonzero(got != want)[0][:10])
        assert cnt.delta() == (0, record_bytes(off, N))


def test_chunks_with_empty_messages(at2v_mod, oracle, chunked):
    """4,096 records whose messages are all empty, in three chunks (1,024 / 1,024 / 2,048): a chunk without message bytes
    has no messages upload (pk, then sig with the offsets; from host_alloc memory pk, sig, then the offsets). Once from
    pageable arrays and once from one host_alloc range with msg_off[0] = 3; verdicts against the oracle"""
    n = 4096
    pk, sig, msg, off, cls = oracle.gen_adversarial(0x9139, 0, n, 0)
    want = oracle.verify_batch(pk, sig, msg, off)
    assert msg.size == 0 and 0 < want.sum() < n
    with at2v_mod.BatchVerifier(small_batch_max=512) as v:
        cnt = Counters(v)
        chunks0 = v.info()["host_chunks"]
        got = v.verify_batch(pk, sig, msg, off)
        assert np.array_equal(got, want), ("pageable", np.nonzero(got != want)[0][:10])
        assert cnt.delta() == (0, 96 * n)
        c = pinned_layout.carve(v.host_alloc(pinned_layout.carved_bytes(n, 0)), pk, sig, msg, off)
        assert c.msg_bytes == 0 and c.off[0] == 3
        carved_call(at2v_mod, v, c, want, "host_alloc")
        assert cnt.delta() == (96 * n, 0)
        assert v.info()["host_chunks"] - chunks0 == 2 * 3


def test_messages_straddling_the_end_of_a_range(at2v_mod, records, chunked):
    """msg registered only up to the middle of the third chunk's messages: the first two chunks' messages go direct, the
    straddling chunk's and every later chunk's are staged; pk and sig are pageable"""
    pk, sig, msg, off, want = records[0]
    msg = off_page(msg)
    first3 = sum(CHUNKS[:2])                          # the third chunk's first record
    cut = int(off[first3 + CHUNKS[2] // 2]) + 7       # inside a message in the middle of the third chunk
    assert int(off[first3]) < cut < int(off[first3 + CHUNKS[2]])
    with at2v_mod.BatchVerifier(small_batch_max=512) as v:
        v.host_register(msg[:cut])
        cnt = Counters(v)
        got = v.verify_batch(pk, sig, msg, off)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        direct = int(off[first3]) - int(off[0])
        assert cnt.delta() == (direct, record_bytes(off, N) - direct)
        v.host_unregister(msg)


def test_unregister_completes_the_call_in_flight(at2v_mod, records, chunked):
    """host_unregister / host_free while a submitted call is in flight: the call is completed first, and its result stays
    for its wait"""
    pk, sig, msg, off, want = records[1]
    pk, sig, msg = off_page(pk), off_page(sig), off_page(msg)
    with at2v_mod.BatchVerifier(small_batch_max=512) as v:
        block = v.host_alloc(4 * ((N + 31) // 32))
        for a in (pk, sig, msg):
            v.host_register(a)
        cnt = Counters(v)
        p = v.submit_batch(pk, sig, msg, off, words=block.view(np.uint32))
        for a in (pk, sig, msg):
            v.host_unregister(a)
        got = v.wait_batch(p)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        assert cnt.delta() == (record_bytes(off, N), 0)
        words = p.words.copy()
        v.host_free(block)
        assert np.array_equal(at2v_mod.unpack_verdicts(words, N), want)


def test_eight_aliased_shards(at2v_mod, records, chunked, monkeypatch):
    """one context over 8 shards (AT2V_TEST_DEVICE_ALIAS: all on the devices present), allocated memory visible to every
    shard's device: against the oracle, counters summed over the shards"""
    monkeypatch.setenv("AT2V_TEST_DEVICE_ALIAS", "1")
    pk, sig, msg, off, want = records[0]
    with at2v_mod.BatchVerifier(num_gpus=8, small_batch_max=512) as v:
        assert v.info()["num_gpus"] == 8
        c = pinned_layout.carve(v.host_alloc(pinned_layout.carved_bytes(N, len(msg))), pk, sig, msg, off)
        cnt = Counters(v)
        for rep in range(2):
            carved_call(at2v_mod, v, c, want, rep)
            assert cnt.delta() == (record_bytes(off, N), 0), rep


def test_sharded_call_world1(at2v_mod, records, chunked):
    """at2v_verify_batch_sharded (one rank) issues its chunks through the same code: direct from allocated memory"""
    pk, sig, msg, off, want = records[1]
    with at2v_mod.BatchVerifier(small_batch_max=512) as v:
        v.comm_init_rank(at2v_mod.comm_unique_id(), 0, 1)
        c = pinned_layout.carve(v.host_alloc(pinned_layout.carved_bytes(N, len(msg))), pk, sig, msg, off)
        cnt = Counters(v)
        got = v.verify_batch_sharded(c.pk, c.sig, c.msg, c.off, words=c.verdict_words())
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        pinned_layout.check_words(c)
        assert cnt.delta() == (record_bytes(off, N), 0)


def test_unknown_pinned_memory_is_staged(at2v_mod, records):
    """memory that is pinned but was never handed to the context (a torch pinned tensor) behaves as before: staged"""
    import torch
    pk, sig, msg, off, want = records[0]
    t = torch.empty(32 * N, dtype=torch.uint8).pin_memory()
    t_pk = t.numpy().reshape(N, 32)
    t_pk[:] = pk
    with at2v_mod.BatchVerifier() as v:
        cnt = Counters(v)
        got = v.verify_batch(t_pk, sig, msg, off)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        assert cnt.delta() == (0, record_bytes(off, N))


def test_error_cases_on_a_gpu_context(at2v_mod):
    import ctypes
    lib = at2v_mod.load_library()
    with at2v_mod.BatchVerifier() as v:
        out = ctypes.c_void_p()
        assert lib.at2v_host_alloc(v._h, 0, ctypes.byref(out)) == -1
        a = v.host_alloc(1000)
        assert a.ctypes.data % 64 == 0
        buf = np.zeros(10000, np.uint8)
        v.host_register(buf[100:5000])
        assert lib.at2v_host_register(v._h, buf.ctypes.data + 4999, 10) == -1       # overlaps a known range
        assert lib.at2v_host_register(v._h, a.ctypes.data + 10, 10) == -1            # inside an allocation
        assert lib.at2v_host_unregister(v._h, buf.ctypes.data + 101) == -1           # interior pointer
        assert lib.at2v_host_free(v._h, buf.ctypes.data + 100) == -1                 # registered, not allocated
        assert lib.at2v_host_unregister(v._h, a.ctypes.data) == -1                   # allocated, not registered
        v.host_register(buf[5000:6000])                                              # adjacent is fine
        v.host_unregister(buf[100:5000])
        assert lib.at2v_host_unregister(v._h, buf.ctypes.data + 100) == -1           # twice
        v.host_free(a)
        assert lib.at2v_host_free(v._h, a.ctypes.data) == -1                         # double free
        # buf[5000:6000] is still registered: at2v_destroy unregisters it
