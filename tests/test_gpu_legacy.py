"""GPU: AT2V_POLICY_DALEK_V1_LEGACY on every kernel route, and the policy-mask pass (at2v_policy_mask_device /
at2v_policy_mask) behind them, through the C ABI of libat2v.so. Expected values come from tests/legacy_ref.py (the
fixtures' stored columns, the oracle on R || (s - l), Python integers; its own cross-checks are in
tests/test_legacy_cpu.py). Every device launch writes into buffers pre-filled with a sentinel: a word after the verdict
words and 64 guard bytes after byte n - 1 of the mask and of the reasons must survive, pad bits must be 0."""
import numpy as np
import pytest

import legacy_ref as lr
import reason_ref as rr

pytestmark = pytest.mark.gpu

GUARD = 64
SENT8, SENT32 = 0xA5, 0x5AA55AA5
SIZES = [1, 63, 64, 65, 129]


@pytest.fixture(scope="module")
def at2v_mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import at2v
    at2v.load_library()
    return at2v


@pytest.fixture(scope="module")
def cases(golden, oracle):
    c = lr.constructed(oracle, golden["at2_cfg1"])
    # one wave holds s < l, an accepted l <= s < 2^253, a rejected s >= 2^253 and an undecodable A
    assert {(x.mask, x.reasons[2]) for x in c} >= {(7, 0), (4, 0), (0, 2), (0, 1)} and len(c) <= 64
    return c


class Records:
    def __init__(self, pk, sig, msg, off):
        self.pk, self.sig, self.msg, self.off = pk, sig, msg, np.asarray(off, np.uint32)
        self.n = len(pk)


class Data(Records):
    """records and everything expected of them under the legacy policy (computed once, read-only)"""

    def __init__(self, pk, sig, msg, off, valid):
        super().__init__(pk, sig, msg, off)
        self.valid = np.asarray(valid, bool)
        self.reasons = lr.reasons_legacy(pk, sig, self.valid)
        self.mask = lr.masks_expected(pk, sig, self.valid)
        for a in (self.valid, self.reasons, self.mask):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def data(golden, oracle, cases):
    out = {}
    for name in ("edge", "adversarial"):
        g = golden[name]
        out[name] = Data(g.pk, g.sig, g.msg, g.off, lr.legacy_expected_set(oracle, g))
    for n in SIZES + [513]:
        t = lr.tile(cases, n)
        out[n] = Data(*lr.pack(t), [c.verdicts[2] for c in t])
        assert out[n].mask.tolist() == [c.mask for c in t] and out[n].reasons.tolist() == [c.reasons[2] for c in t]
    a = out["adversarial"]
    cls = np.array([lr.in_class(a.sig[i].tobytes()) for i in range(a.n)])
    assert cls.sum() == 109 and (cls & a.valid).sum() == 108
    return out


ROUTES = {  # BatchVerifier arguments; launches per data set (a cache serves the second)
    "throughput": (dict(small_batch_max=0xFFFFFFFF), 1),
    "pair": (dict(), 1),
    "tables_cached_and_miss": (dict(small_batch_max=0xFFFFFFFF, sender_cache=1024, admit_first=True), 2),
    "comb_hit_list": (dict(small_batch_max=0xFFFFFFFF, sender_cache=1024, sender_comb=True, admit_first=True), 2),
    "comb_hit_list_wide": (dict(small_batch_max=0xFFFFFFFF, sender_cache=1024, sender_comb=True, admit_first=True,
                                bcomb_wide=True), 2),  # the 24-bit comb of B instead of the 20-bit one
    "comb_low_latency": (dict(sender_cache=1024, sender_comb=True, admit_first=True), 2),  # the 16-bit comb of B
}


@pytest.fixture(scope="module")
def verifiers(at2v_mod):
    vs = {}
    yield lambda r: vs.get(r) or vs.setdefault(r, at2v_mod.BatchVerifier(device=0, policy="dalek-legacy", **ROUTES[r][0]))
    for v in vs.values():
        v.close()


def device_pass(v, d, mask=True, reasons=True):
    """one verify_batch_device launch, then the mask pass and the reasons pass right behind it on the same stream ->
    (bool[n] verdicts, u8[n] mask, u8[n] reasons); checks pad bits, the sentinel word and the guard bytes"""
    import torch
    import at2v
    n = d.n
    off = (d.off[:n + 1] - d.off[0]).astype(np.uint32)
    mb = int(off[-1])
    m = np.zeros(mb + 16, np.uint8)
    m[:mb] = np.asarray(d.msg, np.uint8)[int(d.off[0]):int(d.off[0]) + mb]
    dev = "cuda:0"
    d_pk = torch.from_numpy(np.ascontiguousarray(d.pk, np.uint8).reshape(-1).copy()).to(dev)
    d_sig = torch.from_numpy(np.ascontiguousarray(d.sig, np.uint8).reshape(-1).copy()).to(dev)
    d_msg = torch.from_numpy(m).to(dev)
    d_off = torch.from_numpy(off.view(np.int32).copy()).to(dev)
    nwords = (n + 31) // 32
    d_ver = torch.from_numpy(np.full(nwords + 1, SENT32, np.uint32).view(np.int32)).to(dev)
    d_mask = torch.full((n + GUARD,), SENT8, dtype=torch.uint8, device=dev)
    d_rea = torch.full((n + GUARD,), SENT8, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    v.verify_batch_device(d_pk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), mb, d_off.data_ptr(), n,
                          d_ver.data_ptr(), s)
    if mask:
        v.policy_mask_device(d_pk.data_ptr(), d_sig.data_ptr(), n, d_ver.data_ptr(), d_mask.data_ptr(), s)
    if reasons:
        v.reject_reasons_device(d_pk.data_ptr(), d_sig.data_ptr(), n, d_ver.data_ptr(), d_rea.data_ptr(), s)
    torch.cuda.synchronize()
    words = d_ver.cpu().numpy().view(np.uint32)
    assert words[nwords] == SENT32, "the word after the verdict words was written"
    if n % 32:
        assert words[nwords - 1] >> (n % 32) == 0, "pad bits"
    got_m, got_r = d_mask.cpu().numpy(), d_rea.cpu().numpy()
    assert (got_m[n if mask else 0:] == SENT8).all(), "a byte at or after mask + n was written"
    assert (got_r[n if reasons else 0:] == SENT8).all(), "a byte at or after reasons + n was written"
    return at2v.unpack_verdicts(words, n), got_m[:n], got_r[:n]


def check(d, got, what):
    ok, mask, rea = got
    assert np.array_equal(ok, d.valid), (what, np.nonzero(ok != d.valid)[0][:8])
    assert np.array_equal(mask, d.mask), (what, np.nonzero(mask != d.mask)[0][:8])
    assert np.array_equal(rea, d.reasons), (what, np.nonzero(rea != d.reasons)[0][:8])


@pytest.mark.parametrize("key", SIZES + ["edge", "adversarial"], ids=str)
@pytest.mark.parametrize("route", list(ROUTES))
def test_routes(verifiers, data, route, key):
    """verdicts, mask bytes and reason bytes on every kernel route; a route with a sender cache is launched cold, then
    warm (the second launch takes the senders it cached from their tables or combs)"""
    v, d = verifiers(route), data[key]
    hits = lambda: sum(v.info()[k] for k in ("cache_record_hits", "cache_chunk_hits"))
    for launch in range(ROUTES[route][1]):
        before = hits()
        check(d, device_pass(v, d), (route, key, launch))
        if launch and key in SIZES:  # the tiles' three senders were cached by the cold launch at the latest
            assert hits() > before, "the warm launch took no sender from the cache"


def test_mask_bits_reproduce_the_stored_columns(verifiers, golden):
    """the strong check on the device: bit 0 is the stored verdict_dalek column (OpenSSL), bit 1 verdict_sodium
    (libsodium), bit for bit, on all 13,220 fixture records"""
    v = verifiers("throughput")
    total = 0
    for name, g in golden.items():
        ok = v.verify_batch(g.pk, g.sig, g.msg, g.off)
        _, mask, _ = device_pass(v, Records(g.pk, g.sig, g.msg, g.off), reasons=False)
        assert np.array_equal((mask & 1).astype(bool), g.dalek), name
        assert np.array_equal((mask & 2).astype(bool), g.sodium), name
        assert np.array_equal((mask & 4).astype(bool), ok), name
        total += g.n
    assert total == 13220


def test_mask_host_form_alignment_and_other_policies(at2v_mod, verifiers, data):
    import torch
    v = verifiers("throughput")
    lib = at2v_mod.load_library()
    for key in ("adversarial", 65):
        d = data[key]
        ok = v.verify_batch(d.pk, d.sig, d.msg, d.off)  # a host-buffer call
        assert np.array_equal(ok, d.valid)
        got = v.policy_mask(d.pk, d.sig, ok)
        assert np.array_equal(got, d.mask) and np.array_equal(got, device_pass(v, d)[1])
        assert np.array_equal(v.reject_reasons(d.pk, d.sig, ok), d.reasons)
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    with pytest.raises(at2v_mod.At2vError) as e:
        v.policy_mask_device(p, p, 1, p, p + 1)
    assert e.value.code == -5
    d = data[65]
    pk, sig = np.ascontiguousarray(d.pk), np.ascontiguousarray(d.sig)
    words = np.full(3, 0xFFFFFFFF, np.uint32)
    for pname in ("dalek", "libsodium"):
        with at2v_mod.BatchVerifier(device=0, policy=pname) as o:
            host = np.full(d.n + 16, SENT8, np.uint8)
            assert lib.at2v_policy_mask(o._h, pk.ctypes.data, sig.ctypes.data, d.n, words.ctypes.data,
                                        host.ctypes.data) == -1
            assert (host == SENT8).all()
            dm = torch.full((256,), SENT8, dtype=torch.uint8, device="cuda:0")
            assert lib.at2v_policy_mask_device(o._h, p, p, 1, p, dm.data_ptr(), None) == -1
            torch.cuda.synchronize()
            assert (dm.cpu().numpy() == SENT8).all()


def test_mask_host_form_device_error(at2v_mod, data, monkeypatch):
    """the launch-failure hook reaches the pass's own launch: without the fallback flag a negative code and every byte
    0; with AT2V_CTX_CPU_FALLBACK AT2V_OK and exact bytes from the CPU pool"""
    d = data["edge"]
    lib = at2v_mod.load_library()
    words = rr.words_of(d.valid)
    monkeypatch.setenv("AT2V_TEST_FAIL_LAUNCH", "1")
    pk, sig = np.ascontiguousarray(d.pk), np.ascontiguousarray(d.sig)
    with at2v_mod.BatchVerifier(policy="dalek-legacy") as v:
        buf = np.full(d.n + GUARD, SENT8, np.uint8)
        assert lib.at2v_policy_mask(v._h, pk.ctypes.data, sig.ctypes.data, d.n, words.ctypes.data, buf.ctypes.data) < 0
        assert not buf[:d.n].any() and (buf[d.n:] == SENT8).all()
        assert np.array_equal(v.policy_mask(d.pk, d.sig, words), d.mask)  # the next call runs on the device
    with at2v_mod.BatchVerifier(policy="dalek-legacy", cpu_fallback=True, cpu_threads=4) as v:
        assert np.array_equal(v.policy_mask(d.pk, d.sig, words), d.mask)  # on the CPU pool
        assert np.array_equal(v.policy_mask(d.pk, d.sig, words), d.mask)  # on the device


def test_transfers(at2v_mod, verifiers, oracle):
    snd, sig, rcp, amt = (np.tile(a, (65,) + (1,) * (a.ndim - 1))[:129] for a in lr.transfer_pair(oracle))
    for route in ("throughput", "pair"):
        assert verifiers(route).verify_transfers(snd, sig, rcp, amt).all(), route
    with at2v_mod.BatchVerifier(device=0, policy="dalek") as v:
        assert v.verify_transfers(snd, sig, rcp, amt).tolist() == [i % 2 == 0 for i in range(129)]


def test_eight_aliased_shards(at2v_mod, data, monkeypatch):
    monkeypatch.setenv("AT2V_TEST_DEVICE_ALIAS", "1")
    d = data[513]
    a = data["adversarial"]
    with at2v_mod.BatchVerifier(num_gpus=8, policy="dalek-legacy", small_batch_max=0xFFFFFFFF) as v:
        assert np.array_equal(v.verify_batch(d.pk, d.sig, d.msg, d.off), d.valid)
        lo = a.n - 513  # (the class is spread over the set)
        ok = v.verify_batch(a.pk[lo:], a.sig[lo:], a.msg[int(a.off[lo]):], a.off[lo:] - a.off[lo])
        assert np.array_equal(ok, a.valid[lo:])


@pytest.mark.parametrize("reasons", [False, True])
def test_eager_queue_of_65(data, reasons):
    from at2v.node import IngestQueue
    d = data[65]
    with IngestQueue(device=0, policy="dalek-legacy", max_batch=1024, eager=True, reasons=reasons) as q:
        first = q.submit(d.pk, d.sig, d.msg, d.off)
        q.flush()
        tickets, got = [], []
        while len(tickets) < d.n:
            t, r = q.poll_reasons(4096, 5_000_000) if reasons else q.poll(4096, 5_000_000)
            assert len(t), "queue stalled"
            tickets += t.tolist()
            got += r.tolist()
        assert tickets == list(range(first, first + d.n))
        assert got == (d.reasons.tolist() if reasons else d.valid.astype(int).tolist())
        assert q.stats()["failed_batches"] == 0


def test_old_policies_still_reproduce_the_stored_columns(at2v_mod, golden):
    g = golden["adversarial"]
    for pname, col in (("dalek", g.dalek), ("libsodium", g.sodium)):
        for small in (0xFFFFFFFF, 0):  # the throughput kernel, the pair kernel
            with at2v_mod.BatchVerifier(device=0, policy=pname, small_batch_max=small) as v:
                ok, _, _ = device_pass(v, Records(g.pk, g.sig, g.msg, g.off), mask=False, reasons=False)
                assert np.array_equal(ok, col), (pname, small)
