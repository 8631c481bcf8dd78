"""GPU: AT2V_POLICY_ZIP215 (the cofactored rule) on every kernel route through the C ABI of libat2v.so. Expected verdicts and
reasons come from tests/zip215_ref.py (Python integers on the full-length equation; its own cross-checks are in
tests/test_zip215_cpu.py), never from the library. Records are the constructed set tiled with the `edge` fixture, so one
wave holds an undecodable A, torsion shifts of order 8, a non-canonical R and plain valid records. Every device launch
writes into buffers pre-filled with a sentinel: the word after the verdict words and 64 guard bytes after byte n - 1 of
the reasons must survive, pad bits must be 0."""
import numpy as np
import pytest

import legacy_ref as lr
import reason_ref as rr
import zip215_ref as zr

pytestmark = pytest.mark.gpu

GUARD = 64
SENT8, SENT32 = 0xA5, 0x5AA55AA5
OFF = 0xFFFFFFFF  # AT2V_SMALL_BATCH_OFF
ZIP = zr.POLICIES.index(zr.ZIP215)


@pytest.fixture(scope="module")
def at2v_mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import at2v
    at2v.load_library()
    return at2v


class Data:
    """records and what every policy makes of them: valid bool[n, 4], reasons u8[n, 4] (columns as zr.POLICIES)"""

    def __init__(self, pk, sig, msg, off, valid):
        self.pk, self.sig, self.msg, self.off = pk, sig, msg, np.asarray(off, np.uint32)
        self.n = len(pk)
        self.valid = np.asarray(valid, bool).reshape(self.n, 4)
        self.reasons = np.stack([zr.reasons(pk, sig, self.valid[:, c], p) for c, p in enumerate(zr.POLICIES)], axis=1)
        self.valid.setflags(write=False)
        self.reasons.setflags(write=False)


SIZES = [1, 20, 31, 32, 33, 63, 64, 65, 129, 255, 256, 257]


@pytest.fixture(scope="module")
def data(golden, oracle):
    """"constructed": the 196-case matrix, the torsion-shifted signatures, the negative cases (221 records); "edge": the
    fixture (609); n in SIZES: n records alternating between the 25 constructed records outside the matrix and `edge`"""
    g = golden["edge"]
    cases = zr.constructed()
    small = zr.constructed(matrix=False)
    assert len(cases) == 221 and len(small) == 25
    edge_valid = np.stack([g.dalek, g.sodium, lr.legacy_expected_set(oracle, g), zr.stored("edge", g.n)], axis=1)
    out = {"constructed": Data(*zr.pack(cases), [c.verdicts for c in cases]),
           "edge": Data(g.pk, g.sig, g.msg, g.off, edge_valid)}
    for n in SIZES:
        pk, sig, msgs, valid = [], [], [], []
        for i in range(n):
            if i % 2 == 0:
                c = small[(i // 2) % len(small)]
                pk.append(c.pk), sig.append(c.sig), msgs.append(c.msg), valid.append(c.verdicts)
            else:
                j = (i // 2) % g.n
                pk.append(g.pk[j].tobytes()), sig.append(g.sig[j].tobytes()), msgs.append(g.message(j))
                valid.append(edge_valid[j])
        off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint32)
        out[n] = Data(np.frombuffer(b"".join(pk), np.uint8).reshape(n, 32).copy(),
                      np.frombuffer(b"".join(sig), np.uint8).reshape(n, 64).copy(),
                      np.frombuffer(b"".join(msgs), np.uint8).copy(), off, valid)
    w = out[64]  # one wave: an undecodable A, shifts that only the cofactored rule takes, a non-canonical R, valid records
    assert rr.A_DECODE in w.reasons[:, ZIP] and (w.valid[:, ZIP] & ~w.valid[:, 0]).sum() >= 17
    assert (w.valid[:, 0]).any() and (~w.valid[:, ZIP]).any()
    assert out["constructed"].valid[:196, ZIP].all()  # ZIP-215 accepts the whole matrix
    return out


def device_pass(v, d, reasons=True):
    """one verify_batch_device launch, then the reasons pass behind it on the same stream -> (bool[n] verdicts, u8[n]
    reasons); checks pad bits, the sentinel word and the guard bytes"""
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
    d_rea = torch.full((n + GUARD,), SENT8, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    v.verify_batch_device(d_pk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), mb, d_off.data_ptr(), n,
                          d_ver.data_ptr(), s)
    if reasons:
        v.reject_reasons_device(d_pk.data_ptr(), d_sig.data_ptr(), n, d_ver.data_ptr(), d_rea.data_ptr(), s)
    torch.cuda.synchronize()
    words = d_ver.cpu().numpy().view(np.uint32)
    assert words[nwords] == SENT32, "the word after the verdict words was written"
    if n % 32:
        assert words[nwords - 1] >> (n % 32) == 0, "pad bits"
    got_r = d_rea.cpu().numpy()
    assert (got_r[n if reasons else 0:] == SENT8).all(), "a byte at or after reasons + n was written"
    return at2v.unpack_verdicts(words, n), got_r[:n]


def check(d, got, what, col=ZIP):
    ok, rea = got
    assert np.array_equal(ok, d.valid[:, col]), (what, np.nonzero(ok != d.valid[:, col])[0][:8])
    assert np.array_equal(rea, d.reasons[:, col]), (what, np.nonzero(rea != d.reasons[:, col])[0][:8])


ROUTES = {  # BatchVerifier arguments; data sets; launches per data set (a cache serves the second)
    "joint_throughput": (dict(small_batch_max=OFF), [1, 63, 64, 65, 129, "constructed", "edge"], 1),
    "pair": (dict(), [1, 31, 32, 33, "constructed", "edge"], 1),
    "tables_cold_then_warm": (dict(small_batch_max=OFF, sender_cache=1024, admit_first=True), ["constructed", "edge"], 2),
    "comb_throughput": (dict(small_batch_max=OFF, sender_cache=1024, sender_comb=True, admit_first=True),
                        [1, 255, 256, 257, "constructed", "edge"], 2),  # four records per lane
    "comb_throughput_wide": (dict(small_batch_max=OFF, sender_cache=1024, sender_comb=True, admit_first=True,
                                  bcomb_wide=True), [257, "constructed"], 2),  # the 24-bit comb of B
    "comb_four_wave": (dict(sender_cache=1024, sender_comb=True, admit_first=True), [1, 20, 64, "constructed"], 2),
}


@pytest.fixture(scope="module")
def verifiers(at2v_mod):
    vs = {}
    yield lambda r: vs.get(r) or vs.setdefault(r, at2v_mod.BatchVerifier(device=0, policy="zip215", **ROUTES[r][0]))
    for v in vs.values():
        v.close()


@pytest.mark.parametrize("route,key", [(r, k) for r, (_, keys, _) in ROUTES.items() for k in keys], ids=str)
def test_routes(verifiers, data, route, key):
    """verdicts and reason bytes on every kernel route; a route with a sender cache is launched cold, then warm (the
    second launch takes the senders it cached from their tables or combs)"""
    v, d = verifiers(route), data[key]
    assert v.policy == 4
    hits = lambda: sum(v.info()[k] for k in ("cache_record_hits", "cache_chunk_hits"))
    for launch in range(ROUTES[route][2]):
        before = hits()
        check(d, device_pass(v, d), (route, key, launch))
        if launch:
            assert hits() > before, "the warm launch took no sender from the cache"


def test_unpartitioned_comb_kernel(at2v_mod, data, monkeypatch):
    """verify_kernel_comb (a whole chunk of 256 records from combs, one inversion for four records under the other
    policies, none under this one): the launch form without the classify pass"""
    monkeypatch.setenv("AT2V_CACHE_PARTITION", "0")
    with at2v_mod.BatchVerifier(device=0, policy="zip215", small_batch_max=OFF, sender_cache=1024, sender_comb=True,
                                admit_first=True) as v:
        for key in (257, "edge"):
            for launch in range(2):
                before = v.info()["cache_chunk_hits"]
                check(data[key], device_pass(v, data[key]), (key, launch))
        assert v.info()["cache_chunk_hits"] > before


@pytest.mark.parametrize("comb", [False, True], ids=["tables", "combs"])
def test_partitioned_launch_half_the_senders_cached(at2v_mod, data, comb):
    d = data["edge"]
    keys = np.unique(np.ascontiguousarray(d.pk).reshape(-1, 32), axis=0)
    with at2v_mod.BatchVerifier(device=0, policy="zip215", small_batch_max=64, sender_cache=256,
                                sender_comb=comb) as v:
        v.sender_preload(keys[::2])
        h0 = v.info()["cache_record_hits"]
        check(d, device_pass(v, d), ("partitioned", comb))
        hits = v.info()["cache_record_hits"] - h0
        assert 0 < hits < d.n  # both lists were non-empty


def test_eight_aliased_shards(at2v_mod, data, monkeypatch):
    monkeypatch.setenv("AT2V_TEST_DEVICE_ALIAS", "1")
    with at2v_mod.BatchVerifier(num_gpus=8, policy="zip215", small_batch_max=OFF) as v:
        for key in ("edge", "constructed"):
            d = data[key]
            assert np.array_equal(v.verify_batch(d.pk, d.sig, d.msg, d.off), d.valid[:, ZIP]), key


def test_host_buffer_call_submit_wait_and_reasons(verifiers, data):
    for route in ("joint_throughput", "pair"):
        v = verifiers(route)
        for key in ("edge", "constructed", 65):
            d = data[key]
            ok = v.verify_batch(d.pk, d.sig, d.msg, d.off)
            assert np.array_equal(ok, d.valid[:, ZIP]), (route, key)
            assert np.array_equal(v.reject_reasons(d.pk, d.sig, ok), d.reasons[:, ZIP]), (route, key)
            p = v.submit_batch(d.pk, d.sig, d.msg, d.off)
            assert np.array_equal(v.wait_batch(p), d.valid[:, ZIP]), (route, key)


def test_cpu_fallback_after_a_device_error(at2v_mod, data, monkeypatch):
    d = data["edge"]
    monkeypatch.setenv("AT2V_TEST_FAIL_LAUNCH", "1")
    with at2v_mod.BatchVerifier(policy="zip215", cpu_fallback=True, cpu_threads=4) as v:
        assert np.array_equal(v.verify_batch(d.pk, d.sig, d.msg, d.off), d.valid[:, ZIP])  # on the CPU pool
        assert v.info()["cpu_fallbacks"] == 1
        assert np.array_equal(v.verify_batch(d.pk, d.sig, d.msg, d.off), d.valid[:, ZIP])  # on the device


def test_policy_mask_refuses_a_zip215_context(at2v_mod, verifiers, data):
    import torch
    lib = at2v_mod.load_library()
    v, d = verifiers("joint_throughput"), data[65]
    pk, sig = np.ascontiguousarray(d.pk), np.ascontiguousarray(d.sig)
    words = np.full(3, 0xFFFFFFFF, np.uint32)
    host = np.full(d.n + 16, SENT8, np.uint8)
    assert lib.at2v_policy_mask(v._h, pk.ctypes.data, sig.ctypes.data, d.n, words.ctypes.data, host.ctypes.data) == -1
    assert (host == SENT8).all()
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    dm = torch.full((256,), SENT8, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    assert lib.at2v_policy_mask_device(v._h, p, p, 1, p, dm.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert (dm.cpu().numpy() == SENT8).all()


def test_transfers_host_and_device_forms(at2v_mod, verifiers):
    """signed transfers whose sender (and R) is torsion-shifted: the messages are built on the device"""
    import torch
    snd, sig, rcp, amt, want = (np.tile(a, (22,) + (1,) * (a.ndim - 1))[:129] for a in zr.transfer_cases())
    assert (want[:, ZIP] & ~want[:, 0]).sum() > 40
    for route in ("joint_throughput", "pair"):
        v = verifiers(route)
        assert np.array_equal(v.verify_transfers(snd, sig, rcp, amt), want[:, ZIP]), route
        n, dev = len(snd), "cuda:0"
        up = lambda a: torch.from_numpy(np.array(a, copy=True).view(np.uint8).reshape(-1)).to(dev)
        d_snd, d_sig, d_rcp, d_amt = up(snd), up(sig), up(rcp), up(amt)
        ws = at2v_mod.BatchVerifier.transfers_workspace_bytes(n, at2v_mod.WIRE_BYTES)
        d_work = torch.zeros(ws, dtype=torch.uint8, device=dev)
        nwords = (n + 31) // 32
        d_ver = torch.from_numpy(np.full(nwords + 1, SENT32, np.uint32).view(np.int32)).to(dev)
        v.verify_transfers_device(d_snd.data_ptr(), d_sig.data_ptr(), d_rcp.data_ptr(), d_amt.data_ptr(), n,
                                  at2v_mod.WIRE_BYTES, d_work.data_ptr(), ws, d_ver.data_ptr(), 0,
                                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        words = d_ver.cpu().numpy().view(np.uint32)
        assert words[nwords] == SENT32 and words[nwords - 1] >> (n % 32) == 0
        assert np.array_equal(at2v_mod.unpack_verdicts(words, n), want[:, ZIP]), route
    with at2v_mod.BatchVerifier(device=0, policy="dalek") as v:
        assert np.array_equal(v.verify_transfers(snd, sig, rcp, amt), want[:, 0])


@pytest.mark.parametrize("reasons", [False, True])
def test_ingest_queue_in_ticket_order(data, reasons):
    from at2v.node import IngestQueue
    with IngestQueue(device=0, policy="zip215", max_batch=1024, eager=True, reasons=reasons) as q:
        want, first = [], None
        for key in (65, "constructed"):
            d = data[key]
            t0 = q.submit(d.pk, d.sig, d.msg, d.off)
            first = t0 if first is None else first
            want += (d.reasons[:, ZIP] if reasons else d.valid[:, ZIP].astype(int)).tolist()
        q.flush()
        tickets, got = [], []
        while len(tickets) < len(want):
            t, r = q.poll_reasons(4096, 5_000_000) if reasons else q.poll(4096, 5_000_000)
            assert len(t), "queue stalled"
            tickets += t.tolist()
            got += r.tolist()
        assert tickets == list(range(first, first + len(want)))
        assert got == want
        assert q.stats()["failed_batches"] == 0


@pytest.mark.parametrize("col", [0, 1, 2], ids=["dalek", "libsodium", "dalek-legacy"])
def test_existing_policies_on_the_same_records(at2v_mod, data, col):
    """a leak of the cofactored branch into the kernels of the other policies would show on the records built for it"""
    routes = (dict(small_batch_max=OFF), dict(),
              dict(small_batch_max=OFF, sender_cache=1024, sender_comb=True, admit_first=True),
              dict(sender_cache=1024, sender_comb=True, admit_first=True))
    for kw in routes:
        with at2v_mod.BatchVerifier(device=0, policy=zr.NAMES[zr.POLICIES[col]], **kw) as v:
            for launch in range(2 if "sender_cache" in kw else 1):
                for key in ("constructed", "edge", 65):
                    check(data[key], device_pass(v, data[key]), (kw, key, launch), col)
