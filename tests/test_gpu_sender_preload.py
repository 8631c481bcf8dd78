"""GPU: known senders — at2v_sender_preload / _unpin / _query and at2v_queue_sender_preload (include/at2v.h).

The sender cache learns keys from traffic (a key is usable after its second sighting and a build behind a launch) and
forgets them by age alone. These calls let the caller say who will send: a preloaded key is served from the cache by the
very next launch, a pinned key survives every replacement pass, and a query reports what the cache holds. Every expected
verdict comes from the oracle or the golden fixtures; the hit counters (at2v_info) show which path served the records:
`cache_record_hits` for partitioned launches (above small_batch_max), `cache_chunk_hits` for the four-wave small-batch
comb kernel. The caches are small (64 keys) and the launches a few hundred records, so each test takes seconds; where the
[j]A-table cache must serve a launch, small_batch_max is 64 (32 for a batch that two shards split) and the launch larger."""
import threading

import numpy as np
import pytest

import golden_io

pytestmark = pytest.mark.gpu

CACHED, PINNED, BAD_KEY = 1, 2, 4
E_INVALID = -1
L = 48  # message bytes per record


@pytest.fixture(params=[False, True], ids=["tables", "comb"])
def comb(request):
    return request.param


@pytest.fixture(scope="module")
def at2v_mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import at2v
    return at2v


def _keys(oracle, tag, count):
    """`count` fresh (seed, public key) pairs: seed_i = SHA-512(tag || i)[0:32]"""
    seeds = [oracle.sha512(b"at2v/preload/" + tag + i.to_bytes(4, "little"))[:32] for i in range(count)]
    pk = np.frombuffer(b"".join(oracle.public_key(s) for s in seeds), np.uint8).reshape(count, 32).copy()
    return seeds, pk


def _records(oracle, seeds, pk, n, salt=0):
    """n valid records, record i signed by sender i % len(seeds) over its own message"""
    rng = np.random.default_rng(1000 + salt)
    msg = rng.integers(0, 256, n * L, dtype=np.uint8)
    sig = np.zeros((n, 64), np.uint8)
    for i in range(n):
        sig[i] = np.frombuffer(oracle.sign(seeds[i % len(seeds)], msg[i * L:(i + 1) * L].tobytes()), np.uint8)
    rpk = pk[np.arange(n) % len(seeds)].copy()
    off = (np.arange(n + 1) * L).astype(np.uint32)
    return rpk, sig, msg, off


def _mutate(pk, sig, msg, off, rng, idx, kinds):
    """records idx mutated by one bit flip in R, S, M or (kinds = 4) A"""
    pk, sig, msg = pk.copy(), sig.copy(), msg.copy()
    for i in idx:
        kind = rng.integers(0, kinds)
        if kind == 0:
            sig[i, rng.integers(0, 32)] ^= 1 << rng.integers(0, 8)
        elif kind == 1:
            sig[i, 32 + rng.integers(0, 31)] ^= 1 << rng.integers(0, 8)
        elif kind == 2:
            msg[off[i] + rng.integers(0, off[i + 1] - off[i])] ^= 1
        else:
            pk[i, rng.integers(0, 32)] ^= 1 << rng.integers(0, 8)
    return pk, sig, msg


def _churn_launch(oracle, k):
    """128 valid records of 64 senders nobody has seen (each sender twice): one launch of cache churn"""
    pk, sig, msg, off = oracle.gen_records(0x5EED0000 + k, 64 * k, 64, L)
    return np.tile(pk, (2, 1)), np.tile(sig, (2, 1)), np.tile(msg, 2), (np.arange(129) * L).astype(np.uint32)


@pytest.fixture(scope="module")
def first_launch_case(oracle):
    """16 fresh senders, 256 records, 26 of them (about 10 %) mutated: 23 in sig or msg anywhere, 3 in pk inside the
    first 64 records (a mutated pk is another sender, one that was not preloaded). So 253 records have a preloaded
    sender, and 3 of the 4 64-record chunks hold preloaded senders only."""
    seeds, keys = _keys(oracle, b"first", 16)
    pk, sig, msg, off = _records(oracle, seeds, keys, 256)
    rng = np.random.default_rng(41)
    pk, sig, msg = _mutate(pk, sig, msg, off, rng, rng.choice(np.arange(3, 256), 23, replace=False), kinds=3)
    for i in (0, 1, 2):
        pk[i, 5 + i] ^= 0x10
    want = oracle.verify_batch(pk, sig, msg, off)
    assert 200 <= want.sum() <= 233
    known = np.array([bytes(r) in {bytes(k) for k in keys} for r in pk])
    assert known.sum() == 253 and known[64:].all()
    return keys, (pk, sig, msg, off), want


@pytest.mark.parametrize("comb,path", [(False, "partitioned"), (True, "partitioned"), (True, "small_batch_comb")],
                         ids=["tables-partitioned", "comb-partitioned", "comb-small_batch"])
def test_preloaded_keys_hit_on_the_first_launch(at2v_mod, first_launch_case, comb, path):
    """default admission (not ADMIT_FIRST): preload, then ONE launch. Its verdicts are the oracle's and the counter of
    the path that ran shows the preloaded senders served from the cache: for the partitioned launch (tables and combs,
    small_batch_max 64 < 256 records) cache_record_hits grows by the 253 records whose sender was preloaded; for the
    four-wave small-batch comb kernel cache_chunk_hits grows by the 3 chunks whose records all have one. The same
    launch on a context that was not told: 0 hits. (The small-batch kernel takes nothing from a [j]A-table cache, so
    that path exists with combs only.)"""
    keys, rec, want = first_launch_case
    counter, expect = ("cache_record_hits", 253) if path == "partitioned" else ("cache_chunk_hits", 3)
    sbm = 64 if path == "partitioned" else 0
    for preload in (True, False):
        with at2v_mod.BatchVerifier(small_batch_max=sbm, sender_cache=64, sender_comb=comb) as v:
            if preload:
                st = v.sender_preload(keys)
                assert (st == CACHED).all(), st
                assert v.info()["cache_entries"] == 16
            h0 = v.info()[counter]
            got = v.verify_batch(*rec)
            assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
            hits = v.info()[counter] - h0
            print(f"{path} comb={comb} preload={preload}: {counter} +{hits}")
            assert hits == (expect if preload else 0)


@pytest.mark.parametrize("policy", ["dalek", "libsodium"])
def test_golden_edge_senders_preloaded(at2v_mod, oracle, policy, comb):
    """every distinct sender of the edge fixture (off-curve sweep, small-order and non-canonical keys) preloaded into a
    cache of more than twice their number: BAD_KEY equals the oracle's decode, every key is cached (an undecodable key
    with decode verdict 0), and the set's first launch is served from the cache with the stored verdicts"""
    g = golden_io.load("edge")
    keys = np.unique(np.ascontiguousarray(g.pk).reshape(-1, 32), axis=0)
    bad = np.array([0 if oracle.decompress_ok(bytes(k)) else BAD_KEY for k in keys], np.uint8)
    capacity = 256
    assert 2 * len(keys) <= capacity and g.n > 64
    want = g.dalek if policy == "dalek" else g.sodium
    with at2v_mod.BatchVerifier(policy=policy, small_batch_max=64, sender_cache=capacity, sender_comb=comb) as v:
        st = v.sender_preload(keys)
        assert np.array_equal(st & BAD_KEY, bad)
        assert ((st & CACHED) == CACHED).all() and not (st & PINNED).any()
        assert np.array_equal(v.sender_query(keys), st)
        h0 = v.info()["cache_record_hits"]
        got = v.verify_batch(g.pk, g.sig, g.msg, g.off)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        assert v.info()["cache_record_hits"] - h0 == g.n


def test_pins_survive_churn(at2v_mod, oracle, comb):
    """capacity 64, ADMIT_FIRST, 8 pinned keys; launches of 64 new senders each until the cache has been compacted at
    least twice and has evicted entries. The 8 are still CACHED|PINNED, a launch of their records is all hits; after
    unpin a query reports CACHED without PINNED at once."""
    seeds, keys = _keys(oracle, b"pins", 8)
    rec = _records(oracle, seeds, keys, 256, salt=3)
    rng = np.random.default_rng(43)
    rec = (*_mutate(*rec, rng, rng.choice(256, 25, replace=False), kinds=3), rec[3])
    want = oracle.verify_batch(*rec)
    with at2v_mod.BatchVerifier(small_batch_max=64, sender_cache=64, sender_comb=comb, admit_first=True) as v:
        assert (v.sender_preload(keys, pin=True) == (CACHED | PINNED)).all()
        i0 = v.info()
        for k in range(80):
            churn = _churn_launch(oracle, k)
            assert np.array_equal(v.verify_batch(*churn), oracle.verify_batch(*churn)), k
            info = v.info()
            if info["cache_compactions"] - i0["cache_compactions"] >= 2 and info["cache_evicted"] > 0:
                break
        print(f"churn: {k + 1} launches, {info}")
        assert info["cache_compactions"] - i0["cache_compactions"] >= 2 and info["cache_evicted"] > 0, info
        assert (v.sender_query(keys) == (CACHED | PINNED)).all()
        h0 = v.info()["cache_record_hits"]
        got = v.verify_batch(*rec)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        assert v.info()["cache_record_hits"] - h0 == 256
        v.sender_unpin(keys)
        assert (v.sender_query(keys) == CACHED).all()


def test_preload_makes_room(at2v_mod, oracle, comb):
    """a 64-key cache filled from traffic (4 pinned keys, 60 senders learned by a launch): preloading 32 new keys runs one
    compaction inside the call (keep target 64 - 32), all 32 come back CACHED, their launch is all hits with exact
    verdicts, and the keys pinned before are still CACHED|PINNED"""
    pseeds, pinned = _keys(oracle, b"room/pinned", 4)
    tseeds, traffic = _keys(oracle, b"room/traffic", 60)
    nseeds, fresh = _keys(oracle, b"room/new", 32)
    fill = _records(oracle, tseeds, traffic, 240, salt=5)
    rec = _records(oracle, nseeds, fresh, 256, salt=6)
    rng = np.random.default_rng(47)
    rec = (*_mutate(*rec, rng, rng.choice(256, 25, replace=False), kinds=3), rec[3])
    want = oracle.verify_batch(*rec)
    with at2v_mod.BatchVerifier(small_batch_max=64, sender_cache=64, sender_comb=comb, admit_first=True) as v:
        assert (v.sender_preload(pinned, pin=True) == (CACHED | PINNED)).all()
        assert v.verify_batch(*fill).all()
        i0 = v.info()
        assert i0["cache_entries"] == 64, i0
        st = v.sender_preload(fresh)
        assert (st == CACHED).all(), st
        i1 = v.info()
        assert i1["cache_compactions"] == i0["cache_compactions"] + 1, (i0, i1)
        assert i1["cache_entries"] == 64 and i1["cache_evicted"] - i0["cache_evicted"] == 32, i1
        got = v.verify_batch(*rec)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        assert v.info()["cache_record_hits"] - i1["cache_record_hits"] == 256
        assert (v.sender_query(pinned) == (CACHED | PINNED)).all()
        assert (v.sender_query(fresh) == CACHED).all()


def test_limits_change_nothing(at2v_mod, oracle):
    """capacity 64: 33 distinct keys in one call, and a 33rd pinned key, are AT2V_E_INVALID and cache and pin nothing;
    duplicates in one list count once"""
    _, keys = _keys(oracle, b"limits", 66)
    with at2v_mod.BatchVerifier(small_batch_max=64, sender_cache=64) as v:
        with pytest.raises(at2v_mod.At2vError) as e:
            v.sender_preload(keys[:33])
        assert e.value.code == E_INVALID
        assert not v.sender_query(keys[:33]).any() and v.info()["cache_entries"] == 0
        # 64 listed keys, 32 distinct: within the limit
        twice = np.concatenate([keys[:32], keys[:32]])
        assert (v.sender_preload(twice) == CACHED).all()
        assert v.info()["cache_entries"] == 32
        # pinning those 32 (listed twice) reaches the pin limit exactly; pinning them again adds nothing
        assert (v.sender_preload(twice, pin=True) == (CACHED | PINNED)).all()
        assert (v.sender_preload(keys[:5], pin=True) == (CACHED | PINNED)).all()
        before = v.info()
        with pytest.raises(at2v_mod.At2vError) as e:
            v.sender_preload(keys[40:41], pin=True)
        assert e.value.code == E_INVALID
        with pytest.raises(at2v_mod.At2vError) as e:
            v.sender_preload(np.concatenate([keys[:3], keys[40:41]]), pin=True)  # 3 pinned already + 1 new: 33
        assert e.value.code == E_INVALID
        assert not v.sender_query(keys[40:41]).any()
        assert (v.sender_query(keys[:32]) == (CACHED | PINNED)).all()
        after = v.info()
        assert after["cache_entries"] == before["cache_entries"] == 32 and after["cache_claims"] == before["cache_claims"]
        # an unpinned key is still welcome, and unpinning makes room in the pin set again
        assert (v.sender_preload(keys[40:41]) == CACHED).all()
        v.sender_unpin(keys[:1])
        assert (v.sender_preload(keys[40:41], pin=True) == (CACHED | PINNED)).all()
        assert v.sender_query(keys[:1])[0] == CACHED


def test_forced_fingerprint_collisions(at2v_mod, oracle, monkeypatch, comb):
    """4 fingerprint bits (test hook): 32 keys share at most 16 fingerprints. A key whose fingerprint another key holds
    is simply not cached: the call returns AT2V_OK, at most 16 report CACHED, none is counted as pinned without being
    cached, and a launch over all 32 senders' records gives the oracle's verdicts"""
    monkeypatch.setenv("AT2V_TEST_CACHE_FP_BITS", "4")
    seeds, keys = _keys(oracle, b"collide", 32)
    rec = _records(oracle, seeds, keys, 256, salt=7)
    rng = np.random.default_rng(53)
    rec = (*_mutate(*rec, rng, rng.choice(256, 25, replace=False), kinds=4), rec[3])
    want = oracle.verify_batch(*rec)
    with at2v_mod.BatchVerifier(small_batch_max=64, sender_cache=64, sender_comb=comb) as v:
        st = v.sender_preload(keys, pin=True)
        cached = (st & CACHED) != 0
        assert 1 <= cached.sum() <= 16, st
        assert np.array_equal((st & PINNED) != 0, cached) and not (st & BAD_KEY).any()
        assert np.array_equal(v.sender_query(keys), st)
        assert v.info()["cache_entries"] == cached.sum()
        for rep in range(2):
            got = v.verify_batch(*rec)
            assert np.array_equal(got, want), (rep, np.nonzero(got != want)[0][:10])
        # the keys that could not be cached left the pin set: pinning up to the limit is still possible
        _, more = _keys(oracle, b"collide/more", 16)
        st2 = v.sender_preload(more, pin=True)
        assert np.array_equal((st2 & PINNED) != 0, (st2 & CACHED) != 0)


def test_query_has_no_side_effects(at2v_mod, oracle, comb):
    _, known = _keys(oracle, b"query/known", 8)
    _, unknown = _keys(oracle, b"query/unknown", 40)
    with at2v_mod.BatchVerifier(small_batch_max=64, sender_cache=64, sender_comb=comb) as v:
        v.sender_preload(known)
        before = v.info()
        for _ in range(3):
            assert not v.sender_query(unknown).any()
        assert (v.sender_query(np.concatenate([unknown[:3], known])) == [0, 0, 0] + [CACHED] * 8).all()
        after = v.info()
        for f in ("cache_claims", "cache_sightings", "cache_entries", "cache_compactions", "cache_built"):
            assert after[f] == before[f], (f, before, after)
        # ... and asked-for keys were not made cacheable by asking: a later preload still has to claim them
        assert (v.sender_preload(unknown[:8]) == CACHED).all()
        assert v.info()["cache_claims"] == before["cache_claims"] + 8


def test_two_shards_on_one_gpu(at2v_mod, oracle, monkeypatch, comb):
    """num_gpus = 2 aliased onto one device: the preload builds the keys on both shards' caches, and a 129-record
    host-buffer batch (64 records on one shard, 65 on the other, small_batch_max 32) is all hits on both"""
    monkeypatch.setenv("AT2V_TEST_DEVICE_ALIAS", "1")
    seeds, keys = _keys(oracle, b"shards", 16)
    rec = _records(oracle, seeds, keys, 129, salt=9)
    rng = np.random.default_rng(59)
    rec = (*_mutate(*rec, rng, rng.choice(129, 13, replace=False), kinds=3), rec[3])
    want = oracle.verify_batch(*rec)
    with at2v_mod.BatchVerifier(num_gpus=2, small_batch_max=32, sender_cache=64, sender_comb=comb) as v:
        assert v.info()["num_gpus"] == 2 and v.info()["cache_capacity"] == 128
        assert (v.sender_preload(keys, pin=True) == (CACHED | PINNED)).all()
        i0 = v.info()
        assert i0["cache_entries"] == 32  # 16 keys on each shard
        got = v.verify_batch(*rec)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        assert v.info()["cache_record_hits"] - i0["cache_record_hits"] == 129
        v.sender_unpin(keys)
        assert (v.sender_query(keys) == CACHED).all()


def test_preload_between_overlapping_launches(at2v_mod, oracle, comb):
    """a 4,096-record device launch on each of two streams, a preload at once (no synchronisation in between), then a
    third launch of the preloaded senders' records: all three verdict sets are the oracle's, and the third launch hits"""
    import torch
    seeds, keys = _keys(oracle, b"overlap", 16)
    sets = [oracle.gen_records(0x0A0A0000 + j, 4096 * j, 4096, L) for j in range(2)]
    sets.append(_records(oracle, seeds, keys, 4096, salt=11))
    rng = np.random.default_rng(61)
    sets = [(*_mutate(*s, rng, rng.choice(4096, 400, replace=False), kinds=3), s[3]) for s in sets]
    wants = [oracle.verify_batch(*s) for s in sets]
    dev = []
    for pk, sig, msg, off in sets:
        dev.append((torch.from_numpy(pk.reshape(-1)).cuda(), torch.from_numpy(sig.reshape(-1)).cuda(),
                    torch.from_numpy(np.concatenate([msg, np.zeros(16, np.uint8)])).cuda(),
                    torch.from_numpy(off.view(np.int32)).cuda(), torch.zeros(128, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()
    streams = at2v_mod.launch_streams(2)
    with at2v_mod.BatchVerifier(small_batch_max=64, sender_cache=64, sender_comb=comb) as v:

        def launch(j, stream):
            d_pk, d_sig, d_msg, d_off, d_ver = dev[j]
            v.verify_batch_device(d_pk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), 4096 * L, d_off.data_ptr(), 4096,
                                  d_ver.data_ptr(), stream.cuda_stream)

        h0 = v.info()["cache_record_hits"]
        launch(0, streams[0])
        launch(1, streams[1])
        st = v.sender_preload(keys)  # ordered behind both launches by the library itself
        launch(2, streams[0])
        torch.cuda.synchronize()
        assert (st == CACHED).all(), st
        for j in range(3):
            got = at2v_mod.unpack_verdicts(dev[j][4].cpu().numpy().view(np.uint32), 4096)
            assert np.array_equal(got, wants[j]), (j, np.nonzero(got != wants[j])[0][:10])
        assert v.info()["cache_record_hits"] - h0 == 4096  # the third launch's records, none of the first two's


def test_queue_preload_from_a_second_thread(at2v_mod, oracle):
    """an eager comb queue: a producer submits 16 senders' records in small pieces while a second thread preloads those
    senders; every polled verdict is the oracle's and the statuses are CACHED"""
    from at2v.node import IngestQueue
    seeds, keys = _keys(oracle, b"queue", 16)
    n = 2048
    rec = _records(oracle, seeds, keys, n, salt=13)
    rng = np.random.default_rng(67)
    pk, sig, msg = _mutate(*rec, rng, rng.choice(n, 200, replace=False), kinds=3)
    off = rec[3]
    want = oracle.verify_batch(pk, sig, msg, off)
    status, errors = [], []
    with IngestQueue(eager=True, sender_comb=True, sender_cache=64, max_batch=1024) as q:

        def producer():
            try:
                for a in range(0, n, 32):
                    q.submit(pk[a:a + 32], sig[a:a + 32], msg[off[a]:off[a + 32]], off[a:a + 33] - off[a])
            except Exception as e:  # noqa: BLE001 (reported by the main thread)
                errors.append(e)

        def preloader():
            try:
                status.append(q.preload_senders(keys))
                status.append(q.preload_senders(keys, pin=True))
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        th = [threading.Thread(target=producer), threading.Thread(target=preloader)]
        for t in th:
            t.start()
        got = np.full(n, 0xEE, np.uint8)
        seen = 0
        for _ in range(4000):
            tickets, verdicts = q.poll(4096, 5000)
            got[np.asarray(tickets, np.int64)] = verdicts
            seen += len(tickets)
            if seen == n:
                break
        for t in th:
            t.join()
        assert not errors, errors
        assert seen == n
        assert np.array_equal(got, want.astype(np.uint8)), np.nonzero(got != want)[0][:10]
        assert (status[0] == CACHED).all() and (status[1] == (CACHED | PINNED)).all(), status
