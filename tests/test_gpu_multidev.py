"""GPU: the multi-device paths that a one-GPU box can still execute (VERDICT r4 "Next round" 1).

* Single process, several devices (`at2v_opts.num_gpus` > 1, at2v_api_hostcall.h at2v_verify_batch): the test hook
  AT2V_TEST_DEVICE_ALIAS=1 maps shard g to device g % ndev, so `num_gpus = 8` runs the real split on device 0: eight
  64-aligned index shards, eight shard streams, eight scratch-set pairs and B tables, eight sender caches, and every
  shard's verdict words copied into its place of the host bitmap. What changes with 8 real devices is only where those
  resources live.
* One process per GPU at config 3's per-rank load: 16M records over 8 ranks is 2,097,152 records per rank. At world 1
  the RCCL all-gather of libat2v runs with that slice size (device form) and with the host form's gather window
  (kGatherWindow = 65,536 words per round, so 2M + 100 records take two rounds).

The consumer of the bitmap is the delivery filter at /root/reference/src/bin/server/rpc.rs:156-173."""
import numpy as np
import pytest

import golden_io

pytestmark = pytest.mark.gpu

CFG_SEED = 0x4154325F
OFF = 0xFFFFFFFF


@pytest.fixture(scope="module")
def at2v_mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import at2v
    return at2v


@pytest.fixture
def alias(monkeypatch):
    monkeypatch.setenv("AT2V_TEST_DEVICE_ALIAS", "1")


KERNELS = {"lowlat": 0, "throughput": OFF}


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("policy", ["dalek", "libsodium"])
def test_eight_shards_golden_sets(at2v_mod, golden, alias, policy, kernel):
    """every golden set through an 8-shard context (both policies, both kernels): the shards' words land in record
    order, pad bits stay 0"""
    with at2v_mod.BatchVerifier(num_gpus=8, policy=policy, small_batch_max=KERNELS[kernel]) as v:
        assert v.info()["num_gpus"] == 8
        for name in golden_io.SETS:
            g = golden[name]
            want = g.dalek if policy == "dalek" else g.sodium
            got = v.verify_batch(g.pk, g.sig, g.msg, g.off)
            assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:10])


@pytest.mark.parametrize("n", [1, 63, 64 * 8 + 1, 100_003])
def test_eight_shards_sizes(at2v_mod, oracle, alias, n):
    """n records over 8 shards: fewer records than shards (most shards empty), one ragged chunk on one shard, a
    ragged last shard; adversarial records against the oracle, with a sentinel word after the bitmap"""
    pk, sig, msg, off, cls = oracle.gen_adversarial(CFG_SEED + 61, 0, n, 80)
    want = oracle.verify_batch(pk, sig, msg, off)
    lib = at2v_mod.load_library()
    for small in (0, OFF):
        with at2v_mod.BatchVerifier(num_gpus=8, small_batch_max=small) as v:
            words = np.full((n + 31) // 32 + 1, 0xA5A5A5A5, np.uint32)
            rc = lib.at2v_verify_batch(v._h, pk.ctypes.data, sig.ctypes.data, msg.ctypes.data, off.ctypes.data, n,
                                       words.ctypes.data)
            assert rc == 0
            assert words[-1] == 0xA5A5A5A5
            got = at2v_mod.unpack_verdicts(words[:-1], n)
            assert np.array_equal(got, want), (small, np.nonzero(got != want)[0][:10])
            if n % 32:
                assert int(words[(n - 1) // 32]) >> (n % 32) == 0


def test_eight_shards_sender_combs(at2v_mod, oracle, alias):
    """an 8-shard context with per-sender combs: each shard has its own cache (its own tags, payloads, build stream);
    config-1 traffic tiled 8x (every shard sees all 64 senders), mutated, cold then warm: verdicts equal the oracle's,
    and the warm launches take the comb path on every shard"""
    pk, sig, msg, off, snd, seq = oracle.gen_at2_transactions()
    L = 48
    pk = np.tile(pk, (8, 1))
    sig = np.tile(sig, (8, 1)).copy()
    msg = np.tile(msg, 8)
    n = len(pk)
    off = (np.arange(n + 1) * L).astype(np.uint32)
    rng = np.random.default_rng(67)
    bad = rng.choice(n, 800, replace=False)
    sig[bad, 40] ^= 0x04  # S changes: rejected
    want = oracle.verify_batch(pk, sig, msg, off)
    assert want.sum() == n - 800
    with at2v_mod.BatchVerifier(num_gpus=8, sender_cache=256, sender_comb=True, small_batch_max=OFF) as v:
        for rep in range(4):
            got = v.verify_batch(pk, sig, msg, off)
            assert np.array_equal(got, want), (rep, np.nonzero(got != want)[0][:10])
            info = v.info()  # (waits for every shard's build stream)
        assert info["cache_capacity"] == 8 * 256
        assert info["cache_claims"] == 8 * 64, info  # every shard claimed the 64 senders once
        assert info["cache_chunk_hits"] > 0, info


def test_world1_gather_device_at_config3_rank_load(at2v_mod):
    """config 3's per-rank slice (2,097,152 records, minus 5 for pad bits) through at2v_verify_shard_gather_device at
    world 1: all generated records verify; after mutating 2,000 random records exactly those are rejected, and the pad
    bits of the slice's last word are 0 (property checks: the oracle would need minutes at this size)"""
    import torch
    n_slice, L = 1 << 21, 100
    n = n_slice - 5
    wpr = n_slice // 32
    with at2v_mod.BatchVerifier(small_batch_max=OFF) as v:
        v.comm_init_rank(at2v_mod.comm_unique_id(), 0, 1)
        s = torch.cuda.current_stream().cuda_stream
        d_pk = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        d_sig = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
        d_msg = torch.zeros(n * L, dtype=torch.uint8, device="cuda")
        d_off = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        d_bitmap = torch.full((wpr,), -1, dtype=torch.int32, device="cuda")
        v.gen_records_device(CFG_SEED + 71, 0, n, L, d_pk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(),
                             d_off.data_ptr(), s)
        g0 = v.info()["gathers"]
        v.verify_shard_gather_device(d_pk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), n * L, d_off.data_ptr(), n,
                                     wpr, d_bitmap.data_ptr(), s)
        torch.cuda.synchronize()
        w = d_bitmap.cpu().numpy().view(np.uint32)
        ok = at2v_mod.unpack_verdicts(w, n)
        assert ok.all(), (~ok).sum()
        assert int(w[-1]) >> (n % 32) == 0
        rng = np.random.default_rng(73)
        idx = np.unique(rng.integers(0, n, 2000))
        rows = torch.from_numpy(idx).cuda()
        cols = torch.from_numpy(rng.integers(32, 63, idx.size)).cuda()  # S bytes below the top one: s changes
        view = d_sig.view(-1, 64)
        view[rows, cols] = view[rows, cols] ^ 0x01
        v.verify_shard_gather_device(d_pk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), n * L, d_off.data_ptr(), n,
                                     wpr, d_bitmap.data_ptr(), s)
        torch.cuda.synchronize()
        ok = at2v_mod.unpack_verdicts(d_bitmap.cpu().numpy().view(np.uint32), n)
        assert np.array_equal(np.nonzero(~ok)[0], idx)
        assert v.info()["gathers"] == g0 + 2


def test_world1_sharded_host_batch_two_gather_rounds(at2v_mod):
    """at2v_verify_batch_sharded with 2,097,252 host records (two all-gather rounds of the 65,536-word window): every
    verdict lands in record order on the rank, mutated records rejected, pad bits 0"""
    import torch
    n, L = (1 << 21) + 100, 64
    with at2v_mod.BatchVerifier(small_batch_max=OFF) as v:
        s = torch.cuda.current_stream().cuda_stream
        d_pk = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        d_sig = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
        d_msg = torch.zeros(n * L, dtype=torch.uint8, device="cuda")
        d_off = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        v.gen_records_device(CFG_SEED + 79, 0, n, L, d_pk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(),
                             d_off.data_ptr(), s)
        torch.cuda.synchronize()
        pk = d_pk.cpu().numpy().reshape(n, 32)
        sig = d_sig.cpu().numpy().reshape(n, 64).copy()
        msg = d_msg.cpu().numpy()
        off = d_off.cpu().numpy().view(np.uint32)
        del d_pk, d_sig, d_msg, d_off
        rng = np.random.default_rng(83)
        idx = np.unique(np.concatenate([rng.integers(0, n, 1000), [0, (1 << 21) - 1, 1 << 21, n - 1]]))
        sig[idx, 33] ^= 0x80
        v.comm_init_rank(at2v_mod.comm_unique_id(), 0, 1)
        g0 = v.info()["gathers"]
        got = v.verify_batch_sharded(pk, sig, msg, off)
        assert v.info()["gathers"] == g0 + 2  # two window rounds
        assert np.array_equal(np.nonzero(~got)[0], idx)


def test_config3_whole_batch_eight_shards_host_buffers(at2v_mod, alias):
    """BASELINE config 3's whole node batch, 16,777,216 records (100-byte M), from HOST buffers through an 8-shard
    context (at2v_verify_batch, VERDICT r5 "Next" 1): each shard's 2,097,152 records go through its own chunked staging
    pipeline, the shards' chunks interleave round robin, and every shard's words land at word shard*65,536. Every
    generated record verifies; after flipping an S bit of exactly 3,000 distinct records, exactly those are rejected;
    the sentinel word after the bitmap stays untouched (n is a multiple of 32: no pad bits)"""
    import torch
    n, L = 1 << 24, 100
    with at2v_mod.BatchVerifier(num_gpus=1) as g:
        s = torch.cuda.current_stream().cuda_stream
        d_pk = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        d_sig = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
        d_msg = torch.zeros(n * L, dtype=torch.uint8, device="cuda")
        d_off = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        g.gen_records_device(CFG_SEED + 97, 0, n, L, d_pk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(),
                             d_off.data_ptr(), s)
        torch.cuda.synchronize()
        pk = d_pk.cpu().numpy()
        sig = d_sig.cpu().numpy().reshape(n, 64).copy()
        msg = d_msg.cpu().numpy()
        off = d_off.cpu().numpy().view(np.uint32)
        del d_pk, d_sig, d_msg, d_off
        torch.cuda.empty_cache()
    lib = at2v_mod.load_library()
    rng = np.random.default_rng(20261018)
    idx = np.sort(rng.choice(n, 3000, replace=False))
    with at2v_mod.BatchVerifier(num_gpus=8, small_batch_max=OFF) as v:
        assert v.info()["num_gpus"] == 8
        for mutate in (False, True):
            if mutate:
                sig[idx, 32 + rng.integers(0, 31, idx.size)] ^= 0x02  # an S byte below the top one: s changes
            words = np.full(n // 32 + 1, 0xA5A5A5A5, np.uint32)
            rc = lib.at2v_verify_batch(v._h, pk.ctypes.data, sig.ctypes.data, msg.ctypes.data, off.ctypes.data, n,
                                       words.ctypes.data)
            assert rc == 0
            assert words[-1] == 0xA5A5A5A5
            ok = at2v_mod.unpack_verdicts(words[:-1], n)
            if not mutate:
                assert ok.all(), f"{(~ok).sum()} generated records rejected"
            else:
                assert np.array_equal(np.nonzero(~ok)[0], idx)
