"""GPU: verify_kernel's joint-table ladder (verify_half_fu_joint: one table of A and R, 2-bit windows) through the C ABI
of libat2v.so. A plain context (no sender cache) with the low-latency kernel off, device buffers, one launch per case:
that is the path that runs verify_kernel whatever the batch size. Expected verdicts are the golden sets' stored ones
(OpenSSL / libsodium). Every launch also checks that pad bits are 0 and that nothing is written past ceil(n/32) words."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
L_ORDER = 2 ** 252 + 27742317777372353535851937790883648493
N8 = 8 * L_ORDER


@pytest.fixture(scope="module")
def verifiers():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import at2v
    vs = {p: at2v.BatchVerifier(device=0, policy=p, small_batch_max=at2v.SMALL_BATCH_OFF) for p in ("dalek", "libsodium")}
    yield vs
    for v in vs.values():
        v.close()


def launch(v, g, lo, hi):
    """records [lo, hi) of set g as one device launch -> bool[hi - lo]"""
    import torch
    import at2v
    n = hi - lo
    off = (g.off[lo:hi + 1] - g.off[lo]).astype(np.uint32)
    mb = int(off[-1])
    msg = np.zeros(mb + 16, np.uint8)
    msg[:mb] = g.msg[int(g.off[lo]):int(g.off[hi])]
    dev = "cuda:0"
    d_pk = torch.from_numpy(g.pk[lo:hi].reshape(-1).copy()).to(dev)
    d_sig = torch.from_numpy(g.sig[lo:hi].reshape(-1).copy()).to(dev)
    d_msg = torch.from_numpy(msg).to(dev)
    d_off = torch.from_numpy(off.view(np.int32).copy()).to(dev)
    nwords = (n + 31) // 32
    d_ver = torch.full((nwords + 1,), SENTINEL, dtype=torch.int32, device=dev)
    v.verify_batch_device(d_pk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), mb, d_off.data_ptr(), n,
                          d_ver.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    words = d_ver.cpu().numpy().view(np.uint32)
    assert words[nwords] == SENTINEL, "a word past ceil(n/32) was written"
    if n % 32:
        assert words[nwords - 1] >> (n % 32) == 0, "pad bits must be 0"
    return at2v.unpack_verdicts(words[:nwords], n)


def expected(g, policy):
    return g.dalek if policy == "dalek" else g.sodium


@pytest.mark.parametrize("policy", ["dalek", "libsodium"])
@pytest.mark.parametrize("name", ["rfc8032", "at2_cfg1", "adversarial", "edge", "ragged"])
def test_golden_sets(verifiers, golden, name, policy):
    g = golden[name]
    assert np.array_equal(launch(verifiers[policy], g, 0, g.n), expected(g, policy))


@pytest.mark.parametrize("policy", ["dalek", "libsodium"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_sizes_around_the_wave(verifiers, golden, n, policy):
    """one lane, a wave less one, a full wave, a wave plus one lane, two waves plus one: tail lanes recompute the
    last record and are masked. From the edge set's small-order block and from the adversarial mix."""
    for name, lo in (("edge", 0), ("adversarial", 1000)):
        g = golden[name]
        assert np.array_equal(launch(verifiers[policy], g, lo, lo + n), expected(g, policy)[lo:lo + n])


def scalar_digits(pk, sig, msg):
    """digit count of the joint ladder for one record: the half-size scalars by Euclid on (8l, k) stopped below
    sqrt(8l), the shortest candidate with c1 odd, then the smallest m with max(|c0|, |c1|) <= 2 (4^m - 1) / 3"""
    k = int.from_bytes(hashlib.sha512(sig[:32] + pk + msg).digest(), "little") % L_ORDER
    r0, t0, r1, t1 = N8, 0, k, 1
    while r1 * r1 >= N8:
        q = r0 // r1
        r0, t0, r1, t1 = r1, t1, r0 - q * r1, t0 - q * t1
    q = r0 // r1 if r1 else 0
    r2, t2 = (r0 - q * r1, t0 - q * t1) if r1 else (r0, t0)
    cands = [(r1, t1), (r2, t2), (r0, t0), (r1 + r2, t1 + t2), (r1 - r2, t1 - t2)]
    size = min(max(abs(c0), abs(c1)) for c0, c1 in cands if c1 % 2)
    m = 0
    while 3 * size > 2 * (4 ** m - 1):
        m += 1
    return m


def test_failing_decode_beside_the_longest_scalar(verifiers, golden):
    """The window count of a wave is the maximum of its lanes' digit counts, and a lane that fails a check counts 0
    windows but still rides the wave's ladder on whatever its failed decode left. Launches cut so that a record whose A
    does not decode (class 7) and the record with the longest scalars of its neighbourhood share the first wave,
    with the failing record first, last and in between."""
    g = golden["adversarial"]
    bad = [int(i) for i in np.flatnonzero(g.cls == 7) if 64 <= i < g.n - 200][:3]
    assert len(bad) == 3
    for f in bad:
        near = range(f - 63, f + 64)
        digits = {j: scalar_digits(g.pk[j].tobytes(), g.sig[j].tobytes(), g.message(j)) for j in near if j != f}
        top = max(digits.values())
        assert top > min(digits.values())  # the long one does set the wave's count
        j = max(j for j in digits if digits[j] == top)
        cuts = {min(f, j), max(f, j) - 63, (min(f, j) + max(f, j) - 63) // 2}
        for lo in cuts:
            assert lo <= min(f, j) and max(f, j) < lo + 64
            for policy in ("dalek", "libsodium"):
                got = launch(verifiers[policy], g, lo, lo + 129)
                assert np.array_equal(got, expected(g, policy)[lo:lo + 129])
                assert not got[f - lo]
