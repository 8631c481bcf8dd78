"""Helper of the pinned-memory tests (test_host_pinned_cpu.py, test_gpu_pinned.py): a whole batch carved out of ONE
block of bytes (BatchVerifier.host_alloc memory, or any uint8 array), the way a node lays received payloads out."""
from dataclasses import dataclass

import numpy as np

SENTINEL = 0xDEADBEEF


@dataclass
class Carved:
    pk: np.ndarray     # (n, 32) u8 view
    sig: np.ndarray    # (n, 64) u8 view
    msg: np.ndarray    # u8 view starting at an ODD address; the messages start `lead` bytes in
    off: np.ndarray    # (n + 1,) u32 view, off[0] == lead > 0
    words: np.ndarray  # ceil(n/32) + 1 u32 view: the verdict words and a sentinel word after them
    n: int

    @property
    def msg_bytes(self):
        return int(self.off[self.n]) - int(self.off[0])

    def verdict_words(self):
        return self.words[:-1]


def carved_bytes(n: int, msg_bytes: int, lead: int = 3) -> int:
    return 100 * n + 4 * (n + 1) + msg_bytes + lead + 4 * ((n + 31) // 32 + 2) + 512


def carve(block: np.ndarray, pk, sig, msg, off, lead: int = 3) -> Carved:
    """copy the batch into `block` (uint8, at least carved_bytes long): pk | sig | offsets | messages | verdict words.
    The messages lie at an odd address and msg_off[0] = lead > 0; the verdict words are followed by a sentinel word."""
    assert block.dtype == np.uint8 and block.ndim == 1 and lead > 0
    n = len(off) - 1
    mb = int(off[n]) - int(off[0])
    base = block.ctypes.data
    at = 0

    def take(nbytes, align, odd=False):
        nonlocal at
        at += (-(base + at)) % align
        if odd and (base + at) % 2 == 0:
            at += 1
        v = block[at:at + nbytes]
        assert len(v) == nbytes, "block too small"
        at += nbytes
        return v

    c_pk = take(32 * n, 1).reshape(n, 32)
    c_sig = take(64 * n, 64).reshape(n, 64)
    c_off = take(4 * (n + 1), 4).view(np.uint32)
    c_msg = take(lead + mb, 1, odd=True)
    c_words = take(4 * ((n + 31) // 32 + 1), 4).view(np.uint32)
    c_pk[:] = np.asarray(pk, np.uint8).reshape(n, 32)
    c_sig[:] = np.asarray(sig, np.uint8).reshape(n, 64)
    c_msg[:lead] = 0xA5
    c_msg[lead:] = np.asarray(msg, np.uint8).reshape(-1)[int(off[0]):int(off[n])]
    c_off[:] = np.asarray(off, np.uint64) - int(off[0]) + lead
    c_words[:] = SENTINEL
    assert c_msg.ctypes.data % 2 == 1 and c_off[0] == lead
    return Carved(c_pk, c_sig, c_msg, c_off, c_words, n)


def check_words(c: Carved):
    """pad bits 0 and the sentinel after the bitmap untouched"""
    assert c.words[-1] == SENTINEL, "the word after the verdict bitmap was written"
    if c.n % 32:
        assert int(c.words[(c.n - 1) // 32]) >> (c.n % 32) == 0, "pad bits set"
