"""CPU: the pinned host memory calls of ABI 9 (include/at2v.h at2v_host_alloc / _free / _register / _unregister) on a
CPU context (num_gpus = 0), where they only allocate and record ranges and touch no device: a caller's code is the same
on both backends. The GPU side (uploads straight from such memory) is tests/test_gpu_pinned.py; the registry itself is
tests/test_hostmem_host.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_io
import pinned_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1


@pytest.fixture(scope="module")
def at2v_mod():
    import at2v
    at2v.load_library()
    return at2v


@pytest.fixture()
def cpu_ctx(at2v_mod):
    with at2v_mod.BatchVerifier(num_gpus=0, cpu_threads=3) as v:
        yield v


def test_abi_version_and_symbols(at2v_mod):
    lib = at2v_mod.load_library()
    assert at2v_mod.ABI_VERSION == 9 and lib.at2v_abi_version() == 9
    for name in ("at2v_host_alloc", "at2v_host_free", "at2v_host_register", "at2v_host_unregister"):
        assert name in at2v_mod.EXPORTED_SYMBOLS and hasattr(lib, name)


@pytest.mark.parametrize("policy", ["dalek", "libsodium"])
def test_golden_sets_from_one_allocation(at2v_mod, golden, policy):
    """pk, sig, offsets, messages (odd address, msg_off[0] > 0) and the verdict words carved out of one host_alloc
    block: the stored verdicts, pad bits 0, the word after the bitmap untouched"""
    with at2v_mod.BatchVerifier(num_gpus=0, cpu_threads=3, policy=policy) as v:
        for name in golden_io.SETS:
            g = golden[name]
            block = v.host_alloc(pinned_layout.carved_bytes(g.n, len(g.msg)))
            assert block.dtype == np.uint8 and block.ctypes.data % 64 == 0
            c = pinned_layout.carve(block, g.pk, g.sig, g.msg, g.off)
            got = v.verify_batch(c.pk, c.sig, c.msg, c.off, words=c.verdict_words())
            want = g.dalek if policy == "dalek" else g.sodium
            assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:10])
            assert np.array_equal(at2v_mod.unpack_verdicts(c.verdict_words(), g.n), want)
            pinned_layout.check_words(c)
            v.host_free(block)
        inf = v.info()
    assert inf["num_gpus"] == 0 and inf["host_direct_bytes"] == 0 and inf["host_staged_bytes"] == 0
    assert inf["cpu_batches"] == len(golden_io.SETS)


def test_register_and_unregister_a_numpy_array(at2v_mod, cpu_ctx, golden):
    g = golden["ragged"]
    pk, sig, msg = g.pk.copy(), g.sig.copy(), g.msg.copy()
    for a in (pk, sig, msg):
        cpu_ctx.host_register(a)
    assert np.array_equal(cpu_ctx.verify_batch(pk, sig, msg, g.off), g.dalek)
    for a in (pk, sig, msg):
        cpu_ctx.host_unregister(a)
    assert np.array_equal(cpu_ctx.verify_batch(pk, sig, msg, g.off), g.dalek)
    cpu_ctx.host_register(msg)  # known again after an unregister; at2v_destroy drops what is still registered
    inf = cpu_ctx.info()
    assert inf["host_direct_bytes"] == 0 and inf["host_staged_bytes"] == 0


def test_error_cases(at2v_mod, cpu_ctx):
    lib = at2v_mod.load_library()
    h = cpu_ctx._h
    out = ctypes.c_void_p()
    # zero bytes, null out / p / ctx
    assert lib.at2v_host_alloc(h, 0, ctypes.byref(out)) == E_INVALID and not out.value
    assert lib.at2v_host_alloc(h, 64, None) == E_INVALID
    assert lib.at2v_host_alloc(None, 64, ctypes.byref(out)) == E_INVALID
    assert lib.at2v_host_free(h, None) == E_INVALID and lib.at2v_host_unregister(h, None) == E_INVALID
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    assert lib.at2v_host_register(h, p, 0) == E_INVALID
    assert lib.at2v_host_register(h, None, 16) == E_INVALID
    # unknown pointers
    assert lib.at2v_host_free(h, p) == E_INVALID and lib.at2v_host_unregister(h, p) == E_INVALID
    # a registered range: overlaps refused (inside, across either end, covering, the same again), neighbours accepted
    assert lib.at2v_host_register(h, p + 1000, 1000) == 0
    for q, n in ((p + 1000, 1000), (p + 1500, 10), (p + 999, 2), (p + 1999, 2), (p + 500, 2000)):
        assert lib.at2v_host_register(h, q, n) == E_INVALID, (q - p, n)
    assert lib.at2v_host_register(h, p + 2000, 96) == 0 and lib.at2v_host_register(h, p + 900, 100) == 0
    # an interior pointer is not the start of a range; a registered range is not freed, an allocated one not unregistered
    assert lib.at2v_host_unregister(h, p + 1001) == E_INVALID
    assert lib.at2v_host_free(h, p + 1000) == E_INVALID
    assert lib.at2v_host_unregister(h, p + 1000) == 0
    assert lib.at2v_host_unregister(h, p + 1000) == E_INVALID  # twice
    assert lib.at2v_host_register(h, p + 1000, 1000) == 0       # free again once unregistered
    # an allocation: 64-byte aligned, overlap with it refused, interior pointer refused, double free refused
    assert lib.at2v_host_alloc(h, 100, ctypes.byref(out)) == 0 and out.value and out.value % 64 == 0
    a = out.value
    assert lib.at2v_host_register(h, a + 10, 10) == E_INVALID
    assert lib.at2v_host_unregister(h, a) == E_INVALID
    assert lib.at2v_host_free(h, a + 1) == E_INVALID
    assert lib.at2v_host_free(h, a) == 0
    assert lib.at2v_host_free(h, a) == E_INVALID
    with pytest.raises(at2v_mod.At2vError):
        cpu_ctx.host_alloc(0)
    with pytest.raises(ValueError):
        cpu_ctx.host_register(np.zeros((4, 4), np.uint8)[:, 1])  # not contiguous


def test_allocation_keeps_the_verifier_alive(at2v_mod):
    v = at2v_mod.BatchVerifier(num_gpus=0, cpu_threads=1)
    a = v.host_alloc(1000)
    view = a[10:20]
    del v, a
    import gc
    gc.collect()
    view[:] = 7  # the context (which owns the memory) is still there
    assert int(view.sum()) == 70


def test_destroy_releases_what_is_left(at2v_mod):
    """a context destroyed with allocations and registrations outstanding frees / forgets them (no error, no crash)"""
    buf = np.zeros(256, np.uint8)
    v = at2v_mod.BatchVerifier(num_gpus=0, cpu_threads=1)
    v.host_alloc(4096)
    v.host_alloc(1)
    v.host_register(buf)
    v.close()
    with at2v_mod.BatchVerifier(num_gpus=0, cpu_threads=1) as w:  # the array can be registered with another context
        w.host_register(buf)
        w.host_unregister(buf)


CHILD = r"""
import os, sys
sys.path[:0] = [%r, %r]
os.environ["AT2V_TEST_HOOKS"] = "1"
import numpy as np
import at2v, golden_io, pinned_layout

def gpu_fds():
    out = []
    for f in os.listdir("/proc/self/fd"):
        try:
            t = os.readlink("/proc/self/fd/" + f)
        except OSError:
            continue
        if t.startswith("/dev/kfd") or t.startswith("/dev/dri/"):
            out.append(t)
    return out

g = golden_io.load("edge")
with at2v.BatchVerifier(num_gpus=0, cpu_threads=2) as v:
    block = v.host_alloc(pinned_layout.carved_bytes(g.n, len(g.msg)))
    c = pinned_layout.carve(block, g.pk, g.sig, g.msg, g.off)
    assert np.array_equal(v.verify_batch(c.pk, c.sig, c.msg, c.off, words=c.verdict_words()), g.dalek)
    extra = np.zeros(999, np.uint8)
    v.host_register(extra)
    assert np.array_equal(v.verify_batch(g.pk, g.sig, g.msg, g.off), g.dalek)
    v.host_unregister(extra)
    v.host_free(block)
    inf = v.info()
    assert inf["num_gpus"] == 0 and inf["host_direct_bytes"] == 0 and inf["host_staged_bytes"] == 0
print("GPU_FDS", gpu_fds())
"""


def test_cpu_context_opens_no_device():
    """the four calls and verify calls on a CPU context in a fresh process: the process never opens the GPU driver's
    device nodes (the HIP runtime opens /dev/kfd when it initialises), with or without a GPU in the machine"""
    code = CHILD % (os.path.join(ROOT, "at2-node_amd"), os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "GPU_FDS []" in out.stdout, out.stdout[-2000:]
