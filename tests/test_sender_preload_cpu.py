"""CPU: the known-senders calls (at2v_sender_preload / _unpin / _query, at2v_queue_sender_preload; include/at2v.h) on
the CPU backend. A context with num_gpus = 0 and a queue with AT2V_QUEUE_CPU have no sender cache: the calls succeed,
cache nothing and report, per key, only whether its 32 bytes decode (AT2V_SENDER_BAD_KEY), so a caller's code is the
same on both backends. The decode verdict is compared with the oracle's point decode over every distinct public key of
the edge fixture (off-curve sweep, small-order keys, non-canonical keys)."""
import ctypes
import os
import re

import numpy as np
import pytest

import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NEW_SYMBOLS = ("at2v_sender_preload", "at2v_sender_unpin", "at2v_sender_query", "at2v_queue_sender_preload")


@pytest.fixture(scope="module")
def at2v_mod():
    import at2v
    at2v.load_library()
    return at2v


@pytest.fixture(scope="module")
def edge_keys(oracle):
    """every distinct pk of the edge fixture and the status the calls must report for it"""
    g = golden_io.load("edge")
    pk = np.unique(np.ascontiguousarray(g.pk).reshape(-1, 32), axis=0)
    want = np.array([0 if oracle.decompress_ok(bytes(k)) else 4 for k in pk], np.uint8)
    assert 0 < int((want == 4).sum()) < len(pk)  # both kinds present
    return pk, want


def test_preload_query_unpin_report_only_bad_key(at2v_mod, edge_keys):
    pk, want = edge_keys
    assert at2v_mod.SENDER_BAD_KEY == 4
    with at2v_mod.BatchVerifier(num_gpus=0, cpu_threads=2) as v:
        for pin in (False, True):
            got = v.sender_preload(pk, pin=pin)
            assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        assert np.array_equal(v.sender_query(pk), want)
        v.sender_unpin(pk)  # AT2V_OK (raises otherwise)
        assert np.array_equal(v.sender_query(pk), want)
        # duplicates and order are the caller's: one status byte per listed key
        idx = np.array([3, 3, 0, len(pk) - 1, 3])
        assert np.array_equal(v.sender_preload(pk[idx]), want[idx])
        assert v.info()["cache_capacity"] == 0 and v.info()["cache_entries"] == 0


def test_empty_list_null_and_flags(at2v_mod, edge_keys):
    pk, _ = edge_keys
    lib = at2v_mod.load_library()
    with at2v_mod.BatchVerifier(num_gpus=0, cpu_threads=1) as v:
        assert len(v.sender_preload(np.zeros((0, 32), np.uint8))) == 0
        assert len(v.sender_query(np.zeros((0, 32), np.uint8))) == 0
        v.sender_unpin(np.zeros((0, 32), np.uint8))
        h, p = v._h, pk.ctypes.data
        st = np.zeros(len(pk), np.uint8)
        assert lib.at2v_sender_preload(h, None, 0, 0, None) == 0  # n = 0
        assert lib.at2v_sender_preload(h, p, len(pk), 0, None) == 0  # status may be NULL
        assert lib.at2v_sender_preload(h, None, 1, 0, st.ctypes.data) == E_INVALID
        assert lib.at2v_sender_unpin(h, None, 1) == E_INVALID
        assert lib.at2v_sender_query(h, None, 1, st.ctypes.data) == E_INVALID
        assert lib.at2v_sender_query(h, p, 1, None) == E_INVALID
        for flags in (2, 4, 0x80000000, 3):
            assert lib.at2v_sender_preload(h, p, 1, flags, st.ctypes.data) == E_INVALID, flags
        assert lib.at2v_sender_preload(None, p, 1, 0, st.ctypes.data) == E_INVALID
        assert lib.at2v_queue_sender_preload(None, p, 1, 0, st.ctypes.data) == E_INVALID


def test_cpu_queue_preload(at2v_mod, edge_keys):
    from at2v.node import IngestQueue
    pk, want = edge_keys
    lib = at2v_mod.load_library()
    with IngestQueue(cpu=True, cpu_threads=2, max_batch=64) as q:
        for pin in (False, True):
            assert np.array_equal(q.preload_senders(pk, pin=pin), want)
        assert len(q.preload_senders(np.zeros((0, 32), np.uint8))) == 0
        st = np.zeros(1, np.uint8)
        assert lib.at2v_queue_sender_preload(q._h, None, 1, 0, st.ctypes.data) == E_INVALID
        assert lib.at2v_queue_sender_preload(q._h, pk.ctypes.data, 1, 8, st.ctypes.data) == E_INVALID


CHILD = """
import os, sys
sys.path[:0] = [%r, %r]
import numpy as np
import at2v, golden_io
from at2v.node import IngestQueue

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

pk = np.unique(np.ascontiguousarray(golden_io.load("edge").pk).reshape(-1, 32), axis=0)
with at2v.BatchVerifier(num_gpus=0, cpu_threads=2) as v:
    a = v.sender_preload(pk, pin=True)
    assert np.array_equal(v.sender_query(pk), a) and not (a & 3).any()
    v.sender_unpin(pk)
with IngestQueue(cpu=True, cpu_threads=2, max_batch=64) as q:
    assert np.array_equal(q.preload_senders(pk), a)
print("GPU_FDS", gpu_fds())
"""


def test_cpu_backend_opens_no_device():
    """the four calls on a CPU context and a CPU queue in a fresh process: the process never opens the GPU driver's
    device nodes (the HIP runtime opens /dev/kfd when it initialises), with or without a GPU in the machine"""
    import subprocess
    import sys
    code = CHILD % (os.path.join(ROOT, "at2-node_amd"), os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "GPU_FDS []" in out.stdout, out.stdout[-2000:]


def test_symbols_exported_declared_and_abi_still_9(at2v_mod):
    lib = at2v_mod.load_library()
    assert lib.at2v_abi_version() == 9 and at2v_mod.ABI_VERSION == 9
    header = open(os.path.join(ROOT, "include", "at2v.h")).read()
    assert re.search(r"#define\s+AT2V_ABI_VERSION\s+9\b", header)
    raw = ctypes.CDLL(at2v_mod.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in at2v_mod.EXPORTED_SYMBOLS
        assert hasattr(raw, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    for macro, value in (("AT2V_SENDER_PIN", 1), ("AT2V_SENDER_CACHED", 1), ("AT2V_SENDER_PINNED", 2),
                         ("AT2V_SENDER_BAD_KEY", 4)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"u\b", header), macro
    assert (at2v_mod.SENDER_PIN, at2v_mod.SENDER_CACHED, at2v_mod.SENDER_PINNED, at2v_mod.SENDER_BAD_KEY) == (1, 1, 2, 4)
    sys_rs = open(os.path.join(ROOT, "at2v-sys", "src", "lib.rs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"pub fn " + name + r"\s*\(", sys_rs), name


def test_missing_symbol_is_named(at2v_mod, monkeypatch, tmp_path):
    """a library of the same ABI version that predates these calls is refused with the missing symbol's name"""
    monkeypatch.setattr(at2v_mod, "_lib", None)
    monkeypatch.setattr(at2v_mod, "EXPORTED_SYMBOLS", at2v_mod.EXPORTED_SYMBOLS + ("at2v_sender_not_there",))
    with pytest.raises(at2v_mod.At2vError, match="at2v_sender_not_there"):
        at2v_mod.load_library()
