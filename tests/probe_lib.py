"""ctypes binding of the test-only probe library libat2v_probe.so (tests/device/at2v_probe.hip): one call per inline
function of at2-node_amd/csrc, raw limbs and words in, raw limbs and words out, on the host (where = 0) or on device 0
(where = 1). The package Makefile builds it next to libat2v.so; a missing library is an error, not a skip."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "at2-node_amd", "at2v", "libat2v_probe.so")
HOST, DEVICE = 0, 1

_lib = None
_ops = None


def load():
    """the library and {name: (number, in_words, out_words, arg_min, arg_max)}"""
    global _lib, _ops
    if _lib is not None:
        return _lib, _ops
    if not os.path.exists(PATH):
        raise RuntimeError(f"{PATH} not built; run `make -C at2-node_amd` or __graft_entry__.build()")
    try:  # one HIP runtime per process, as at2v._load: torch's copy first where torch is present
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(PATH)
    u32p, ip = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int)
    lib.at2v_probe_count.argtypes = []
    lib.at2v_probe_count.restype = ctypes.c_int
    lib.at2v_probe_info.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ip, ip, ip, ip]
    lib.at2v_probe_info.restype = ctypes.c_int
    lib.at2v_probe_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, u32p, u32p, ctypes.c_int]
    lib.at2v_probe_run.restype = ctypes.c_int
    ops = {}
    for op in range(lib.at2v_probe_count()):
        name = ctypes.c_char_p()
        a, b, lo, hi = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.at2v_probe_info(op, ctypes.byref(name), ctypes.byref(a), ctypes.byref(b), ctypes.byref(lo),
                                   ctypes.byref(hi)) == 0
        ops[name.value.decode()] = (op, a.value, b.value, lo.value, hi.value)
    _lib, _ops = lib, ops
    return _lib, _ops


def run(where: int, name: str, rows, arg: int = 0) -> np.ndarray:
    """one probe over len(rows) cases, a lane each: rows is (n, in_words) of values below 2^32, the result
    (n, out_words) uint32. A batch whose length is a multiple of 64 gets its first case again at the end (dropped from
    the result), so the last wave of every launch is a partial one."""
    lib, ops = load()
    op, nin, nout, lo, hi = ops[name]
    a = np.ascontiguousarray(np.asarray(rows, dtype=np.uint64).astype(np.uint32))
    assert a.ndim == 2 and a.shape[1] == nin and len(a) > 0, (name, a.shape, nin)
    assert lo <= arg <= hi, (name, arg)
    n = len(a)
    if n % 64 == 0:
        a = np.ascontiguousarray(np.concatenate([a, a[:1]]))
    out = np.zeros((len(a), nout), np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    st = lib.at2v_probe_run(where, op, len(a), a.ctypes.data_as(u32p), out.ctypes.data_as(u32p), arg)
    if st != 0:
        raise RuntimeError(f"at2v_probe_run({name}, where={where}) returned {st}")
    assert len(a) % 64 != 0
    return out[:n]
