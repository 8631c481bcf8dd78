"""at2v — Python binding (ctypes) of libat2v.so, the MI355X batch Ed25519 verifier.

Thin plumbing over the C ABI in include/at2v.h, used by the tests and bench.py. The product is the
HIP library. This module has no Python fallback: if libat2v.so is missing, every call raises, and a GPU
context without a gfx950 device raises. The library's own CPU backend (``BatchVerifier(num_gpus=0)``, and the opt-in
``cpu_fallback`` of a GPU context) runs the kernels' verify routine compiled for the host over a thread pool; it never
routes through the oracle. ``verify_one`` is the per-signature entry point, a CPU function by contract.

Reference interface mirrored (drop::crypto::sign, used by at2-node at src/lib.rs:5,19,
src/client.rs:72-78, src/bin/server/rpc.rs:269,281):
  * ``Signature.verify(message, public_key)`` raises ``VerifyError`` on a bad signature, like
    drop's ``Signature::verify(&self, &T, &PublicKey) -> Result<(), VerifyError>``;
  * ``BatchVerifier.verify_batch(...)`` is the batch form the server ingest uses.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libat2v.so")

POLICY_DALEK_V1 = 0
POLICY_LIBSODIUM_1_0_18 = 1
POLICY_DALEK_V1_LEGACY = 2  # dalek built with `legacy_compatibility`: V1 is "the three top bits of S clear", s unreduced
POLICY_ZIP215 = 4  # the cofactored rule of ZIP-215: s < l, A and R decoded permissively, [8]([s]B - [k]A - R) = 0 (3: unassigned)
_POLICIES = {"dalek": POLICY_DALEK_V1, "dalek_v1": POLICY_DALEK_V1, "libsodium": POLICY_LIBSODIUM_1_0_18,
             "libsodium_1_0_18": POLICY_LIBSODIUM_1_0_18, "dalek-legacy": POLICY_DALEK_V1_LEGACY,
             "dalek_v1_legacy": POLICY_DALEK_V1_LEGACY, POLICY_DALEK_V1: POLICY_DALEK_V1,
             POLICY_LIBSODIUM_1_0_18: POLICY_LIBSODIUM_1_0_18, POLICY_DALEK_V1_LEGACY: POLICY_DALEK_V1_LEGACY,
             "zip215": POLICY_ZIP215, POLICY_ZIP215: POLICY_ZIP215}
# include/at2v.h AT2V_MASK_*: bit p of a policy-mask byte is set iff policy p accepts the record
MASK_DALEK_V1, MASK_LIBSODIUM, MASK_DALEK_V1_LEGACY = 1, 2, 4

# must match include/at2v.h (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = ("at2v_abi_version", "at2v_create", "at2v_destroy", "at2v_verify_batch", "at2v_verify_batch_device",
                    "at2v_verify_one", "at2v_verify_one_policy", "at2v_strerror", "at2v_gen_records_device",
                    "at2v_reject_reasons", "at2v_reject_reasons_device", "at2v_verify_one_reason", "at2v_reason_name",
                    "at2v_queue_poll_reasons", "at2v_policy_mask", "at2v_policy_mask_device",
                    "at2v_gen_records_senders_device", "at2v_gen_records_keys_device", "at2v_sign_batch", "at2v_get_info", "at2v_decode_points",
                    "at2v_comm_get_unique_id", "at2v_comm_init_rank", "at2v_verify_shard_gather_device",
                    "at2v_verify_batch_sharded", "at2v_verify_batch_submit", "at2v_verify_batch_wait",
                    "at2v_host_alloc", "at2v_host_free", "at2v_host_register", "at2v_host_unregister",
                    "at2v_sender_preload", "at2v_sender_unpin", "at2v_sender_query", "at2v_queue_sender_preload",
                    "at2v_transfers_workspace_bytes", "at2v_verify_transfers_device", "at2v_verify_transfers",
                    "at2v_verify_transfers_submit", "at2v_queue_submit_transfers",
                    "at2v_queue_create", "at2v_queue_destroy", "at2v_queue_submit", "at2v_queue_flush",
                    "at2v_queue_poll", "at2v_queue_get_stats", "at2v_queue_reset_latency",
                    "at2v_pack_send_asset",
                    "at2v_ledger_create", "at2v_ledger_destroy", "at2v_ledger_balance", "at2v_ledger_last_sequence",
                    "at2v_ledger_transfer", "at2v_ledger_recent_put", "at2v_ledger_recent_get",
                    "at2v_ledger_deliver", "at2v_ledger_pending")


def _second_pass_args(pk, sig, verdict_words):
    """pk, sig and the verdict words (uint32 words, or bool[n] verdicts) of a pass that follows a verify call"""
    pk = np.ascontiguousarray(pk, dtype=np.uint8)
    sig = np.ascontiguousarray(sig, dtype=np.uint8)
    n = pk.size // 32
    w = np.asarray(verdict_words)
    if w.dtype == bool:
        if w.shape != (n,):
            raise ValueError("bool verdicts must have one entry per record")
        b = np.packbits(w.astype(np.uint8), bitorder="little")
        w = np.concatenate([b, np.zeros((-len(b)) % 4, np.uint8)]).view("<u4")
    words = np.ascontiguousarray(w, dtype=np.uint32).reshape(-1)
    if pk.size != 32 * n or sig.size != 64 * n or words.size < (n + 31) // 32:
        raise ValueError("pk/sig/verdict_words sizes disagree")
    return pk, sig, n, words


class At2vError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        super().__init__(f"at2v error {code}: {strerror(code)}{(' (' + what + ')') if what else ''}")
        self.code = code


# include/at2v.h at2v_reason: why a record was rejected (0 = it was not)
REASON_VALID, REASON_A_DECODE, REASON_S_RANGE, REASON_A_POLICY, REASON_R_POLICY, REASON_R_ENCODING, REASON_EQUATION = \
    range(7)
REASON_UNKNOWN = 0xFF  # the call or the batch failed: neither valid nor invalid


def reason_name(reason: int) -> str:
    """at2v_reason_name: a short description of an at2v_reason"""
    return load_library().at2v_reason_name(int(reason)).decode()


class VerifyError(Exception):
    """Signature rejected (drop::crypto::sign::VerifyError). `reason` is the at2v_reason (REASON_*): 1 is what the
    reference answers with InvalidArgument at ingest (an undecodable sender key), 2..6 a payload never delivered."""

    def __init__(self, message: str = "signature verification failed", reason: int = REASON_UNKNOWN):
        super().__init__(message)
        self.reason = reason


ABI_VERSION = 9  # include/at2v.h AT2V_ABI_VERSION: the struct layouts below are those of this version
E_PEER = -7      # AT2V_E_PEER: another rank of the communicator failed this collective batch


class _Opts(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("num_gpus", ctypes.c_int), ("policy", ctypes.c_int),
                ("small_batch_max", ctypes.c_uint32), ("sender_cache", ctypes.c_uint32),
                ("sender_comb", ctypes.c_uint32), ("cpu_threads", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


CTX_CPU_FALLBACK = 1   # include/at2v.h AT2V_CTX_CPU_FALLBACK: a failed GPU batch (host buffers) re-runs on the CPU backend
CTX_ADMIT_FIRST = 2    # include/at2v.h AT2V_CTX_ADMIT_FIRST: sender-cache keys claim a payload at their first sighting
CTX_BCOMB_WIDE = 4     # include/at2v.h AT2V_CTX_BCOMB_WIDE: with combs, also a 24-bit-window comb of B (11.8 GB)


WIRE_BYTES, WIRE_ARRAY = 0, 1  # include/at2v.h AT2V_WIRE_*: how a transfer's recipient key is serialised in its message

SMALL_BATCH_DEFAULT = 32768    # include/at2v.h AT2V_SMALL_BATCH_DEFAULT
SMALL_BATCH_OFF = 0xFFFFFFFF    # include/at2v.h AT2V_SMALL_BATCH_OFF: never use the low-latency kernel


class _Info(ctypes.Structure):
    _fields_ = [("num_gpus", ctypes.c_int), ("grid_blocks", ctypes.c_int), ("block_threads", ctypes.c_int),
                ("waves_per_cu", ctypes.c_int), ("cus", ctypes.c_int), ("vgprs", ctypes.c_int),
                ("rank", ctypes.c_int), ("world", ctypes.c_int), ("gathers", ctypes.c_uint64),
                ("cache_entries", ctypes.c_uint64), ("cache_chunks", ctypes.c_uint64),
                ("cache_chunk_hits", ctypes.c_uint64), ("cache_capacity", ctypes.c_uint64),
                ("cache_claims", ctypes.c_uint64), ("cache_evicted", ctypes.c_uint64),
                ("cache_compactions", ctypes.c_uint64), ("cpu_threads", ctypes.c_uint64),
                ("cpu_batches", ctypes.c_uint64), ("cpu_fallbacks", ctypes.c_uint64),
                ("cache_sightings", ctypes.c_uint64), ("cache_built", ctypes.c_uint64),
                ("cache_build_us", ctypes.c_uint64), ("cache_record_hits", ctypes.c_uint64),
                ("experiments", ctypes.c_uint64), ("host_chunks", ctypes.c_uint64),
                ("host_direct_bytes", ctypes.c_uint64), ("host_staged_bytes", ctypes.c_uint64)]


UNIQUE_ID_BYTES = 128  # AT2V_UNIQUE_ID_BYTES (RCCL ncclUniqueId)

SENDER_PIN = 1      # include/at2v.h AT2V_SENDER_PIN: flag of at2v_sender_preload
SENDER_CACHED = 1   # status bits of the known-senders calls, one byte per key: cached on every device of the context
SENDER_PINNED = 2   # ... and no replacement pass evicts it
SENDER_BAD_KEY = 4  # the 32 bytes do not decode under dalek's rules (records of such a key are rejected)


_lib = None
_loading = False


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libat2v.so (raises if it is missing: there is no fallback)."""
    global _lib, _loading
    if _lib is not None:
        return _lib
    _loading = True
    try:
        _lib = _load(path)
    finally:
        _loading = False
    return _lib


def _load(path: str) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise At2vError(-2, f"{path} not built; run `make -C at2-node_amd` or __graft_entry__.build()")
    # One HIP runtime per process: torch bundles its own libamdhip64 (same SONAME as ROCm's). If torch is
    # present it must be loaded first so libat2v.so binds to the same runtime and torch streams/pointers
    # passed to the *_device entry points belong to the runtime that launches our kernels.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    lib.at2v_abi_version.argtypes = []
    lib.at2v_abi_version.restype = ctypes.c_int
    if lib.at2v_abi_version() != ABI_VERSION:  # the structs below would not match the library's
        raise At2vError(-1, f"{path} has ABI version {lib.at2v_abi_version()}, this binding needs {ABI_VERSION}")
    # functions added within this ABI version (the known-senders calls): a library of the same version may predate them
    for name in EXPORTED_SYMBOLS:
        if not hasattr(lib, name):
            raise At2vError(-1, f"{path} does not export {name}; rebuild it from this tree")
    P, u8p, u32p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    lib.at2v_create.argtypes = [ctypes.POINTER(_Opts), ctypes.POINTER(P)]
    lib.at2v_create.restype = ctypes.c_int
    lib.at2v_destroy.argtypes = [P]
    lib.at2v_destroy.restype = None
    lib.at2v_verify_batch.argtypes = [P, P, P, P, P, ctypes.c_size_t, P]
    lib.at2v_verify_batch.restype = ctypes.c_int
    lib.at2v_verify_batch_submit.argtypes = [P, P, P, P, P, ctypes.c_size_t, P, ctypes.POINTER(ctypes.c_uint64)]
    lib.at2v_verify_batch_submit.restype = ctypes.c_int
    lib.at2v_verify_batch_wait.argtypes = [P, ctypes.c_uint64]
    lib.at2v_verify_batch_wait.restype = ctypes.c_int
    lib.at2v_host_alloc.argtypes = [P, ctypes.c_size_t, ctypes.POINTER(P)]
    lib.at2v_host_alloc.restype = ctypes.c_int
    lib.at2v_host_free.argtypes = [P, P]
    lib.at2v_host_free.restype = ctypes.c_int
    lib.at2v_host_register.argtypes = [P, P, ctypes.c_size_t]
    lib.at2v_host_register.restype = ctypes.c_int
    lib.at2v_host_unregister.argtypes = [P, P]
    lib.at2v_host_unregister.restype = ctypes.c_int
    lib.at2v_sender_preload.argtypes = [P, P, ctypes.c_size_t, ctypes.c_uint32, P]
    lib.at2v_sender_preload.restype = ctypes.c_int
    lib.at2v_sender_unpin.argtypes = [P, P, ctypes.c_size_t]
    lib.at2v_sender_unpin.restype = ctypes.c_int
    lib.at2v_sender_query.argtypes = [P, P, ctypes.c_size_t, P]
    lib.at2v_sender_query.restype = ctypes.c_int
    lib.at2v_verify_batch_device.argtypes = [P, P, P, P, ctypes.c_size_t, P, ctypes.c_size_t, P, P]
    lib.at2v_verify_batch_device.restype = ctypes.c_int
    lib.at2v_transfers_workspace_bytes.argtypes = [ctypes.c_size_t, ctypes.c_int]
    lib.at2v_transfers_workspace_bytes.restype = ctypes.c_size_t
    lib.at2v_verify_transfers_device.argtypes = [P, P, P, P, P, ctypes.c_size_t, ctypes.c_int, P, ctypes.c_size_t, P,
                                                 P, P]
    lib.at2v_verify_transfers_device.restype = ctypes.c_int
    lib.at2v_verify_transfers.argtypes = [P, P, P, P, P, ctypes.c_size_t, ctypes.c_int, P, P]
    lib.at2v_verify_transfers.restype = ctypes.c_int
    lib.at2v_verify_transfers_submit.argtypes = [P, P, P, P, P, ctypes.c_size_t, ctypes.c_int, P, P,
                                                 ctypes.POINTER(ctypes.c_uint64)]
    lib.at2v_verify_transfers_submit.restype = ctypes.c_int
    lib.at2v_verify_one.argtypes = [P, P, P, ctypes.c_size_t]
    lib.at2v_verify_one.restype = ctypes.c_int
    lib.at2v_verify_one_policy.argtypes = [P, P, P, ctypes.c_size_t, ctypes.c_int]
    lib.at2v_verify_one_policy.restype = ctypes.c_int
    lib.at2v_comm_get_unique_id.argtypes = [P]
    lib.at2v_comm_get_unique_id.restype = ctypes.c_int
    lib.at2v_comm_init_rank.argtypes = [P, P, ctypes.c_int, ctypes.c_int]
    lib.at2v_comm_init_rank.restype = ctypes.c_int
    lib.at2v_verify_shard_gather_device.argtypes = [P, P, P, P, ctypes.c_size_t, P, ctypes.c_size_t, ctypes.c_size_t,
                                                    P, P]
    lib.at2v_verify_shard_gather_device.restype = ctypes.c_int
    lib.at2v_verify_batch_sharded.argtypes = [P, P, P, P, P, ctypes.c_size_t, P]
    lib.at2v_verify_batch_sharded.restype = ctypes.c_int
    lib.at2v_strerror.argtypes = [ctypes.c_int]
    lib.at2v_strerror.restype = ctypes.c_char_p
    lib.at2v_gen_records_device.argtypes = [P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_uint32,
                                            P, P, P, P, P]
    lib.at2v_gen_records_device.restype = ctypes.c_int
    lib.at2v_gen_records_senders_device.argtypes = [P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_size_t,
                                                    ctypes.c_uint32, ctypes.c_uint64, P, P, P, P, P]
    lib.at2v_gen_records_senders_device.restype = ctypes.c_int
    lib.at2v_gen_records_keys_device.argtypes = [P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_size_t,
                                                 ctypes.c_uint32, P, P, P, P, P, P]
    lib.at2v_gen_records_keys_device.restype = ctypes.c_int
    lib.at2v_sign_batch.argtypes = [P, P, P, P, ctypes.c_size_t, P, P]
    lib.at2v_sign_batch.restype = ctypes.c_int
    lib.at2v_get_info.argtypes = [P, ctypes.POINTER(_Info)]
    lib.at2v_get_info.restype = ctypes.c_int
    lib.at2v_decode_points.argtypes = [P, P, ctypes.c_size_t, P]
    lib.at2v_decode_points.restype = ctypes.c_int
    lib.at2v_reject_reasons.argtypes = [P, P, P, ctypes.c_size_t, P, P]
    lib.at2v_reject_reasons.restype = ctypes.c_int
    lib.at2v_reject_reasons_device.argtypes = [P, P, P, ctypes.c_size_t, P, P, P]
    lib.at2v_reject_reasons_device.restype = ctypes.c_int
    lib.at2v_policy_mask.argtypes = [P, P, P, ctypes.c_size_t, P, P]
    lib.at2v_policy_mask.restype = ctypes.c_int
    lib.at2v_policy_mask_device.argtypes = [P, P, P, ctypes.c_size_t, P, P, P]
    lib.at2v_policy_mask_device.restype = ctypes.c_int
    lib.at2v_verify_one_reason.argtypes = [P, P, P, ctypes.c_size_t, ctypes.c_int]
    lib.at2v_verify_one_reason.restype = ctypes.c_int
    lib.at2v_reason_name.argtypes = [ctypes.c_int]
    lib.at2v_reason_name.restype = ctypes.c_char_p
    from . import node as _node  # queue / packer / ledger signatures
    _node.bind(lib)
    return lib


def strerror(code: int) -> str:
    if _loading:  # (an error raised while loading must not load again)
        return "library not loaded"
    try:
        return load_library().at2v_strerror(code).decode()
    except At2vError:
        return "library not loaded"


def _check(rc: int, what: str = "") -> int:
    if rc < 0:
        raise At2vError(rc, what)
    return rc


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data if a.size else 0


def unpack_verdicts(words: np.ndarray, n: int) -> np.ndarray:
    """verdict words (bit i%32 of word i/32) -> bool[n]"""
    bits = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")
    return bits[:n].astype(bool)


def pack_records(pks: Sequence[bytes], sigs: Sequence[bytes], msgs: Sequence[bytes]):
    """lists of bytes -> (pk[n,32], sig[n,64], msg u8[], off u32[n+1]) in the ABI layout"""
    n = len(pks)
    pk = np.frombuffer(b"".join(pks), dtype=np.uint8).reshape(n, 32) if n else np.zeros((0, 32), np.uint8)
    sig = np.frombuffer(b"".join(sigs), dtype=np.uint8).reshape(n, 64) if n else np.zeros((0, 64), np.uint8)
    off = np.zeros(n + 1, dtype=np.uint32)
    if n:
        off[1:] = np.cumsum([len(m) for m in msgs])
    msg = np.frombuffer(b"".join(msgs), dtype=np.uint8) if n else np.zeros(0, np.uint8)
    return pk, sig, msg, off


def launch_streams(count: int = 2, device: Optional[int] = None) -> list:
    """`count` non-blocking HIP streams (hipStreamCreateWithFlags) on `device` (current if None), as
    torch.cuda.ExternalStream objects. Verify launches alternating over them overlap: the context's scratch sets let
    launch k+1 take the CUs launch k leaves during its end-of-launch drain (at2v_api_launch.h). Each stream the runtime
    creates gets its own hardware queue in turn, which is what lets the two kernels run side by side."""
    import torch

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    out = []
    with torch.cuda.device(torch.cuda.current_device() if device is None else device):
        for _ in range(count):
            h = ctypes.c_void_p()
            rc = hip.hipStreamCreateWithFlags(ctypes.byref(h), 1)  # hipStreamNonBlocking
            if rc != 0:
                raise At2vError(-3, f"hipStreamCreateWithFlags failed ({rc})")
            out.append(torch.cuda.ExternalStream(h.value))
    return out


class _PinnedBlock:
    """Memory handed out by at2v_host_alloc, exposed through the array interface: the array made from it (and every
    view of that array) holds this object, and this object holds the verifier."""

    def __init__(self, owner: "BatchVerifier", address: int, nbytes: int):
        self.owner, self.address, self.nbytes = owner, address, nbytes
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (address, False), "version": 3}


class PendingBatch:
    """A submitted host-buffer batch (BatchVerifier.submit_batch): its ticket, verdict words and the arrays the library
    reads until the wait."""

    def __init__(self, ticket: int, n: int, words: np.ndarray, refs: tuple,
                 recipient_words: Optional[np.ndarray] = None):
        self.ticket, self.n, self.words, self._refs = ticket, n, words, refs
        self.recipient_words = recipient_words  # submit_transfers(recipient_ok=True): final after wait_batch

    def recipient_ok(self) -> np.ndarray:
        """bool[n]: which recipients decode (a transfers call submitted with recipient_ok; valid after wait_batch)"""
        if self.recipient_words is None:
            raise ValueError("this call was not submitted with recipient_ok")
        return unpack_verdicts(self.recipient_words, self.n)


class BatchVerifier:
    """Owns an at2v context: one or more gfx950 devices, or (num_gpus=0) the library's CPU batch backend."""

    def __init__(self, device: int = 0, num_gpus: int = 1, policy="dalek", small_batch_max: int = 0,
                 sender_cache: int = 0, sender_comb: bool = False, cpu_threads: int = 0, cpu_fallback: bool = False,
                 admit_first: bool = False, bcomb_wide: bool = False):
        """small_batch_max: launches of at most this many records run the low-latency kernel (two lanes per record);
        0 = the library default (SMALL_BATCH_DEFAULT), SMALL_BATCH_OFF = always the throughput kernel.
        sender_cache: capacity of the per-sender A cache in distinct public keys (0 = off).
        sender_comb: with sender_cache, also keep a comb of -A per cached key (1.7 MB of HBM each, plus combs of B of 67
        MB and 872 MB per context; include/at2v.h): records whose sender is cached verify by table additions only
        (at2v_comb.h), launches of every size. bcomb_wide: with sender_comb, the throughput kernel's comb of B gets 24-bit
        windows (11.8 GB, two additions fewer per cached record; AT2V_CTX_BCOMB_WIDE).
        num_gpus=0: the CPU batch backend (no device; cpu_threads host threads, 0 = every usable CPU).
        cpu_fallback: a GPU context re-runs a host-buffer batch on the CPU backend after a device error (same verdicts;
        info()["cpu_fallbacks"] counts it). admit_first: cache keys claim a payload at their first sighting."""
        self._lib = load_library()
        self.policy = _POLICIES[policy]
        flags = ((CTX_CPU_FALLBACK if cpu_fallback else 0) | (CTX_ADMIT_FIRST if admit_first else 0)
                 | (CTX_BCOMB_WIDE if bcomb_wide else 0))
        opts = _Opts(device, num_gpus, self.policy, small_batch_max, sender_cache, 1 if sender_comb else 0,
                     cpu_threads, flags)
        h = ctypes.c_void_p()
        _check(self._lib.at2v_create(ctypes.byref(opts), ctypes.byref(h)), "at2v_create")
        self._h = h
        self._registered = {}  # host_register: address -> the array (kept alive while the library may read it)

    def close(self):
        """at2v_destroy: also frees what host_alloc handed out (arrays made from it must not be used afterwards) and
        unregisters what is still registered"""
        if getattr(self, "_h", None):
            self._lib.at2v_destroy(self._h)
            self._h = None
            self._registered = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self) -> dict:
        inf = _Info()
        _check(self._lib.at2v_get_info(self._h, ctypes.byref(inf)), "at2v_get_info")
        return {f: getattr(inf, f) for f, _ in _Info._fields_}

    # ---- pinned host memory (include/at2v.h at2v_host_*): records that lie in it are uploaded without a host copy
    def host_alloc(self, nbytes: int) -> np.ndarray:
        """at2v_host_alloc: `nbytes` of pinned memory (64-byte aligned, visible to every device of the context; plain
        host memory on a CPU context) as a uint8 array. Carve pk / sig / msg (and the verdict words) out of it with
        slices and views: verify_batch uploads what lies in it straight from there. The array keeps the verifier
        alive; host_free (or close) releases the memory."""
        p = ctypes.c_void_p()
        _check(self._lib.at2v_host_alloc(self._h, int(nbytes), ctypes.byref(p)), "at2v_host_alloc")
        return np.asarray(_PinnedBlock(self, p.value, int(nbytes)))

    def host_free(self, arr: np.ndarray) -> None:
        """at2v_host_free: `arr` is the array host_alloc returned (or a view that starts at its first byte); it and
        its views must not be used afterwards"""
        _check(self._lib.at2v_host_free(self._h, arr.ctypes.data), "at2v_host_free")

    def host_register(self, arr: np.ndarray) -> None:
        """at2v_host_register: pin the C-contiguous array's bytes in place (any alignment) and make them known to the
        context. The verifier holds the array until host_unregister."""
        if not arr.flags.c_contiguous or arr.nbytes == 0:
            raise ValueError("host_register needs a non-empty C-contiguous array")
        _check(self._lib.at2v_host_register(self._h, arr.ctypes.data, arr.nbytes), "at2v_host_register")
        self._registered[arr.ctypes.data] = arr

    def host_unregister(self, arr: np.ndarray) -> None:
        """at2v_host_unregister: `arr` starts at the first byte of a registered array"""
        _check(self._lib.at2v_host_unregister(self._h, arr.ctypes.data), "at2v_host_unregister")
        self._registered.pop(arr.ctypes.data, None)

    # ---- known senders (include/at2v.h at2v_sender_*): tell the sender cache who will send, instead of waiting for it
    # to learn keys from traffic
    def sender_preload(self, pk: np.ndarray, pin: bool = False) -> np.ndarray:
        """at2v_sender_preload: cache the listed keys (n x 32 bytes) on every device now, so the next launch serves their
        records from the cache; pin: no replacement pass evicts them. Returns a status byte per key (SENDER_CACHED |
        SENDER_PINNED | SENDER_BAD_KEY). At most sender_cache / 2 distinct keys per call, and as many pinned keys in
        all. A context without a sender cache (or the CPU backend) caches nothing and reports only SENDER_BAD_KEY."""
        pk = np.ascontiguousarray(pk, dtype=np.uint8).reshape(-1, 32)
        status = np.zeros(max(1, len(pk)), np.uint8)
        _check(self._lib.at2v_sender_preload(self._h, _ptr(pk) or None, len(pk), SENDER_PIN if pin else 0,
                                             _ptr(status)), "at2v_sender_preload")
        return status[:len(pk)]

    def sender_unpin(self, pk: np.ndarray) -> None:
        """at2v_sender_unpin: the listed keys lose their pin (unknown keys are ignored); their entries stay until the
        replacement takes them"""
        pk = np.ascontiguousarray(pk, dtype=np.uint8).reshape(-1, 32)
        _check(self._lib.at2v_sender_unpin(self._h, _ptr(pk) or None, len(pk)), "at2v_sender_unpin")

    def sender_query(self, pk: np.ndarray) -> np.ndarray:
        """at2v_sender_query: a status byte per key, read-only (asking does not keep a key alive)"""
        pk = np.ascontiguousarray(pk, dtype=np.uint8).reshape(-1, 32)
        status = np.zeros(max(1, len(pk)), np.uint8)
        _check(self._lib.at2v_sender_query(self._h, _ptr(pk) or None, len(pk), _ptr(status)), "at2v_sender_query")
        return status[:len(pk)]

    @staticmethod
    def _verdict_words(n: int, words: Optional[np.ndarray]) -> np.ndarray:
        """the caller's verdict words (uint32, C-contiguous, at least ceil(n/32)), or fresh ones"""
        if words is None:
            return np.zeros(max(1, (n + 31) // 32), dtype=np.uint32)
        if words.dtype != np.uint32 or not words.flags.c_contiguous or words.size < max(1, (n + 31) // 32):
            raise ValueError("words must be a C-contiguous uint32 array of at least ceil(n/32) entries")
        return words

    def verify_batch(self, pk: np.ndarray, sig: np.ndarray, msg: np.ndarray, msg_off: np.ndarray,
                     words: Optional[np.ndarray] = None) -> np.ndarray:
        """host arrays -> bool[n] verdicts. Arrays that are uint8 (msg_off: uint32) and C-contiguous are passed as they
        are, so records in host_alloc / host_register memory are uploaded from there. words: the verdict words go into
        this uint32 array (e.g. a view of host_alloc memory) instead of a fresh one."""
        pk = np.ascontiguousarray(pk, dtype=np.uint8)
        sig = np.ascontiguousarray(sig, dtype=np.uint8)
        msg = np.ascontiguousarray(msg, dtype=np.uint8).reshape(-1)
        msg_off = np.ascontiguousarray(msg_off, dtype=np.uint32)
        n = len(msg_off) - 1
        if pk.size != 32 * n or sig.size != 64 * n:
            raise ValueError("pk/sig/msg_off sizes disagree")
        words = self._verdict_words(n, words)
        msg_arg = msg if msg.size else np.zeros(1, np.uint8)
        _check(self._lib.at2v_verify_batch(self._h, _ptr(pk), _ptr(sig), _ptr(msg_arg), _ptr(msg_off), n,
                                           _ptr(words)), "at2v_verify_batch")
        return unpack_verdicts(words, n)

    def submit_batch(self, pk: np.ndarray, sig: np.ndarray, msg: np.ndarray, msg_off: np.ndarray,
                     words: Optional[np.ndarray] = None) -> "PendingBatch":
        """at2v_verify_batch_submit: stage the batch and enqueue its verification; returns the pending call (it holds
        the arrays until wait_batch). At most two in flight per context."""
        pk = np.ascontiguousarray(pk, dtype=np.uint8)
        sig = np.ascontiguousarray(sig, dtype=np.uint8)
        msg = np.ascontiguousarray(msg, dtype=np.uint8).reshape(-1)
        msg_off = np.ascontiguousarray(msg_off, dtype=np.uint32)
        n = len(msg_off) - 1
        if pk.size != 32 * n or sig.size != 64 * n:
            raise ValueError("pk/sig/msg_off sizes disagree")
        words = self._verdict_words(n, words)
        msg_arg = msg if msg.size else np.zeros(1, np.uint8)
        t = ctypes.c_uint64(0)
        _check(self._lib.at2v_verify_batch_submit(self._h, _ptr(pk), _ptr(sig), _ptr(msg_arg), _ptr(msg_off), n,
                                                  _ptr(words), ctypes.byref(t)), "at2v_verify_batch_submit")
        return PendingBatch(t.value, n, words, (pk, sig, msg_arg, msg_off))

    def wait_batch(self, pending: "PendingBatch") -> np.ndarray:
        """at2v_verify_batch_wait -> bool[n] verdicts of a submitted batch"""
        _check(self._lib.at2v_verify_batch_wait(self._h, pending.ticket), "at2v_verify_batch_wait")
        return unpack_verdicts(pending.words, pending.n)

    def verify_batch_device(self, d_pk: int, d_sig: int, d_msg: int, msg_bytes: int, d_off: int, n: int,
                            d_verdicts: int, stream: int = 0) -> None:
        """device pointers (e.g. torch tensor data_ptr()), asynchronous on `stream` (a hipStream_t)"""
        _check(self._lib.at2v_verify_batch_device(self._h, d_pk, d_sig, d_msg, msg_bytes, d_off, n, d_verdicts,
                                                  stream or None), "at2v_verify_batch_device")

    # ---- AT2 transfers from their fields (include/at2v.h at2v_verify_transfers*): the node's ledger arrays go in as
    # they are, the messages bincode(ThinTransaction{recipient, amount}) are built by the library
    @staticmethod
    def _transfer_fields(sender, sig, recipient, amount):
        sender = np.ascontiguousarray(sender, dtype=np.uint8)
        sig = np.ascontiguousarray(sig, dtype=np.uint8)
        recipient = np.ascontiguousarray(recipient, dtype=np.uint8)
        amount = np.ascontiguousarray(amount, dtype=np.uint64).reshape(-1)
        n = amount.size
        if sender.size != 32 * n or sig.size != 64 * n or recipient.size != 32 * n:
            raise ValueError("sender/sig/recipient/amount sizes disagree")
        return sender, sig, recipient, amount, n

    def _transfer_outputs(self, n: int, words, recipient_ok, recipient_words):
        words = self._verdict_words(n, words)
        if recipient_words is not None:
            recipient_words = self._verdict_words(n, recipient_words)
        elif recipient_ok:
            recipient_words = self._verdict_words(n, None)
        return words, recipient_words

    @staticmethod
    def transfers_workspace_bytes(n: int, wire: int = WIRE_BYTES) -> int:
        """at2v_transfers_workspace_bytes: device bytes verify_transfers_device needs for n transfers (0: a bad wire, or
        an n the device form refuses)"""
        return int(load_library().at2v_transfers_workspace_bytes(int(n), int(wire)))

    def verify_transfers(self, sender: np.ndarray, sig: np.ndarray, recipient: np.ndarray, amount: np.ndarray,
                         wire: int = WIRE_BYTES, recipient_ok: bool = False, words: Optional[np.ndarray] = None,
                         recipient_words: Optional[np.ndarray] = None):
        """at2v_verify_transfers: sender [n,32], sig [n,64], recipient [n,32] (uint8) and amount [n] (uint64) -> bool[n]
        verdicts, those of verify_batch over the messages bincode(ThinTransaction{recipient, amount}). recipient_ok
        (or a recipient_words array): also which recipients decode, returned as a second bool[n]. words /
        recipient_words: the output words go into these uint32 arrays instead of fresh ones. Arrays of the right dtype
        that are C-contiguous are passed as they are (host_alloc memory is uploaded from there)."""
        sender, sig, recipient, amount, n = self._transfer_fields(sender, sig, recipient, amount)
        words, rw = self._transfer_outputs(n, words, recipient_ok, recipient_words)
        _check(self._lib.at2v_verify_transfers(self._h, _ptr(sender) or None, _ptr(sig) or None, _ptr(recipient) or None,
                                               _ptr(amount) or None, n, int(wire), _ptr(words),
                                               None if rw is None else _ptr(rw)), "at2v_verify_transfers")
        v = unpack_verdicts(words, n)
        return v if rw is None else (v, unpack_verdicts(rw, n))

    def submit_transfers(self, sender: np.ndarray, sig: np.ndarray, recipient: np.ndarray, amount: np.ndarray,
                         wire: int = WIRE_BYTES, recipient_ok: bool = False, words: Optional[np.ndarray] = None,
                         recipient_words: Optional[np.ndarray] = None) -> "PendingBatch":
        """at2v_verify_transfers_submit: the pending call (wait_batch returns its verdicts, then
        PendingBatch.recipient_ok() its recipient bits). Shares the two call slots with submit_batch."""
        sender, sig, recipient, amount, n = self._transfer_fields(sender, sig, recipient, amount)
        words, rw = self._transfer_outputs(n, words, recipient_ok, recipient_words)
        t = ctypes.c_uint64(0)
        _check(self._lib.at2v_verify_transfers_submit(self._h, _ptr(sender) or None, _ptr(sig) or None,
                                                      _ptr(recipient) or None, _ptr(amount) or None, n, int(wire),
                                                      _ptr(words), None if rw is None else _ptr(rw), ctypes.byref(t)),
               "at2v_verify_transfers_submit")
        return PendingBatch(t.value, n, words, (sender, sig, recipient, amount), rw)

    def verify_transfers_device(self, d_sender: int, d_sig: int, d_recipient: int, d_amount: int, n: int, wire: int,
                                d_work: int, work_bytes: int, d_verdicts: int, d_recipient_ok: int = 0,
                                stream: int = 0) -> None:
        """at2v_verify_transfers_device: device pointers, asynchronous on `stream`; d_work: work_bytes >=
        transfers_workspace_bytes(n, wire) of 16-byte-aligned device memory the call may use until the stream gets
        there; d_recipient_ok: 0 = not asked for"""
        _check(self._lib.at2v_verify_transfers_device(self._h, d_sender, d_sig, d_recipient, d_amount, n, int(wire),
                                                      d_work, work_bytes, d_verdicts, d_recipient_ok or None,
                                                      stream or None), "at2v_verify_transfers_device")

    # ---- one rank per GPU: RCCL all-gather of the verdict words (include/at2v.h)
    def comm_init_rank(self, unique_id: bytes, rank: int, world: int) -> None:
        """Attach an RCCL communicator (collective over `world` processes; unique_id from comm_unique_id() on
        rank 0, shared out of band)."""
        if len(unique_id) != UNIQUE_ID_BYTES:
            raise ValueError("unique id must be %d bytes" % UNIQUE_ID_BYTES)
        _check(self._lib.at2v_comm_init_rank(self._h, bytes(unique_id), rank, world), "at2v_comm_init_rank")

    def verify_shard_gather_device(self, d_pk: int, d_sig: int, d_msg: int, msg_bytes: int, d_off: int,
                                   n_local: int, words_per_rank: int, d_bitmap: int, stream: int = 0) -> None:
        """verify this rank's n_local device records into its slice of d_bitmap, then all-gather (asynchronous)"""
        _check(self._lib.at2v_verify_shard_gather_device(self._h, d_pk or None, d_sig or None, d_msg or None,
                                                         msg_bytes, d_off or None, n_local, words_per_rank,
                                                         d_bitmap, stream or None),
               "at2v_verify_shard_gather_device")

    def verify_batch_sharded(self, pk: np.ndarray, sig: np.ndarray, msg: np.ndarray, msg_off: np.ndarray,
                             words: Optional[np.ndarray] = None) -> np.ndarray:
        """the node batch (same on every rank) -> bool[n] verdicts of the whole batch on every rank"""
        pk = np.ascontiguousarray(pk, dtype=np.uint8)
        sig = np.ascontiguousarray(sig, dtype=np.uint8)
        msg = np.ascontiguousarray(msg, dtype=np.uint8).reshape(-1)
        msg_off = np.ascontiguousarray(msg_off, dtype=np.uint32)
        n = len(msg_off) - 1
        if pk.size != 32 * n or sig.size != 64 * n:
            raise ValueError("pk/sig/msg_off sizes disagree")
        words = self._verdict_words(n, words)
        msg_arg = msg if msg.size else np.zeros(1, np.uint8)
        _check(self._lib.at2v_verify_batch_sharded(self._h, _ptr(pk), _ptr(sig), _ptr(msg_arg), _ptr(msg_off), n,
                                                   _ptr(words)), "at2v_verify_batch_sharded")
        return unpack_verdicts(words, n)

    def gen_records_device(self, cfg_seed: int, first: int, n: int, msg_len: int, d_pk: int, d_sig: int, d_msg: int,
                           d_off: Optional[int], stream: int = 0, senders: int = 0) -> None:
        """GPU generator; senders > 0: record i is signed by sender (first + i) % senders"""
        if senders:
            _check(self._lib.at2v_gen_records_senders_device(self._h, cfg_seed, first, n, msg_len, senders, d_pk, d_sig,
                                                             d_msg, d_off or None, stream or None),
                   "at2v_gen_records_senders_device")
            return
        _check(self._lib.at2v_gen_records_device(self._h, cfg_seed, first, n, msg_len, d_pk, d_sig, d_msg,
                                                 d_off or None, stream or None), "at2v_gen_records_device")

    def gen_records_keys_device(self, cfg_seed: int, first: int, n: int, msg_len: int, d_keys: int, d_pk: int,
                                d_sig: int, d_msg: int, d_off: Optional[int], stream: int = 0) -> None:
        """GPU generator with a key per record: record i signed by seed index d_keys[i] (u64 device array)"""
        _check(self._lib.at2v_gen_records_keys_device(self._h, cfg_seed, first, n, msg_len, d_keys, d_pk, d_sig, d_msg,
                                                      d_off or None, stream or None), "at2v_gen_records_keys_device")

    def decode_points(self, pts: np.ndarray) -> np.ndarray:
        """bool[n]: 32-byte encodings that decode under dalek rules (GPU kernel)"""
        pts = np.ascontiguousarray(pts, dtype=np.uint8).reshape(-1, 32)
        n = len(pts)
        words = np.zeros(max(1, (n + 31) // 32), dtype=np.uint32)
        _check(self._lib.at2v_decode_points(self._h, _ptr(pts), n, _ptr(words)), "at2v_decode_points")
        return unpack_verdicts(words, n)

    def reject_reasons(self, pk: np.ndarray, sig: np.ndarray, verdict_words: np.ndarray) -> np.ndarray:
        """host arrays and the verdict words of a verify call over them (uint32, ceil(n/32); or bool[n] verdicts) ->
        u8[n] at2v_reason per record: 0 where the verdict bit is set, else the first failing check (REASON_*). The pass
        does not re-verify. A failed call raises; the library has then filled every byte with REASON_UNKNOWN."""
        pk, sig, n, words = _second_pass_args(pk, sig, verdict_words)
        reasons = np.full(max(1, n), REASON_UNKNOWN, np.uint8)
        _check(self._lib.at2v_reject_reasons(self._h, _ptr(pk), _ptr(sig), n, _ptr(words), _ptr(reasons)),
               "at2v_reject_reasons")
        return reasons[:n]

    def reject_reasons_device(self, d_pk: int, d_sig: int, n: int, d_verdicts: int, d_reasons: int,
                              stream: int = 0) -> None:
        """device pointers, asynchronous on `stream`: enqueue right after verify_batch_device on the same stream with
        its d_pk, d_sig and d_verdicts; d_reasons receives n bytes (16-byte aligned)"""
        _check(self._lib.at2v_reject_reasons_device(self._h, d_pk, d_sig, n, d_verdicts, d_reasons, stream or None),
               "at2v_reject_reasons_device")

    def policy_mask(self, pk: np.ndarray, sig: np.ndarray, verdict_words: np.ndarray) -> np.ndarray:
        """host arrays and the verdict words of a verify call over them by THIS verifier, which must have been created
        with policy="dalek-legacy" (uint32, ceil(n/32); or bool[n] verdicts) -> u8[n]: bit p set iff policy p accepts the
        record (MASK_*; 0, 4, 5 or 7). The pass does not re-verify. A failed call raises; the library has then filled
        every byte with 0 (a verifier of another policy is refused and nothing is written)."""
        pk, sig, n, words = _second_pass_args(pk, sig, verdict_words)
        mask = np.zeros(max(1, n), np.uint8)
        _check(self._lib.at2v_policy_mask(self._h, _ptr(pk), _ptr(sig), n, _ptr(words), _ptr(mask)), "at2v_policy_mask")
        return mask[:n]

    def policy_mask_device(self, d_pk: int, d_sig: int, n: int, d_verdicts: int, d_mask: int, stream: int = 0) -> None:
        """device pointers, asynchronous on `stream`: enqueue right after verify_batch_device on the same stream with
        its d_pk, d_sig and d_verdicts (policy="dalek-legacy" only); d_mask receives n bytes (16-byte aligned)"""
        _check(self._lib.at2v_policy_mask_device(self._h, d_pk, d_sig, n, d_verdicts, d_mask, stream or None),
               "at2v_policy_mask_device")

    def sign_batch(self, seeds: np.ndarray, msg: np.ndarray, msg_off: np.ndarray):
        seeds = np.ascontiguousarray(seeds, dtype=np.uint8)
        msg = np.ascontiguousarray(msg, dtype=np.uint8).reshape(-1)
        msg_off = np.ascontiguousarray(msg_off, dtype=np.uint32)
        n = len(msg_off) - 1
        pk = np.zeros((n, 32), np.uint8)
        sig = np.zeros((n, 64), np.uint8)
        msg_arg = msg if msg.size else np.zeros(1, np.uint8)
        _check(self._lib.at2v_sign_batch(self._h, _ptr(seeds), _ptr(msg_arg), _ptr(msg_off), n, _ptr(pk), _ptr(sig)),
               "at2v_sign_batch")
        return pk, sig


def comm_unique_id() -> bytes:
    """RCCL unique id for at2v_comm_init_rank (rank 0 creates it; hand it to the other ranks out of band)"""
    buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
    _check(load_library().at2v_comm_get_unique_id(buf), "at2v_comm_get_unique_id")
    return buf.raw


def verify_one(pk: bytes, sig: bytes, msg: bytes, policy="dalek") -> bool:
    """One signature on the CPU (at2v_verify_one: the product's verify code built for the host; no GPU)."""
    lib = load_library()
    if len(pk) != 32 or len(sig) != 64:
        raise ValueError("public key must be 32 bytes and signature 64 bytes")
    return bool(_check(lib.at2v_verify_one_policy(bytes(pk), bytes(sig), bytes(msg) if msg else None, len(msg),
                                                  _POLICIES[policy]), "at2v_verify_one_policy"))


def verify_one_reason(pk: bytes, sig: bytes, msg: bytes, policy="dalek") -> int:
    """One signature on the CPU -> its at2v_reason (REASON_VALID = 0 for a valid one; at2v_verify_one_reason)."""
    lib = load_library()
    if len(pk) != 32 or len(sig) != 64:
        raise ValueError("public key must be 32 bytes and signature 64 bytes")
    return _check(lib.at2v_verify_one_reason(bytes(pk), bytes(sig), bytes(msg) if msg else None, len(msg),
                                             _POLICIES[policy]), "at2v_verify_one_reason")


# ------------------------------------------------ drop::crypto::sign mirror
class PublicKey:
    """32-byte Ed25519 public key (drop::crypto::sign::PublicKey). Decoding is checked by verify."""

    def __init__(self, data: bytes):
        if len(data) != 32:
            raise ValueError("public key must be 32 bytes")
        self.bytes = bytes(data)

    def __bytes__(self):
        return self.bytes

    def __eq__(self, other):
        return isinstance(other, PublicKey) and other.bytes == self.bytes

    def __hash__(self):
        return hash(self.bytes)

    def __repr__(self):
        return f"PublicKey({self.bytes.hex()})"


class Signature:
    """64-byte Ed25519 signature R || S (drop::crypto::sign::Signature)."""

    def __init__(self, data: bytes):
        if len(data) != 64:
            raise ValueError("signature must be 64 bytes")
        self.bytes = bytes(data)

    def verify(self, message: bytes, public_key: PublicKey) -> None:
        """Raise VerifyError unless the signature is valid (at2v_verify_one: the per-signature CPU entry point,
        as drop's synchronous verify is; batches go through BatchVerifier on the GPU)."""
        reason = verify_one_reason(public_key.bytes, self.bytes, bytes(message))
        if reason != REASON_VALID:
            raise VerifyError(f"signature verification failed: {reason_name(reason)}", reason)
