#!/usr/bin/env python3
"""What the transfers entry points cost beside the records path, interleaved rounds in ONE process.

usage: python3 tools/transfers_probe.py [--n 1048576] [--rounds 7] [--host-rounds 5] [--only device|host]

n AT2 transfers with 48-byte messages u64le(32) || recipient || u64le(amount), signed on the GPU (at2v_sign_batch), so
every record is valid on both paths. Two contexts: distinct sender keys on a plain context (verify_kernel), and 64
repeating senders on a context with sender combs, warmed first.
  baseline   at2v_verify_batch_device over the pre-expanded messages and offsets (what a node had to build before)
  transfers  at2v_verify_transfers_device over the fields of the same records, without d_recipient_ok
  +decode    the same with d_recipient_ok
Each round times one launch of each, in turn, between two events on the launch stream; the medians, the baseline's
run-to-run spread (max - min over the rounds) and the three ratios are printed as one JSON line per context. The prep
kernel's own time is not visible from outside a launch: take it from a kernel trace of this tool, in a run of its own
(rocprofv3 --kernel-trace --stats -- python3 tools/transfers_probe.py --only device --rounds 3).
--only host: at2v_verify_transfers from pinned fields against at2v_verify_batch from pinned records, both as n-record
calls from at2v_host_alloc memory, wall clock per call."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "at2-node_amd"))
import at2v  # noqa: E402

L = 48


def make_transfers(v, n, senders, rng):
    """(sender, sig, recipient, amount, msg, off): n valid transfers signed under `senders` repeating keys (0: distinct)"""
    k = senders or n
    seeds = rng.integers(0, 256, (k, 32), dtype=np.uint8)
    seeds = seeds[np.arange(n) % k]
    # recipients: valid keys (the public keys of some of the seeds), amounts over the whole u64 range
    m = min(n, 4096)
    pool, _ = v.sign_batch(seeds[:m], np.zeros(1, np.uint8), np.zeros(m + 1, np.uint32))
    recipient = np.ascontiguousarray(pool[rng.integers(0, len(pool), n)])
    amount = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    msg = np.empty((n, L), np.uint8)
    msg[:, :8] = np.frombuffer((32).to_bytes(8, "little"), np.uint8)
    msg[:, 8:40] = recipient
    msg[:, 40:] = amount.astype("<u8").view(np.uint8).reshape(n, 8)
    off = (np.arange(n + 1, dtype=np.uint64) * L).astype(np.uint32)
    sender, sig = v.sign_batch(seeds, msg.reshape(-1), off)
    return sender, sig, recipient, amount, msg.reshape(-1), off


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")


def device_rounds(v, rec, rounds, label):
    sender, sig, recipient, amount, msg, off = rec
    n = len(amount)
    words = (n + 31) // 32
    d_sender, d_sig, d_recipient, d_amount, d_msg, d_off = (to_dev(a) for a in (sender, sig, recipient, amount, msg, off))
    d_msg = torch.cat([d_msg, torch.zeros(16, dtype=torch.uint8, device="cuda:0")])
    ws = at2v.BatchVerifier.transfers_workspace_bytes(n, at2v.WIRE_BYTES)
    d_work = torch.empty(ws, dtype=torch.uint8, device="cuda:0")
    d_ver = [torch.zeros(words, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    d_rok = torch.zeros(words, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    runs = {
        "baseline": lambda: v.verify_batch_device(d_sender.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), n * L,
                                                  d_off.data_ptr(), n, d_ver[0].data_ptr(), s),
        "transfers": lambda: v.verify_transfers_device(d_sender.data_ptr(), d_sig.data_ptr(), d_recipient.data_ptr(),
                                                       d_amount.data_ptr(), n, at2v.WIRE_BYTES, d_work.data_ptr(), ws,
                                                       d_ver[1].data_ptr(), 0, s),
        "transfers_decode": lambda: v.verify_transfers_device(d_sender.data_ptr(), d_sig.data_ptr(),
                                                              d_recipient.data_ptr(), d_amount.data_ptr(), n,
                                                              at2v.WIRE_BYTES, d_work.data_ptr(), ws,
                                                              d_ver[2].data_ptr(), d_rok.data_ptr(), s),
    }
    for _ in range(2):  # warm-up: code objects, and the sender cache learns its keys
        for f in runs.values():
            f()
        torch.cuda.synchronize()
        v.info()  # (waits for the cache builds)
    ms = {k: [] for k in runs}
    for _ in range(rounds):
        for k, f in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    for d in d_ver:
        assert at2v.unpack_verdicts(d.cpu().numpy().view(np.uint32), n).all(), "a record was rejected"
    assert at2v.unpack_verdicts(d_rok.cpu().numpy().view(np.uint32), n).all()
    med = {k: statistics.median(x) for k, x in ms.items()}
    out = {"probe": "device", "context": label, "n": n, "rounds": rounds,
           "ms": {k: round(x, 4) for k, x in med.items()},
           "baseline_spread_ms": round(max(ms["baseline"]) - min(ms["baseline"]), 4),
           "ratio_transfers": round(med["transfers"] / med["baseline"], 5),
           "ratio_transfers_decode": round(med["transfers_decode"] / med["baseline"], 5),
           "ratio_decode_over_transfers": round(med["transfers_decode"] / med["transfers"], 5),
           "info": {k: v.info()[k] for k in ("cache_entries", "cache_record_hits")}}
    print(json.dumps(out), flush=True)


def host_rounds(v, rec, rounds):
    sender, sig, recipient, amount, msg, off = rec
    n = len(amount)
    words = (n + 31) // 32

    def pinned(a):
        a = np.ascontiguousarray(a)
        p = v.host_alloc(max(a.nbytes, 1)).view(a.dtype)[:a.size].reshape(a.shape)
        p[...] = a
        return p

    p_sender, p_sig, p_recipient, p_amount, p_msg, p_off = (pinned(a) for a in rec)
    w = [v.host_alloc(words * 4).view(np.uint32) for _ in range(2)]
    runs = {
        "records": lambda: v.verify_batch(p_sender, p_sig, p_msg, p_off, words=w[0]),
        "transfers": lambda: v.verify_transfers(p_sender, p_sig, p_recipient, p_amount, words=w[1]),
    }
    for f in runs.values():
        assert f().all()
    ms = {k: [] for k in runs}
    i0 = v.info()
    for _ in range(rounds):
        for k, f in runs.items():
            t0 = time.perf_counter()
            f()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    i1 = v.info()
    med = {k: statistics.median(x) for k, x in ms.items()}
    print(json.dumps({"probe": "host", "n": n, "rounds": rounds, "ms": {k: round(x, 4) for k, x in med.items()},
                      "records_spread_ms": round(max(ms["records"]) - min(ms["records"]), 4),
                      "ratio_transfers": round(med["transfers"] / med["records"], 5),
                      "direct_bytes": i1["host_direct_bytes"] - i0["host_direct_bytes"],
                      "staged_bytes": i1["host_staged_bytes"] - i0["host_staged_bytes"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=5)
    ap.add_argument("--only", choices=["device", "host"])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0x7A5F)
    with at2v.BatchVerifier() as v:
        distinct = make_transfers(v, a.n, 0, rng)
        if a.only != "host":
            device_rounds(v, distinct, a.rounds, "plain context, distinct keys")
        if a.only != "device":
            host_rounds(v, distinct, a.host_rounds)
    if a.only != "host":
        with at2v.BatchVerifier(sender_cache=1024, sender_comb=True) as v:
            device_rounds(v, make_transfers(v, a.n, 64, rng), a.rounds, "sender combs, 64 repeating senders")


if __name__ == "__main__":
    main()
