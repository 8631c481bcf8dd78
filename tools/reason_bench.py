#!/usr/bin/env python3
"""Cost of the reject-reasons pass beside the verify launch it follows (DESIGN.md "Reject reasons").

Device buffers, one process, one stream: for a batch of n records (default 1,048,576) it times, with device events,
  * the verify launch (at2v_verify_batch_device, the throughput kernel: n is above small_batch_max), and
  * the reasons pass (at2v_reject_reasons_device) over the verdict words that launch wrote,
alternating the two for `--reps` repetitions after `--warmup` untimed ones, on two inputs generated before any timed
region: the config-4 adversarial mix (oracle_gen_adversarial, ~10 % rejected, spread over the batch) and an all-valid
batch (the GPU generator). Prints the median and the spread of each and the ratio pass / verify as one JSON line.
Needs a gfx950 device; there is no CPU path."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "at2-node_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def timed(fn, ev):
    import torch
    a, b = ev
    a.record(torch.cuda.current_stream())
    fn()
    b.record(torch.cuda.current_stream())
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--msg-len", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()

    import torch

    import at2v
    import oracle_py

    if not torch.cuda.is_available():
        sys.exit("reason_bench needs a GPU")
    torch.cuda.set_device(0)
    dev, n, L = "cuda:0", args.n, args.msg_len
    s = torch.cuda.current_stream().cuda_stream
    v = at2v.BatchVerifier(device=0)
    out = {"n": n, "msg_len": L, "reps": args.reps, "info": {k: v.info()[k] for k in ("vgprs", "waves_per_cu", "cus")}}

    def device_batch(pk, sig, msg):
        return (torch.from_numpy(pk.reshape(-1)).to(dev), torch.from_numpy(sig.reshape(-1)).to(dev),
                torch.from_numpy(np.concatenate([msg, np.zeros(16, np.uint8)])).to(dev))

    pk, sig, msg, _, _ = oracle_py.Oracle().gen_adversarial(0x4154325F, 0, n, L, threads=min(16, os.cpu_count() or 1))
    batches = {"config4_mix": device_batch(pk, sig, msg)}
    d_pk = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_sig = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    d_msg = torch.zeros(n * L + 16, dtype=torch.uint8, device=dev)
    v.gen_records_device(0x4154325F, 0, n, L, d_pk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), None, s)
    batches["all_valid"] = (d_pk, d_sig, d_msg)
    d_off = (torch.arange(n + 1, dtype=torch.int64, device=dev) * L).to(torch.int32)
    d_ver = torch.zeros((n + 31) // 32, dtype=torch.int32, device=dev)
    d_rea = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

    for name, (b_pk, b_sig, b_msg) in batches.items():
        def verify():
            v.verify_batch_device(b_pk.data_ptr(), b_sig.data_ptr(), b_msg.data_ptr(), n * L, d_off.data_ptr(), n,
                                  d_ver.data_ptr(), s)

        def reasons():
            v.reject_reasons_device(b_pk.data_ptr(), b_sig.data_ptr(), n, d_ver.data_ptr(), d_rea.data_ptr(), s)

        tv, tr = [], []
        for k in range(args.warmup + args.reps):
            a, b = timed(verify, ev), timed(reasons, ev)
            if k >= args.warmup:
                tv.append(a)
                tr.append(b)
        rea = d_rea.cpu().numpy()
        rejected = int(n - np.unpackbits(d_ver.cpu().numpy().view(np.uint8)).sum())
        assert int((rea != 0).sum()) == rejected
        sv, sr = stats(tv), stats(tr)
        out[name] = {"rejected": rejected, "reasons": {int(k): int(c) for k, c in zip(*np.unique(rea, return_counts=True))},
                     "verify": sv, "reasons_pass": sr, "ratio": round(sr["median_ms"] / sv["median_ms"], 4)}
    v.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
