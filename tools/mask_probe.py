#!/usr/bin/env python3
"""The policy-mask pass beside the verify launch it follows: device buffers, one stream, a context of
AT2V_POLICY_DALEK_V1_LEGACY. Generates n valid records (default 1,048,576, 100-byte messages), adds l to the scalar of
every 16th so that all three mask values of accepted records occur, then runs `--reps` times the verify launch, the mask
pass and the reasons pass. Meant for `rocprofv3 --kernel-trace --stats -- python3 tools/mask_probe.py` (the per-kernel
durations); on its own it prints device-event medians as one JSON line. Needs a gfx950 device."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "at2-node_amd"))
L = 2 ** 252 + 27742317777372353535851937790883648493


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--msg-len", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    import at2v

    torch.cuda.set_device(0)
    dev, n, ml = "cuda:0", a.n, a.msg_len
    s = torch.cuda.current_stream().cuda_stream
    v = at2v.BatchVerifier(device=0, policy="dalek-legacy")
    d_pk = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_sig = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    d_msg = torch.zeros(n * ml + 16, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    v.gen_records_device(0x4154325F, 0, n, ml, d_pk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), d_off.data_ptr(), s)
    torch.cuda.synchronize()
    sig = d_sig.cpu().numpy().reshape(n, 64)
    shifted = 0
    for i in range(0, n, 16):
        t = int.from_bytes(sig[i, 32:].tobytes(), "little") + L
        if t < 2 ** 253:
            sig[i, 32:] = np.frombuffer(t.to_bytes(32, "little"), np.uint8)
            shifted += 1
    d_sig.copy_(torch.from_numpy(sig.reshape(-1)))
    d_ver = torch.zeros((n + 31) // 32, dtype=torch.int32, device=dev)
    d_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_rea = torch.zeros(n, dtype=torch.uint8, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ms = {"verify": [], "mask": [], "reasons": []}
    for _ in range(a.reps + 1):
        ev[0].record()
        v.verify_batch_device(d_pk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), n * ml, d_off.data_ptr(), n,
                              d_ver.data_ptr(), s)
        ev[1].record()
        v.policy_mask_device(d_pk.data_ptr(), d_sig.data_ptr(), n, d_ver.data_ptr(), d_mask.data_ptr(), s)
        ev[2].record()
        v.reject_reasons_device(d_pk.data_ptr(), d_sig.data_ptr(), n, d_ver.data_ptr(), d_rea.data_ptr(), s)
        ev[3].record()
        torch.cuda.synchronize()
        for k, name in enumerate(ms):
            ms[name].append(ev[k].elapsed_time(ev[k + 1]))
    mask = d_mask.cpu().numpy()
    counts = {int(k): int(c) for k, c in zip(*np.unique(mask, return_counts=True))}
    assert counts == {4: shifted, 7: n - shifted}, counts
    assert not d_rea.cpu().numpy().any()
    v.close()
    print(json.dumps({"n": n, "mask_counts": counts,
                      **{k: {"median_ms": round(float(np.median(t[1:])), 4), "min_ms": round(min(t[1:]), 4),
                             "max_ms": round(max(t[1:]), 4)} for k, t in ms.items()}}))


if __name__ == "__main__":
    main()
