#!/usr/bin/env python3
"""The Hamming scans against the byte-EUCLIDEAN scan of an identically shaped view: same run, interleaved rounds.

  python tools/bench_hamming.py [--rows-per-shard N] [--bytes 96,16] [--rounds R] [--iters I] [--out FILE]

Per shape (8 shards × N rows of `bytes` bytes, DIST_INT8 synthetic: uniform random bits) it stages an
OSK_BYTE / OSK_HAMMING view and an OSK_BYTE / OSK_EUCLIDEAN view and measures round-robin, kernel time from the
scan launch's own stamps (osk_view_profile / osk_view_scan_time) and stream time around the calls:
  * ham_1q        one query, k = 10, on scan_ham_stream;
  * ham_1q_batch  the same query on scan_ham<·,·,1> (tune ham_stream = 0): the batch kernel's loop at NQ = 1;
  * ham_8q        8 queries, k = 10, on scan_ham<·,·,8> (one launch);
  * ham_k1000     one query, k = 1000: the select path (kernel time = its writer sel_keys_ham; the call adds the
                  radix select and the sort);
  * byte_1q       the yardstick: one query, k = 10, scan_i8_stream over the byte-EUCLIDEAN view.
Bytes per scan: rows × units × 16 (+ 4 B per row for the byte scan's norms; + 8 B per row of keys the select
writer stores).  The bar: ham_1q's median kernel time ≤ byte_1q's + the spread between rounds (the larger of the
two variants' max − min).  Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opensearch_amd import _lib  # noqa: E402
from opensearch_amd.lucene import synth_host  # noqa: E402

L = _lib.lib()
NSH = 8


def make_view(n, dim, sim):
    segs = []
    for s in range(NSH):
        h = C.c_void_p()
        _lib.check(L.osk_seg_synth(0, n, dim, _lib.BYTE, sim, 42, _lib.DIST_INT8, s * n, C.byref(h)))
        segs.append(h.value)
    arr = (C.c_void_p * NSH)(*segs)
    seg_shard = np.arange(NSH, dtype=np.int32)
    view = C.c_void_p()
    _lib.check(L.osk_view_create(arr, NSH, seg_shard.ctypes.data, None, NSH, None, C.byref(view)))
    foot = 0
    for h in segs:
        b = C.c_int64()
        _lib.check(L.osk_seg_footprint(C.c_void_p(h), C.byref(b)))
        foot += b.value
    return view, segs, foot


def bench_shape(n, dim, rounds, iters, stream):
    units = (dim + 15) // 16
    ham, ham_segs, ham_foot = make_view(n, dim, _lib.OSK_HAMMING)
    byt, byt_segs, byt_foot = make_view(n, dim, _lib.EUCLIDEAN)
    q = torch.from_numpy(synth_host(0, 8, dim, 43, _lib.DIST_INT8)).cuda()
    keys = torch.empty((8, NSH, 1000), dtype=torch.int64, device="cuda")
    kcnt = torch.empty((8, NSH), dtype=torch.int32, device="cuda")

    def call(view, nq, k):
        return lambda: _lib.check(L.osk_view_search_device(view, q.data_ptr(), nq, k, None, keys.data_ptr(),
                                                           kcnt.data_ptr(), None, stream))

    def timed(view, knobs, fn):
        for key, value in knobs.items():
            _lib.tune(key, value)
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        _lib.check(L.osk_view_profile(view, 1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms, calls = C.c_double(), C.c_int64()
        _lib.check(L.osk_view_scan_time(view, C.byref(ms), C.byref(calls)))
        _lib.check(L.osk_view_profile(view, 0))
        return ms.value / max(1, calls.value), e0.elapsed_time(e1) / iters

    ON, OFF = {"ham_stream": 1, "i8_stream": 1}, {"ham_stream": 0, "i8_stream": 1}
    variants = {
        "ham_1q": (ham, ON, call(ham, 1, 10)),
        "byte_1q": (byt, ON, call(byt, 1, 10)),
        "ham_1q_batch": (ham, OFF, call(ham, 1, 10)),
        "ham_8q": (ham, ON, call(ham, 8, 10)),
        "ham_k1000": (ham, ON, call(ham, 1, 1000)),
    }
    res = {name: [] for name in variants}
    for r in range(rounds):
        for name, (view, knobs, fn) in variants.items():
            res[name].append(timed(view, knobs, fn))
        print(f"{dim} B round {r} done", file=sys.stderr, flush=True)
    _lib.tune("ham_stream", 1)

    rows = NSH * n
    scan_bytes = {"ham_1q": rows * units * 16, "ham_1q_batch": rows * units * 16, "ham_8q": rows * units * 16,
                  "ham_k1000": rows * (units * 16 + 8), "byte_1q": rows * (units * 16 + 4)}
    out = {"shape": f"{NSH} shards x {n} x {dim} bytes ({8 * dim} bits)", "rows": rows, "units": units,
           "hamming_footprint_bytes": ham_foot, "byte_euclidean_footprint_bytes": byt_foot}
    for name, xs in res.items():
        kern = [x[0] for x in xs]
        med = statistics.median(kern)
        out[name] = {"kernel_ms": round(med, 5), "kernel_ms_min": round(min(kern), 5), "kernel_ms_max": round(max(kern), 5),
                     "call_stream_ms": round(statistics.median(x[1] for x in xs), 5), "bytes": scan_bytes[name],
                     "GBps": round(scan_bytes[name] / 1e9 / (med * 1e-3), 1)}
    spread = max(out["ham_1q"]["kernel_ms_max"] - out["ham_1q"]["kernel_ms_min"],
                 out["byte_1q"]["kernel_ms_max"] - out["byte_1q"]["kernel_ms_min"])
    out["round_spread_ms"] = round(spread, 5)
    out["ham_1q_over_byte_1q"] = round(out["ham_1q"]["kernel_ms"] / out["byte_1q"]["kernel_ms"], 4)
    out["meets_yardstick"] = bool(out["ham_1q"]["kernel_ms"] <= out["byte_1q"]["kernel_ms"] + spread)
    out["per_round_kernel_ms"] = {k_: [round(x[0], 5) for x in v] for k_, v in res.items()}

    _lib.check(L.osk_view_release(ham))
    _lib.check(L.osk_view_release(byt))
    for h in ham_segs + byt_segs:
        _lib.check(L.osk_seg_release(C.c_void_p(h)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-per-shard", type=int, default=1_250_000)
    ap.add_argument("--bytes", default="96,16", help="bytes per vector, one shape each")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.cuda.set_stream(torch.cuda.Stream())   # non-null: 0 would mean the library's own stream
    stream = torch.cuda.current_stream().cuda_stream
    out = {"rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "shapes": [bench_shape(a.rows_per_shard, int(b), a.rounds, a.iters, stream) for b in a.bytes.split(",")]}
    out["meets_yardstick"] = all(s["meets_yardstick"] for s in out["shapes"])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
