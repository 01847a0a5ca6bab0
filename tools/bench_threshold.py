#!/usr/bin/env python3
"""Similarity-threshold search against the fp32 streaming scan, same view, same run, interleaved.

  python tools/bench_threshold.py [--rows-per-shard N] [--rounds R] [--iters I] [--out FILE]

Stages the C3 shape (8 shards × 1.25M × 768 fp32 COSINE, synthetic as bench.py builds it) and, for one query,
measures round-robin:
  * scan_f32      the k-NN streaming scan's kernel time (prefilter off — bench.py's `fp32_stream`
                  configuration: tune sq8 = 0, k = 10), osk_view_profile / osk_view_scan_time;
  * thr_scan_f32  the threshold scan's kernel time the same way, min_score = the query's 100th best score;
  * the whole threshold call on its stream (events around it): query prep + mask clear + thr_scan +
    thr_offsets + thr_emit; call − scan bounds thr_offsets + thr_emit from above;
  * the same at min_score = −inf with cap = rows per shard: every row a hit, the worst case for the emit;
  * the same at min_score = the median score of the view: the worst case for the int8 first pass;
  * each threshold variant again with the certified int8 first pass (tune thr_sq8 = 1, sq8 = 1: thr_scan_sq8's
    kernel time from the same stamps; the call adds thr_settle_f32) and the rows its settle re-scored per call
    (counter threshold_sq8_settled_rows).  The int8 pass reads 784 B per 768-dim row against 3072 B.
Both fp32 scans read the same corpus bytes; the threshold scan adds the mask words it stores.  Prints one JSON line.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-per-shard", type=int, default=1_250_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rank", type=int, default=100, help="min_score = the query's rank-th best score")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dim, nsh, n = a.dim, 8, a.rows_per_shard
    _lib.tune("sq8", 0)   # fp32_stream: no prefilter copies, every k-NN search on the fp32 scan / select path
    segs = []
    for s in range(nsh):
        h = C.c_void_p()
        _lib.check(L.osk_seg_synth(0, n, dim, _lib.FLOAT32, _lib.COSINE, 42, _lib.DIST_NORMALISH_UNIT, s * n, C.byref(h)))
        segs.append(h.value)
    arr = (C.c_void_p * nsh)(*segs)
    seg_shard = np.arange(nsh, dtype=np.int32)
    view = C.c_void_p()
    _lib.check(L.osk_view_create(arr, nsh, seg_shard.ctypes.data, None, nsh, None, C.byref(view)))
    q_host = synth_host(0, 1, dim, 43, _lib.DIST_NORMALISH_UNIT)

    # the threshold: the query's rank-th best score over the whole view (exact k-NN, host entry)
    k = a.rank
    sc, dc, sh = np.empty((1, k), np.float32), np.empty((1, k), np.int32), np.empty((1, k), np.int32)
    cnt, tot, mx = np.empty(1, np.int32), np.empty(1, np.int64), np.empty(1, np.float32)
    _lib.check(L.osk_view_search(view, q_host.ctypes.data, 1, k, 0, k, None, sc.ctypes.data, dc.ctypes.data,
                                 sh.ctypes.data, cnt.ctypes.data, tot.ctypes.data, mx.ctypes.data))
    min_score = float(sc[0, cnt[0] - 1])

    q = torch.from_numpy(q_host).cuda()
    keys = torch.empty((1, nsh, 10), dtype=torch.int64, device="cuda")
    kcnt = torch.empty((1, nsh), dtype=torch.int32, device="cuda")
    cap_small, cap_all = 1024, n
    docs = torch.empty((1, nsh, cap_all), dtype=torch.int32, device="cuda")
    scores = torch.empty((1, nsh, cap_all), dtype=torch.float32, device="cuda")
    tcnt = torch.empty((1, nsh), dtype=torch.int32, device="cuda")
    ttot = torch.empty((1, nsh), dtype=torch.int64, device="cuda")
    ms_sel = torch.tensor([min_score], dtype=torch.float32, device="cuda")
    ms_all = torch.tensor([float("-inf")], dtype=torch.float32, device="cuda")
    ms_med = torch.zeros(1, dtype=torch.float32, device="cuda")   # (filled below: the view's median score)
    torch.cuda.set_stream(torch.cuda.Stream())   # non-null: 0 would mean the library's own stream
    stream = torch.cuda.current_stream().cuda_stream

    def knn():
        _lib.check(L.osk_view_search_device(view, q.data_ptr(), 1, 10, None, keys.data_ptr(), kcnt.data_ptr(), None, stream))

    def thr(ms, cap):
        _lib.check(L.osk_view_search_threshold_device(view, q.data_ptr(), 1, ms.data_ptr(), None, cap, docs.data_ptr(),
                                                      scores.data_ptr(), tcnt.data_ptr(), ttot.data_ptr(), None, stream))

    def counter(name):
        v = C.c_int64()
        _lib.check(L.osk_view_counter(view, name.encode(), C.byref(v)))
        return v.value

    def timed(knobs, fn):
        """(kernel ms per call from the scan launches' own stamps, stream ms per call around the calls)."""
        for key, value in knobs.items():
            _lib.tune(key, value)
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        _lib.check(L.osk_view_profile(view, 1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms, calls = C.c_double(), C.c_int64()
        _lib.check(L.osk_view_scan_time(view, C.byref(ms), C.byref(calls)))
        _lib.check(L.osk_view_profile(view, 0))
        return ms.value / max(1, calls.value), e0.elapsed_time(e1) / a.iters

    # every row's score (min_score = −inf, cap = a shard's rows) → the view's median score
    thr(ms_all, cap_all)
    torch.cuda.synchronize()
    hits_all = int(ttot.sum().item())
    ms_med.copy_(scores.flatten().median())
    torch.cuda.synchronize()

    FP32, SQ8 = {"sq8": 0, "thr_sq8": 0}, {"sq8": 1, "thr_sq8": 1}
    thr_fns = {"thr_selective": lambda: thr(ms_sel, cap_small), "thr_all_rows": lambda: thr(ms_all, cap_all),
               "thr_median": lambda: thr(ms_med, cap_small)}
    variants = {"scan_f32": (FP32, knn)}
    for name, fn in thr_fns.items():
        variants[name] = (FP32, fn)
        variants[name + "_sq8"] = (SQ8, fn)
    res = {name: [] for name in variants}
    for r in range(a.rounds):
        for name, (knobs, fn) in variants.items():
            res[name].append(timed(knobs, fn))
        print(f"round {r} done", file=sys.stderr, flush=True)

    # hits, and the rows one call's settle re-scores, per variant (both paths must count the same hits)
    hits, settled = {}, {}
    for name, fn in thr_fns.items():
        for knobs, tag in ((FP32, ""), (SQ8, "_sq8")):
            for key, value in knobs.items():
                _lib.tune(key, value)
            s0, c0 = counter("threshold_sq8_settled_rows"), counter("threshold_sq8_calls")
            fn()
            torch.cuda.synchronize()
            hits[name + tag] = int(ttot.sum().item())
            settled[name + tag] = counter("threshold_sq8_settled_rows") - s0
            assert counter("threshold_sq8_calls") - c0 == (1 if tag else 0), name + tag
        assert hits[name] == hits[name + "_sq8"], (name, hits)
    hits_sel = hits["thr_selective"]
    assert hits["thr_all_rows"] == hits_all

    def med(name, i):
        return statistics.median(x[i] for x in res[name])

    corpus_gb = nsh * n * dim * 4 / 1e9
    out = {
        "shape": f"{nsh} shards x {n} x {dim} fp32 COSINE, 1 query", "corpus_GB": corpus_gb,
        "rounds": a.rounds, "iters": a.iters, "min_score": min_score, "rank": a.rank,
        "hits_selective": hits_sel, "hits_all_rows": hits_all,
        "scan_f32_kernel_ms": med("scan_f32", 0), "scan_f32_GBps": corpus_gb / (med("scan_f32", 0) * 1e-3),
        "knn_call_stream_ms": med("scan_f32", 1),
        "thr_scan_kernel_ms": med("thr_selective", 0), "thr_scan_GBps": corpus_gb / (med("thr_selective", 0) * 1e-3),
        "thr_scan_over_scan_f32": med("thr_selective", 0) / med("scan_f32", 0),
        "thr_call_stream_ms": med("thr_selective", 1),
        "thr_rest_ms_upper_bound": med("thr_selective", 1) - med("thr_selective", 0),
        "all_rows_scan_kernel_ms": med("thr_all_rows", 0), "all_rows_call_stream_ms": med("thr_all_rows", 1),
        "all_rows_rest_ms_upper_bound": med("thr_all_rows", 1) - med("thr_all_rows", 0),
        "all_rows_cap_per_shard": cap_all,
        "median_score": float(ms_med.item()), "hits_median": hits["thr_median"],
        "median_scan_kernel_ms": med("thr_median", 0), "median_call_stream_ms": med("thr_median", 1),
        # the certified int8 first pass (thr_sq8 = 1), same rounds
        "sq8_corpus_GB": nsh * n * (16 * ((dim + 15) // 16) + 16) / 1e9,
        "sq8_thr_scan_kernel_ms": med("thr_selective_sq8", 0),
        "sq8_thr_scan_GBps": nsh * n * (16 * ((dim + 15) // 16) + 16) / 1e9 / (med("thr_selective_sq8", 0) * 1e-3),
        "sq8_thr_call_stream_ms": med("thr_selective_sq8", 1),
        "sq8_scan_kernel_speedup": med("thr_selective", 0) / med("thr_selective_sq8", 0),
        "sq8_call_speedup": med("thr_selective", 1) / med("thr_selective_sq8", 1),
        "thr_call_stream_ms_spread": [min(x[1] for x in res["thr_selective"]), max(x[1] for x in res["thr_selective"])],
        "sq8_thr_call_stream_ms_spread": [min(x[1] for x in res["thr_selective_sq8"]),
                                          max(x[1] for x in res["thr_selective_sq8"])],
        "sq8_settled_rows_selective": settled["thr_selective_sq8"],
        "sq8_all_rows_scan_kernel_ms": med("thr_all_rows_sq8", 0), "sq8_all_rows_call_stream_ms": med("thr_all_rows_sq8", 1),
        "sq8_settled_rows_all_rows": settled["thr_all_rows_sq8"],
        "sq8_median_scan_kernel_ms": med("thr_median_sq8", 0), "sq8_median_call_stream_ms": med("thr_median_sq8", 1),
        "sq8_settled_rows_median": settled["thr_median_sq8"],
        "sq8_settled_share_median": settled["thr_median_sq8"] / (nsh * n),
        "per_round": {k_: [[round(x, 4) for x in p] for p in v] for k_, v in res.items()},
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    _lib.tune("sq8", 1)
    _lib.tune("thr_sq8", 1)


if __name__ == "__main__":
    main()
