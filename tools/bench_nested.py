#!/usr/bin/env python3
"""Nested k-NN — the fp32 scan and the certified int8 first pass — against the k-NN and threshold scans, same
view, same run, interleaved.

  python tools/bench_nested.py [--rows-per-shard N] [--families 1,8,64] [--rounds R] [--iters I] [--out FILE]

Stages the C3 shape (8 shards × 1.25M × 768 fp32 COSINE, synthetic as bench.py builds it; dense: every doc has a
vector) once per family size f — docs f−1, 2f−1, … and the last doc are the parents, so a family is f consecutive
rows — and, for one query at k = 10, measures round-robin:
  * scan_f32       the k-NN streaming scan's kernel time (prefilter off — bench.py's `fp32_stream` configuration:
                   tune sq8 = 0), osk_view_profile / osk_view_scan_time;
  * nest_scan_f32  the nested scan's kernel time the same way: the same rows plus 4 B per row of the row→parent
                   table, plus one 64-bit atomic max per run of equal parents in a walk step;
  * the whole nested call on its stream (events around it): query prep + clear of the best-child keys + nest_scan +
    nest_topk + merge_shards; call − scan bounds the clear + nest_topk + merge from above;
  * nest_scan_sq8  the same call with tune nest_sq8 = 1 (the fp32 side runs with nest_sq8 = 0): the int8 pass's kernel
                   time, the whole call (prep, clears, nest_scan_sq8, the floor's nest_topk + merge_shards,
                   nest_settle_f32, nest_topk, merge_shards) and the rows the settle re-scored per call;
  * thr_scan_sq8   the threshold search's int8 pass on the same view (min_score 0.99: next to nothing to settle or
                   emit): the same loop without the parent fold, so nest_scan_sq8 / thr_scan_sq8 is what the fold
                   costs.
The knobs are switched per variant inside each round, so the variants alternate in one process.  Prints one JSON
line.
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
from opensearch_amd.lucene import bits_from_bool, synth_host  # noqa: E402

L = _lib.lib()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-per-shard", type=int, default=1_250_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--families", default="1,8,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dim, nsh, n, k = a.dim, 8, a.rows_per_shard, 10
    q_host = synth_host(0, 1, dim, 43, _lib.DIST_NORMALISH_UNIT)
    q = torch.from_numpy(q_host).cuda()
    keys = torch.empty((1, nsh, k), dtype=torch.int64, device="cuda")
    kcnt = torch.empty((1, nsh), dtype=torch.int32, device="cuda")
    cap = 64
    tmin = torch.full((1,), 0.99, dtype=torch.float32, device="cuda")
    tdocs = torch.empty((1, nsh, cap), dtype=torch.int32, device="cuda")
    tscores = torch.empty((1, nsh, cap), dtype=torch.float32, device="cuda")
    tcount = torch.empty((1, nsh), dtype=torch.int32, device="cuda")
    ttotal = torch.empty((1, nsh), dtype=torch.int64, device="cuda")
    torch.cuda.set_stream(torch.cuda.Stream())   # non-null: 0 would mean the library's own stream
    stream = torch.cuda.current_stream().cuda_stream
    corpus_gb = nsh * n * dim * 4 / 1e9
    out = {"shape": f"{nsh} shards x {n} x {dim} fp32 COSINE, 1 query, k = {k}", "corpus_GB": corpus_gb,
           "rounds": a.rounds, "iters": a.iters, "families": {}}

    for fam in [int(x) for x in a.families.split(",")]:
        mask = np.arange(n) % fam == fam - 1
        mask[-1] = True
        bits = bits_from_bool(mask)
        segs = []
        for s in range(nsh):
            h = C.c_void_p()
            _lib.check(L.osk_seg_synth(0, n, dim, _lib.FLOAT32, _lib.COSINE, 42, _lib.DIST_NORMALISH_UNIT, s * n, C.byref(h)))
            _lib.check(L.osk_seg_set_parents(h, bits.ctypes.data))
            segs.append(h)
        arr = (C.c_void_p * nsh)(*[h.value for h in segs])
        seg_shard = np.arange(nsh, dtype=np.int32)
        view = C.c_void_p()
        _lib.check(L.osk_view_create(arr, nsh, seg_shard.ctypes.data, None, nsh, None, C.byref(view)))
        _lib.check(L.osk_view_warm(view, 0))      # the nested search's view tables

        def knn():
            _lib.check(L.osk_view_search_device(view, q.data_ptr(), 1, k, None, keys.data_ptr(), kcnt.data_ptr(), None, stream))

        def nested():
            _lib.check(L.osk_view_search_nested_device(view, q.data_ptr(), 1, k, None, keys.data_ptr(), kcnt.data_ptr(),
                                                       None, stream))

        def threshold():
            _lib.check(L.osk_view_search_threshold_device(view, q.data_ptr(), 1, tmin.data_ptr(), None, cap, tdocs.data_ptr(),
                                                          tscores.data_ptr(), tcount.data_ptr(), ttotal.data_ptr(), None,
                                                          stream))

        def counter(name):
            v = C.c_int64()
            _lib.check(L.osk_view_counter(view, name.encode(), C.byref(v)))
            return v.value

        def timed(fn, knobs):
            """(kernel ms per call from the scan launches' own stamps, stream ms per call around the calls, rows the
            nested settle re-scored per call)."""
            for key, value in knobs.items():
                _lib.tune(key, value)
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            _lib.check(L.osk_view_profile(view, 1))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0 = counter("nested_sq8_settled_rows")
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms, calls = C.c_double(), C.c_int64()
            _lib.check(L.osk_view_scan_time(view, C.byref(ms), C.byref(calls)))
            _lib.check(L.osk_view_profile(view, 0))
            return (ms.value / max(1, calls.value), e0.elapsed_time(e1) / a.iters,
                    (counter("nested_sq8_settled_rows") - s0) / a.iters)

        # scan_f32: bench.py's `fp32_stream` configuration (no prefilter: every k-NN search on the fp32 scan)
        variants = {"scan_f32": (knn, {"sq8": 0}), "nest_scan_f32": (nested, {"sq8": 1, "nest_sq8": 0}),
                    "nest_scan_sq8": (nested, {"sq8": 1, "nest_sq8": 1}), "thr_scan_sq8": (threshold, {"sq8": 1, "thr_sq8": 1})}
        res = {name: [] for name in variants}
        for r in range(a.rounds):
            for name, (fn, knobs) in variants.items():
                res[name].append(timed(fn, knobs))
            print(f"family {fam}: round {r} done", file=sys.stderr, flush=True)
        c0 = counter("nested_sq8_calls")
        nested()
        torch.cuda.synchronize()
        assert counter("nested_sq8_calls") - c0 == 1, "the int8 first pass did not run"
        families_returned = int(kcnt.sum().item())
        keys8 = keys.clone()
        _lib.tune("nest_sq8", 0)
        nested()
        torch.cuda.synchronize()
        _lib.tune("nest_sq8", 1)
        assert torch.equal(keys8, keys), "the two nested paths disagree"

        def med(name, i):
            return statistics.median(x[i] for x in res[name])

        out["families"][str(fam)] = {
            "parents_per_shard": int(mask.sum()), "families_returned": families_returned,
            "scan_f32_kernel_ms": med("scan_f32", 0), "scan_f32_GBps": corpus_gb / (med("scan_f32", 0) * 1e-3),
            "knn_call_stream_ms": med("scan_f32", 1),
            "nest_scan_kernel_ms": med("nest_scan_f32", 0), "nest_scan_GBps": corpus_gb / (med("nest_scan_f32", 0) * 1e-3),
            "nest_scan_over_scan_f32": med("nest_scan_f32", 0) / med("scan_f32", 0),
            "nest_call_stream_ms": med("nest_scan_f32", 1),
            "nest_rest_ms_upper_bound": med("nest_scan_f32", 1) - med("nest_scan_f32", 0),
            "nest_scan_sq8_kernel_ms": med("nest_scan_sq8", 0), "thr_scan_sq8_kernel_ms": med("thr_scan_sq8", 0),
            "nest_scan_sq8_over_thr_scan_sq8": med("nest_scan_sq8", 0) / med("thr_scan_sq8", 0),
            "nest_sq8_call_stream_ms": med("nest_scan_sq8", 1),
            "nest_sq8_call_over_f32_call": med("nest_scan_sq8", 1) / med("nest_scan_f32", 1),
            # prep + clears + the floor's nest_topk and merge_shards + nest_settle_f32 + nest_topk + merge_shards
            "nest_sq8_rest_ms_upper_bound": med("nest_scan_sq8", 1) - med("nest_scan_sq8", 0),
            # ...of which the fp32 call has all but the floor, the settle and one clear
            "floor_and_settle_ms_upper_bound": (med("nest_scan_sq8", 1) - med("nest_scan_sq8", 0)) -
                                               (med("nest_scan_f32", 1) - med("nest_scan_f32", 0)),
            "settled_rows_per_call": med("nest_scan_sq8", 2),
            "per_round": {k_: [[round(x, 4) for x in p] for p in v] for k_, v in res.items()},
        }
        _lib.check(L.osk_view_release(view))
        for h in segs:
            _lib.check(L.osk_seg_release(h))
        torch.cuda.synchronize()

    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
