#!/usr/bin/env python3
"""Radial search collected by score on the device against the route that answered it before, same view, same run,
interleaved.

  python tools/bench_threshold_top.py [--rows-per-shard N] [--rounds R] [--iters I] [--shapes f32,byte] [--out FILE]

Stages the C3 shape (8 shards × 1.25M × 768 fp32 COSINE, synthetic as bench.py builds it) and a byte shape
(8 × 1.25M × 768 int8 DOT_PRODUCT) and, for one query, thresholds at the view's 10th, 10⁴th and 10⁶th best score and
k = 10 and k = 1000 — and a batch of 4 queries (one full pass) at k = 1000, every query under the same threshold,
where the old route's buffers here can hold it — measures round-robin:
  * top      osk_view_search_threshold_top_device: stream ms around the calls (events), and host-clock ms of
             call + the copy of the shard lists (k keys, count and total per shard) + synchronise;
  * old      the route of `rewrite` + sort: osk_view_search_threshold_device — the UNCHANGED positional entry —
             with cap = the largest shard total (what rewrite's second call asks for; its first, 1024-hit call is
             left out, in the old route's favour), the device-to-host copy of every shard's hits (doc + score,
             8 bytes each), and the host sort by (−score, doc) cut to k per shard.  Stream ms of the call alone,
             and host-clock ms of call + copy + sort.
Both routes must return the same docs (checked once per case).  Events and the host clock bracket work that ends
in a synchronise.  Prints one JSON line per shape.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opensearch_amd import _lib  # noqa: E402
from opensearch_amd.lucene import decode_keys, synth_host  # noqa: E402

L = _lib.lib()
RANKS = (10, 10_000, 1_000_000)
KS = (10, 1000)


def run_shape(a, name, enc, sim, dist):
    dim, nsh, n = a.dim, 8, a.rows_per_shard
    segs = []
    for s in range(nsh):
        h = C.c_void_p()
        _lib.check(L.osk_seg_synth(0, n, dim, enc, sim, 42, dist, s * n, C.byref(h)))
        segs.append(h)
    arr = (C.c_void_p * nsh)(*[h.value for h in segs])
    seg_shard = np.arange(nsh, dtype=np.int32)
    view = C.c_void_p()
    _lib.check(L.osk_view_create(arr, nsh, seg_shard.ctypes.data, None, nsh, None, C.byref(view)))
    stream = torch.cuda.current_stream().cuda_stream

    NQB = 4                                   # the batch cases: one full pass of kThrNQ queries
    qb_host = synth_host(0, NQB, dim, 43, dist)   # (row 0 is the single query)
    qb = torch.from_numpy(qb_host).cuda()
    docs = torch.empty(nsh * n, dtype=torch.int32, device="cuda")        # the old entry's [query][shard][cap]
    scores = torch.empty(nsh * n, dtype=torch.float32, device="cuda")
    tcnt = torch.empty((NQB, nsh), dtype=torch.int32, device="cuda")
    ttot = torch.empty((NQB, nsh), dtype=torch.int64, device="cuda")
    h_docs = torch.empty(nsh * n, dtype=torch.int32).pin_memory()
    h_scores = torch.empty(nsh * n, dtype=torch.float32).pin_memory()

    def old_call(nq, ms, cap):
        assert nq * nsh * cap <= nsh * n
        _lib.check(L.osk_view_search_threshold_device(view, qb.data_ptr(), nq, ms.data_ptr(), None, cap, docs.data_ptr(),
                                                      scores.data_ptr(), tcnt.data_ptr(), ttot.data_ptr(), None, stream))

    # every row's score (min_score = −inf, cap = a shard's rows) → the thresholds by rank
    ms_all = torch.tensor([float("-inf")], dtype=torch.float32, device="cuda")
    old_call(1, ms_all, n)
    torch.cuda.synchronize()
    cnt = tcnt[0].cpu().numpy()
    every = torch.cat([scores[s * n: s * n + int(cnt[s])] for s in range(nsh)]).sort(descending=True).values
    ranks = [r for r in RANKS if r <= every.numel()]
    thresholds = {r: float(every[r - 1].item()) for r in ranks}
    del every

    def old_route(nq, ms, cap, k):
        """call, copy every hit to the host, sort there: per (query, shard) (docs, scores) of the best k"""
        old_call(nq, ms, cap)
        cn = tcnt[:nq].cpu().numpy().reshape(-1)   # (synchronises: the copies below need the counts)
        for i in range(nq * nsh):
            h_docs[i * cap: i * cap + cn[i]].copy_(docs[i * cap: i * cap + cn[i]], non_blocking=True)
            h_scores[i * cap: i * cap + cn[i]].copy_(scores[i * cap: i * cap + cn[i]], non_blocking=True)
        torch.cuda.synchronize()
        out = []
        for i in range(nq * nsh):
            d, sc = h_docs[i * cap: i * cap + cn[i]].numpy(), h_scores[i * cap: i * cap + cn[i]].numpy()
            order = np.lexsort((d, -sc.astype(np.float64)))[:k]
            out.append((d[order], sc[order]))
        return out

    def timed_stream(fn, iters):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def timed_host(fn, iters):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    def make_case(r, k, nq):
        """buffers and closures of one case (every query of a batch under the rank's threshold), both routes
        checked against each other once"""
        ms = torch.full((nq,), thresholds[r], dtype=torch.float32, device="cuda")
        old_call(nq, ms, 1)
        torch.cuda.synchronize()
        cap = max(1, int(ttot[:nq].max().item()))
        hits = int(ttot[:nq].sum().item())
        if nq * cap > n:
            return None                              # (the old route's buffers here hold one shard set of rows)
        keys = torch.empty((nq, nsh, k), dtype=torch.int64, device="cuda")
        kcnt = torch.empty((nq, nsh), dtype=torch.int32, device="cuda")
        ktot = torch.empty((nq, nsh), dtype=torch.int64, device="cuda")
        h_keys = torch.empty((nq * nsh, k), dtype=torch.int64).pin_memory()

        def top_call():
            _lib.check(L.osk_view_search_threshold_top_device(view, qb.data_ptr(), nq, ms.data_ptr(), k, None,
                                                              keys.data_ptr(), kcnt.data_ptr(), ktot.data_ptr(),
                                                              None, stream))

        def top_route():
            top_call()
            h_keys.copy_(keys.view(nq * nsh, k), non_blocking=True)
            c, t = kcnt.cpu(), ktot.cpu()
            torch.cuda.synchronize()
            return h_keys, c.reshape(-1), t

        want = old_route(nq, ms, cap, k)
        hk, c, t = top_route()
        assert int(t.sum().item()) == hits, (name, r, k, nq)
        s_new, d_new = decode_keys(hk.numpy().view(np.uint64))
        for i in range(nq * nsh):
            m = int(c[i].item())
            assert m == len(want[i][0]) and np.array_equal(d_new[i, :m], want[i][0]), (name, r, k, nq, i)
            assert np.array_equal(s_new[i, :m].view(np.uint32), want[i][1].view(np.uint32)), (name, r, k, nq, i)
        return dict(ms=ms, cap=cap, hits=hits, top_call=top_call, top_route=top_route)

    cases = {}
    for r in ranks:
        for k, nq in [(k, 1) for k in KS] + [(KS[-1], NQB)]:
            cse = make_case(r, k, nq)
            if cse is not None:
                cases[(r, k, nq)] = cse

    res = {key: {"top_stream": [], "top_host": [], "old_stream": [], "old_host": []} for key in cases}
    for rnd in range(a.rounds):
        for (r, k, nq), cse in cases.items():
            slow = cse["hits"] > 100_000                     # the old route's host sort takes long: fewer repeats
            it = max(2, a.iters // 5) if slow else a.iters
            x = res[(r, k, nq)]
            x["top_stream"].append(timed_stream(cse["top_call"], a.iters))
            x["old_stream"].append(timed_stream(lambda: old_call(nq, cse["ms"], cse["cap"]), it))
            x["top_host"].append(timed_host(cse["top_route"], a.iters))
            x["old_host"].append(timed_host(lambda: old_route(nq, cse["ms"], cse["cap"], k), it))
        print(f"{name}: round {rnd} done", file=sys.stderr, flush=True)

    def counter(cname):
        v = C.c_int64()
        _lib.check(L.osk_view_counter(view, cname.encode(), C.byref(v)))
        return v.value

    elem = 4 if enc == _lib.FLOAT32 else 1
    out = {"shape": f"{nsh} shards x {n} x {dim} {name}", "corpus_GB": nsh * n * dim * elem / 1e9,
           "rounds": a.rounds, "iters": a.iters, "int8_first_pass_calls": counter("threshold_sq8_calls"),
           "top_calls": counter("threshold_top_calls"), "top_select_calls": counter("threshold_top_select_calls"),
           "cases": []}
    for (r, k, nq), x in res.items():
        med = {m: statistics.median(v) for m, v in x.items()}
        out["cases"].append({
            "rank": r, "k": k, "queries": nq, "min_score": thresholds[r], "hits": cases[(r, k, nq)]["hits"],
            "old_cap_per_shard": cases[(r, k, nq)]["cap"],
            "top_stream_ms": med["top_stream"], "old_stream_ms": med["old_stream"],
            "top_host_ms": med["top_host"], "old_host_ms": med["old_host"],
            "stream_speedup": med["old_stream"] / med["top_stream"], "host_speedup": med["old_host"] / med["top_host"],
            "spread": {m: [round(min(v), 4), round(max(v), 4)] for m, v in x.items()}})
    _lib.check(L.osk_view_release(view))
    for h in segs:
        _lib.check(L.osk_seg_release(h))
    del docs, scores
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-per-shard", type=int, default=1_250_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", default="f32,byte")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_threshold_top.py needs a GPU: nothing here is measured without one")
    torch.cuda.set_device(0)
    torch.cuda.set_stream(torch.cuda.Stream())   # non-null: 0 would mean the library's own stream
    shapes = {"f32": ("fp32 COSINE", _lib.FLOAT32, _lib.COSINE, _lib.DIST_NORMALISH_UNIT),
              "byte": ("int8 DOT_PRODUCT", _lib.BYTE, _lib.DOT_PRODUCT, _lib.DIST_INT8)}
    lines = []
    for key in a.shapes.split(","):
        line = json.dumps(run_shape(a, *shapes[key]))
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
