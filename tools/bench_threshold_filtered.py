#!/usr/bin/env python3
"""Filtered similarity-threshold calls: the fp32 scan against the certified int8 first pass, same view, same run.

  python tools/bench_threshold_filtered.py [OUT.json]

Stages the C3 shape (8 shards × 1.25M × 768 fp32 COSINE, dense segments) and, for Bernoulli accept bitsets of 1 %,
10 % and 50 % per shard, times the whole device-entry call on its stream with tune thr_sq8 = 0 and = 1, alternated
(5 rounds × 20 calls, medians), min_score = 0.57.  Both paths compact the accepted rows of a dense segment
(walk_rows), so each reads only those rows: 3072 B against 784 B each.  Prints one JSON line."""
import ctypes as C, json, os, statistics, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opensearch_amd import _lib
from opensearch_amd.lucene import synth_host
L = _lib.lib()
torch.cuda.set_device(0)
dim, nsh, n = 768, 8, 1_250_000
segs = []
for s in range(nsh):
    h = C.c_void_p()
    _lib.check(L.osk_seg_synth(0, n, dim, _lib.FLOAT32, _lib.COSINE, 42, _lib.DIST_NORMALISH_UNIT, s * n, C.byref(h)))
    segs.append(h.value)
arr = (C.c_void_p * nsh)(*segs)
seg_shard = np.arange(nsh, dtype=np.int32)
view = C.c_void_p()
_lib.check(L.osk_view_create(arr, nsh, seg_shard.ctypes.data, None, nsh, None, C.byref(view)))
q = torch.from_numpy(synth_host(0, 1, dim, 43, _lib.DIST_NORMALISH_UNIT)).cuda()
cap = 1024
docs = torch.empty((1, nsh, cap), dtype=torch.int32, device="cuda")
scores = torch.empty((1, nsh, cap), dtype=torch.float32, device="cuda")
tcnt = torch.empty((1, nsh), dtype=torch.int32, device="cuda")
ttot = torch.empty((1, nsh), dtype=torch.int64, device="cuda")
ms = torch.tensor([0.57], dtype=torch.float32, device="cuda")
torch.cuda.set_stream(torch.cuda.Stream())
stream = torch.cuda.current_stream().cuda_stream
out = {}
for pct in (1, 10, 50):
    g = torch.Generator(device="cuda"); g.manual_seed(pct)
    words = (n + 63) // 64
    bits = []
    for s in range(nsh):
        m = (torch.rand(words * 64, device="cuda", generator=g) < pct / 100).view(words, 64)
        w = (m.to(torch.int64) << torch.arange(64, device="cuda", dtype=torch.int64)).sum(1)   # wraps at bit 63: fine
        bits.append(w.contiguous())
    table = torch.tensor([b.data_ptr() for b in bits], dtype=torch.int64, device="cuda")
    def call():
        _lib.check(L.osk_view_search_threshold_device(view, q.data_ptr(), 1, ms.data_ptr(), table.data_ptr(), cap,
                   docs.data_ptr(), scores.data_ptr(), tcnt.data_ptr(), ttot.data_ptr(), None, stream))
    res = {0: [], 1: []}
    tot = {}
    for r in range(5):
        for knob in (0, 1):
            _lib.tune("thr_sq8", knob)
            for _ in range(2): call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20): call()
            e1.record(); torch.cuda.synchronize()
            res[knob].append(e0.elapsed_time(e1) / 20)
            tot[knob] = int(ttot.sum().item())
    assert tot[0] == tot[1]
    out[f"{pct}%"] = {"fp32_call_ms": statistics.median(res[0]), "sq8_call_ms": statistics.median(res[1]), "hits": tot[0]}
_lib.tune("thr_sq8", 1)
print(json.dumps(out))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write(json.dumps(out) + "\n")
