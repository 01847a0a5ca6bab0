"""Similarity-threshold search of float32 views through the certified int8 first pass:
`thr_scan_sq8` classifies every accepted row from its int8 score interval [lb, ub] — sure hit, sure miss, or
maybe — and `thr_settle_f32` re-scores the maybes exactly.  Results must not change: docs, score bits, count,
total and visited equal the fp32 path's and the oracle's, with no tolerance.

Reference for every case, as in test_gpu_threshold.py: `oracle.exact_search(rows, q, k = n_rows, sim,
ORDER_DEVICE, ord_to_doc, accept_bits)` filtered by a float32 `>=` and sorted by doc.  Every case runs with the
knob `thr_sq8` at 1 and at 0 and the two must agree bit for bit; a case meant to take the new path asserts that
the view's `threshold_sq8_calls` moved (a silent fallback to the fp32 scan would pass everything else).

The wave split is the part that can go wrong quietly: the masks are addressed per wave by the FLOAT32 lane
config's rows per step R, the int8 pass walks the rows in another config (R8).  Dims 50, 1000 and 2048 are the
ones where R ≠ R8 (8/16, 2/4, 1/2); the others pair equal R with different L and V.
"""
import contextlib

import numpy as np
import pytest

import bounds_inputs as BI
from opensearch_amd import _lib, lucene as LU
from oracle import bounds_reference as BR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIM = LU.VectorSimilarityFunction
F32, BYTE = LU.VectorEncoding.FLOAT32, LU.VectorEncoding.BYTE
NEG_INF, POS_INF = np.float32(-np.inf), np.float32(np.inf)
INT32_MAX = 2**31 - 1
DIST = {SIM.EUCLIDEAN: 1, SIM.DOT_PRODUCT: 3, SIM.COSINE: 3, SIM.MAXIMUM_INNER_PRODUCT: 2}   # O.synth's usual

_oracle_cache: dict = {}


def synth(n, dim, seed, sim=SIM.COSINE):
    return O.synth(0, n, dim, seed, DIST[sim])


def all_scores(key, rows, q, sim, o2d=None, accept=None):
    """Every accepted non-NaN row of one leaf as (docs, scores) in doc order, and visited; one oracle call per key."""
    if key not in _oracle_cache:
        docs = np.arange(len(rows)) if o2d is None else o2d
        if len(rows) == 0 or (accept is not None and not accept[docs].any()):   # nothing for the oracle to visit
            _oracle_cache[key] = (np.zeros(0, np.int32), np.zeros(0, np.float32), 0)
        else:
            ab = None if accept is None else O.bits_from_bool(accept)
            s, d, vis = O.exact_search(rows, q, len(rows), int(sim), O.ORDER_DEVICE, o2d, ab)
            order = np.argsort(d, kind="stable")
            _oracle_cache[key] = (d[order].copy(), s[order].copy(), vis)
        for a in _oracle_cache[key][:2]:
            a.setflags(write=False)
    return _oracle_cache[key]


def reference(scored, min_score, doc_base=0):
    d, s, vis = scored
    keep = s >= np.float32(min_score)          # float32 comparison: NaN on either side is False, −0 == +0
    return d[keep] + doc_base, s[keep], vis


def jth_best(scored, j):
    s = np.sort(scored[1])[::-1]
    return s[min(j, len(s)) - 1]


def assert_hits(got, want, cap, ctx=""):
    docs, scores, count, total = got
    wd, ws = want[0], want[1]
    assert int(total) == len(wd), (ctx, int(total), len(wd))
    n = min(len(wd), cap)
    assert int(count) == n, (ctx, int(count), n)
    assert np.array_equal(docs[:n], wd[:n]), ctx
    assert np.array_equal(scores[:n].view(np.uint32), ws[:n].view(np.uint32)), ctx
    assert np.all(docs[n:cap] == INT32_MAX) and np.all(np.isneginf(scores[n:cap])), ctx


def same_bits(a, b, ctx=""):
    for x, y in zip(a, b):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), ctx


@contextlib.contextmanager
def knob(key, value, default):
    _lib.tune(key, value)
    try:
        yield
    finally:
        _lib.tune(key, default)


def both_paths(ds, fn, new_path=True, ctx=""):
    """fn() with thr_sq8 = 1 and = 0: the results agree bit for bit; the view's counter says which path ran."""
    c0 = ds.counter("threshold_sq8_calls")
    got = fn()
    took = ds.counter("threshold_sq8_calls") - c0
    assert (took >= 1) if new_path else (took == 0), (ctx, took)
    with knob("thr_sq8", 0, 1):
        old = fn()
        assert ds.counter("threshold_sq8_calls") - c0 == took, ctx
    same_bits(got, old, ctx)
    return got


class Leaf1:
    """One reader and the single-leaf view over it (the view carries the counters)."""

    def __init__(self, rows, sim, enc=F32, **kw):
        self.r = LU.GpuFlatVectorsReader("v", rows, sim, enc, **kw)
        self.ds = LU.DeviceShardSet([[LU.LeafReaderContext(0, 0, self.r)]], [0])

    def close(self):
        self.ds.close()
        self.r.close()

    def view(self, q, ms, cap, new_path=True, accept=None, ctx=""):
        """The host-view entry on both paths: (docs[nq, cap], scores, count[nq], total[nq])."""
        d, s, c, t = both_paths(self.ds, lambda: self.ds.search_threshold(q, ms, accept, cap), new_path, ctx)
        return d[:, 0], s[:, 0], c[:, 0], t[:, 0]

    def seg(self, q, ms, cap, bits=None):
        """The segment entry with the knob on and off (its own view: results only)."""
        got = self.r.search_threshold(q, ms, bits, cap)
        with knob("thr_sq8", 0, 1):
            old = self.r.search_threshold(q, ms, bits, cap)
        same_bits(got, old, "segment entry")
        return got


@contextlib.contextmanager
def leaf1(*a, **kw):
    v = Leaf1(*a, **kw)
    try:
        yield v
    finally:
        v.close()


def thresholds(scored):
    """The issue's thresholds, taken from the reference itself."""
    mx = jth_best(scored, 1)
    return np.array([mx, jth_best(scored, 10), jth_best(scored, 500), np.nextafter(mx, POS_INF),
                     NEG_INF, POS_INF, 0.0, -0.0, np.nan], np.float32)


# ------------------------------------------------------------------------------------------------
# lane configs: each dim selects another (fp32 config, int8 config) pair; 4097 rows
# ------------------------------------------------------------------------------------------------
DIMS = (7, 50, 100, 200, 384, 768, 1000, 2048, 4096)
CASES = [(dim, sim) for dim in DIMS for sim in (SIM if dim in (100, 768) else (SIM.EUCLIDEAN, SIM.COSINE))]


@pytest.mark.parametrize("dim,sim", CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_lane_configs_and_thresholds(dim, sim):
    n, cap = 4097, 4097
    rows = synth(n, dim, 100 + dim, sim)
    q = synth(2, dim, 7 + dim, sim)[1]
    scored = all_scores(("lane", dim, sim), rows, q, sim)
    ms = thresholds(scored)
    with leaf1(rows, sim) as v:
        # one 8-query call (two passes of the 4-query instantiation), through the view and the segment entry
        m8 = ms[[0, 1, 2, 3, 4, 6, 7, 8]]
        d, s, c, t = v.view(np.repeat(q[None], 8, 0), m8, cap)
        sd, ss, sc, st, sv = v.seg(np.repeat(q[None], 8, 0), m8, cap)
        same_bits((d, s, c, t), (sd, ss, sc, st))
        assert np.all(sv == n)
        for i, m in enumerate(m8):
            assert_hits((d[i], s[i], c[i], t[i]), reference(scored, m), cap, (dim, sim, i, m))
        assert t[3] == 0 and t[7] == 0                        # above the maximum; NaN threshold
        assert t[4] == t[5] == t[6] == len(scored[0])          # −inf, 0.0 and −0.0: every non-NaN row
        assert t[0] >= 1 and t[1] >= 10 and t[2] >= 500        # the row scoring exactly min_score is a hit
        # every threshold as a single-query call (the one-query instantiation)
        for m in ms:
            d1, s1, c1, t1 = v.view(q, m, cap, ctx=(dim, sim, m))
            assert_hits((d1[0], s1[0], c1[0], t1[0]), reference(scored, m), cap, (dim, sim, "single", m))


# ------------------------------------------------------------------------------------------------
# row counts: word edges, and 4·R·k ± 1 for the fp32 R of the dim (wave ranges that end inside a word; at
# k = 37 they span several words).  R ≠ R8 at dims 50 and 1000.
# ------------------------------------------------------------------------------------------------
FP32_R = {50: 8, 768: 4, 1000: 2}


@pytest.mark.parametrize("dim", sorted(FP32_R))
def test_row_counts_at_word_and_range_edges(dim):
    sim, R = SIM.EUCLIDEAN, FP32_R[dim]
    q = synth(1, dim, 301, sim)[0]
    for n in [1, 63, 64, 65] + [4 * R * k + e for k in (5, 37) for e in (-1, 1)]:
        rows = synth(n, dim, 300 + n, sim)
        scored = all_scores(("edge", dim, n), rows, q, sim)
        with leaf1(rows, sim) as v:
            for m in (NEG_INF, jth_best(scored, (n + 1) // 2), jth_best(scored, 1), jth_best(scored, n)):
                d, s, c, t = v.view(q, m, n + 3, ctx=(dim, n, m))
                assert_hits((d[0], s[0], c[0], t[0]), reference(scored, m), n + 3, (dim, n, m))
            assert v.seg(q, NEG_INF, n + 3)[4][0] == n


# ------------------------------------------------------------------------------------------------
# a view of 4 segments in 2 shards: a sparse ord_to_doc segment, non-zero doc bases, a 0-row segment; filters
# at 1 %, 50 %, nothing accepted and all ones on dense and sparse segments, and a mixed accept table — through
# the segment, host-view and device entries
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def view4():
    dim, sim = 200, SIM.COSINE
    sizes = [3000, 0, 1, 4097]
    shard_of = [0, 0, 0, 1]
    max_doc = [3000, 40, 1, 9000]
    rows = [synth(n, dim, 400 + i, sim) if n else np.zeros((0, dim), np.float32) for i, n in enumerate(sizes)]
    o2d = [None, None, None, np.sort(np.random.default_rng(5).choice(9000, sizes[3], replace=False)).astype(np.int32)]
    bases = [3, 3013, 3060, 17]
    readers = [LU.GpuFlatVectorsReader("v", rows[i], sim, F32, ord_to_doc=o2d[i], max_doc=max_doc[i]) for i in range(4)]
    leaves = [[LU.LeafReaderContext(i, bases[i], readers[i]) for i in range(3)], [LU.LeafReaderContext(0, bases[3], readers[3])]]
    ds = LU.DeviceShardSet(leaves, [0, 1])
    rng = np.random.default_rng(11)
    accepts = {name: [None if pct is None else rng.random(md) < pct for md in max_doc]
               for name, pct in (("1%", 0.01), ("50%", 0.5), ("none", 0.0), ("ones", 1.0))}
    accepts["mixed"] = [rng.random(3000) < 0.5, None, None, rng.random(9000) < 0.3]
    accepts[None] = None
    yield dict(dim=dim, sim=sim, rows=rows, o2d=o2d, max_doc=max_doc, bases=bases, readers=readers, ds=ds,
               queries=synth(9, dim, 450, sim), shard_of=shard_of, accepts=accepts)
    ds.close()
    for r in readers:
        r.close()


def view_reference(v, qi, min_score, aname=None):
    """Per shard (docs, scores) in shard-local doc order + visited per segment."""
    accept = v["accepts"][aname]
    per_shard, visited = [[], []], []
    for i in range(4):
        acc = None if accept is None else accept[i]
        scored = all_scores(("view4", i, qi, aname), v["rows"][i], v["queries"][qi], v["sim"], v["o2d"][i], acc)
        d, s, vis = reference(scored, min_score, v["bases"][i])
        per_shard[v["shard_of"][i]].append((d, s))
        visited.append(vis)
    return [(np.concatenate([p[0] for p in ps]), np.concatenate([p[1] for p in ps])) for ps in per_shard], visited


def view4_threshold(v, qi, j, aname=None):
    accept = v["accepts"][aname]
    s = np.concatenate([all_scores(("view4", i, qi, aname), v["rows"][i], v["queries"][qi], v["sim"], v["o2d"][i],
                                   None if accept is None else accept[i])[1] for i in range(4)])
    return np.sort(s)[::-1][min(j, len(s)) - 1] if len(s) else np.float32(0.5)


def device_call(v, q, ms, cap, accept=None):
    import torch
    ds = v["ds"]
    nq, S = len(q), ds.n_shards
    tq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    tms = torch.from_numpy(np.ascontiguousarray(ms, np.float32)).cuda()
    docs = torch.full((nq, S, cap), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((nq, S, cap), -7.0, dtype=torch.float32, device="cuda")
    count = torch.full((nq, S), -7, dtype=torch.int32, device="cuda")
    total = torch.full((nq, S), -7, dtype=torch.int64, device="cuda")
    visited = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    keep, table = [], None
    if accept is not None:
        for a in accept:
            keep.append(None if a is None else torch.from_numpy(LU.bits_from_bool(a).view(np.int64)).cuda())
        table = torch.tensor([0 if k is None else k.data_ptr() for k in keep], dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        _lib.check(_lib.lib().osk_view_search_threshold_device(
            ds.handle, tq.data_ptr(), nq, tms.data_ptr(), None if table is None else table.data_ptr(), cap,
            docs.data_ptr(), scores.data_ptr(), count.data_ptr(), total.data_ptr(), visited.data_ptr(), st.cuda_stream))
    st.synchronize()
    return docs.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy(), total.cpu().numpy(), visited.cpu().numpy()


@pytest.mark.parametrize("aname", [None, "1%", "50%", "none", "ones", "mixed"])
def test_view_entries_and_filters(view4, aname):
    v, cap = view4, 8000
    accept = v["accepts"][aname]
    for qi, j in [(0, 500), (1, 10)]:
        q = v["queries"][qi]
        for m in (view4_threshold(v, qi, j, aname), NEG_INF):
            want, visited = view_reference(v, qi, m, aname)
            ctx = (aname, qi, float(m))
            d, s, c, t = both_paths(v["ds"], lambda: v["ds"].search_threshold(q, m, accept, cap), True, ctx)
            dd, sd, cd, td, vd = both_paths(v["ds"], lambda: device_call(v, q[None], [m], cap, accept), True, ctx)
            for sh in range(2):
                assert_hits((d[0, sh], s[0, sh], c[0, sh], t[0, sh]), want[sh], cap, ("host",) + ctx)
                assert_hits((dd[0, sh], sd[0, sh], cd[0, sh], td[0, sh]), want[sh], cap, ("device",) + ctx)
            assert list(vd) == visited
            if aname != "none":
                assert sum(visited) > 0
            for i in (0, 3):                                    # the dense and the sparse segment's own entry
                acc = None if accept is None else accept[i]
                scored = all_scores(("view4", i, qi, aname), v["rows"][i], q, v["sim"], v["o2d"][i], acc)
                bits = None if acc is None else LU.bits_from_bool(acc)
                got = v["readers"][i].search_threshold(q, m, bits, cap)
                with knob("thr_sq8", 0, 1):
                    same_bits(got, v["readers"][i].search_threshold(q, m, bits, cap), ("seg",) + ctx)
                assert_hits((got[0][0], got[1][0], got[2][0], got[3][0]), reference(scored, m), cap, ("seg", i) + ctx)
                assert got[4][0] == scored[2]


@pytest.mark.parametrize("nq", [5, 9])
def test_batches_equal_single_queries(view4, nq):
    v, cap = view4, 256
    ms = np.array([view4_threshold(v, qi, j) for qi, j in zip(range(nq), [40, 1, 200, 10, 3, 77, 150, 2, 30])], np.float32)
    d, s, c, t = both_paths(v["ds"], lambda: v["ds"].search_threshold(v["queries"][:nq], ms, None, cap))
    for qi in range(nq):
        want, _ = view_reference(v, qi, ms[qi])
        d1, s1, c1, t1 = both_paths(v["ds"], lambda: v["ds"].search_threshold(v["queries"][qi], ms[qi], None, cap))
        for sh in range(2):
            assert_hits((d[qi, sh], s[qi, sh], c[qi, sh], t[qi, sh]), want[sh], cap, ("batch", qi, sh))
            assert_hits((d1[0, sh], s1[0, sh], c1[0, sh], t1[0, sh]), want[sh], cap, ("single", qi, sh))


# ------------------------------------------------------------------------------------------------
# capacity, ties, NaN scores
# ------------------------------------------------------------------------------------------------
def test_capacity_below_and_at_the_total():
    dim, sim, n = 100, SIM.COSINE, 4097
    rows = synth(n, dim, 800, sim)
    q = synth(1, dim, 801, sim)[0]
    scored = all_scores(("cap",), rows, q, sim)
    m = np.array([jth_best(scored, 500)], np.float32)
    want = reference(scored, m[0])
    total = len(want[0])
    assert total >= 500
    with leaf1(rows, sim) as v:
        for cap in (7, total):
            def call():
                guard = 16
                docs = np.full(cap + guard, -7, np.int32)
                scores = np.full(cap + guard, -7, np.float32)
                count, tot, vis = np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.int64)
                qq = np.ascontiguousarray(q[None])
                _lib.check(_lib.lib().osk_seg_search_threshold(v.r.handle, qq.ctypes.data, 1, m.ctypes.data, None, cap,
                                                               docs.ctypes.data, scores.ctypes.data, count.ctypes.data,
                                                               tot.ctypes.data, vis.ctypes.data))
                return docs, scores, count, tot, vis
            docs, scores, count, tot, vis = call()
            with knob("thr_sq8", 0, 1):
                same_bits((docs, scores, count, tot, vis), call())
            assert count[0] == cap and tot[0] == total and vis[0] == n
            assert np.array_equal(docs[:cap], want[0][:cap])
            assert np.array_equal(scores[:cap].view(np.uint32), want[1][:cap].view(np.uint32))
            assert np.all(docs[cap:] == -7) and np.all(scores[cap:] == -7)      # the guard values
            d, s, c, t = v.view(q, m[0], cap)                                   # (the view entry took the new path)
            assert_hits((d[0], s[0], c[0], t[0]), want, cap)


def test_ties_at_the_threshold():
    dim, sim = 100, SIM.DOT_PRODUCT
    base = synth(300, dim, 500, sim)
    rows = np.ascontiguousarray(np.tile(base, (4, 1)))          # row i, i + 300, i + 600, i + 900 are equal
    q = synth(1, dim, 501, sim)[0]
    scored = all_scores(("ties",), rows, q, sim)
    m = jth_best(scored, 20)                                     # a tied score (ranks 17..20)
    want = reference(scored, m)
    at = want[0][want[1] == m]
    assert len(at) == 4 and len(set(at % 300)) == 1 and len(want[0]) == 20
    with leaf1(rows, sim) as v:
        d, s, c, t = v.view(q, m, 64)
        assert_hits((d[0], s[0], c[0], t[0]), want, 64)
        assert np.all(np.diff(d[0, :c[0]]) > 0)


def test_nan_scores_are_never_hits():
    dim = 100
    rows = synth(1000, dim, 600)
    rows[::7] = 0                                                # zero rows: NaN under COSINE
    q = synth(1, dim, 601)[0]
    scored = all_scores(("nan",), rows, q, SIM.COSINE)
    assert len(scored[0]) == 1000 - len(rows[::7])
    with leaf1(rows, SIM.COSINE) as v:
        for m in (NEG_INF, 0.0, jth_best(scored, 10)):
            d, s, c, t = v.view(np.zeros(dim, np.float32), m, 16)          # a zero query: every score NaN
            assert t[0] == 0 and c[0] == 0
            assert np.all(d[0] == INT32_MAX) and np.all(np.isneginf(s[0]))
            d, s, c, t = v.view(q, m, 1000)
            assert_hits((d[0], s[0], c[0], t[0]), reference(scored, m), 1000)
            assert not np.isnan(s[0, :c[0]]).any()
        assert v.seg(q, NEG_INF, 16)[4][0] == 1000


# ------------------------------------------------------------------------------------------------
# the certificate's range (osk_device.h sq8_in_range): rows outside it keep the fp32 scan, a query outside it
# is settled row by row; byte fields never take the int8 first pass
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [SIM.EUCLIDEAN, SIM.MAXIMUM_INNER_PRODUCT], ids=lambda s: s.name)
def test_a_row_out_of_range_keeps_the_fp32_scan(sim):
    dim, n = 100, 1500
    rows = synth(n, dim, 900, sim)
    rows[777] *= np.float32(2.0 ** 40)
    q = synth(1, dim, 901, sim)[0]
    scored = all_scores(("row-range", sim), rows, q, sim)
    with leaf1(rows, sim) as v:
        v.ds.search_threshold(q, 0.5, None, 8)                   # (the first call builds the int8 copy and finds out)
        for m in (NEG_INF, jth_best(scored, 10), jth_best(scored, 1)):
            d, s, c, t = v.view(q, m, n, new_path=False)
            assert_hits((d[0], s[0], c[0], t[0]), reference(scored, m), n, (sim, m))


@pytest.mark.parametrize("sim", [SIM.EUCLIDEAN, SIM.COSINE, SIM.MAXIMUM_INNER_PRODUCT], ids=lambda s: s.name)
def test_a_query_out_of_range_is_settled_row_by_row(sim):
    dim, n = 100, 1500
    rows = synth(n, dim, 910, sim)
    acc = np.random.default_rng(3).random(n) < 0.5
    q = synth(1, dim, 911, sim)[0] * np.float32(2.0 ** 40)
    for accept, n_acc in ((None, n), ([acc], int(acc.sum()))):
        scored = all_scores(("query-range", sim, accept is None), rows, q, sim, None, None if accept is None else acc)
        with leaf1(rows, sim) as v:
            for m in (jth_best(scored, 10), np.float32(0.0)):
                s0 = v.ds.counter("threshold_sq8_settled_rows")
                c0 = v.ds.counter("threshold_sq8_calls")
                d, s, c, t = v.ds.search_threshold(q, m, accept, n)
                assert v.ds.counter("threshold_sq8_calls") - c0 == 1
                assert v.ds.counter("threshold_sq8_settled_rows") - s0 == n_acc
                assert_hits((d[0, 0], s[0, 0], c[0, 0], t[0, 0]), reference(scored, m), n, (sim, m))


def test_a_byte_field_never_takes_the_int8_first_pass():
    dim, n = 100, 2000
    rows = O.synth(0, n, dim, 920, _lib.DIST_INT8)
    q = O.synth(0, 1, dim, 921, _lib.DIST_INT8)[0]
    scored = all_scores(("byte",), rows, q, SIM.DOT_PRODUCT)
    with leaf1(rows, SIM.DOT_PRODUCT, BYTE) as v:
        m = jth_best(scored, 25)
        d, s, c, t = v.view(q, m, 64, new_path=False)
        assert_hits((d[0], s[0], c[0], t[0]), reference(scored, m), 64)
        assert v.ds.counter("threshold_sq8_settled_rows") == 0


# ------------------------------------------------------------------------------------------------
# the classification, checked exactly (testing build): the rows the settle re-scores are the rows whose record
# of the select path's writer (the same interval function, sel_writer 2) straddles min_score
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [100, 768])
@pytest.mark.parametrize("sim", list(SIM), ids=lambda s: s.name)
def test_the_settle_re_scores_exactly_the_straddling_rows(sim, dim):
    n = 4097
    rows = synth(n, dim, 1000 + dim, sim)
    q = synth(2, dim, 1001 + dim, sim)[1]
    scored = all_scores(("class", dim, sim), rows, q, sim)
    ms = jth_best(scored, 10)
    with _lib.testing(), knob("sel_writer", 2, 2), leaf1(rows, sim) as v:
        c0 = v.ds.counter("select_calls")
        v.ds.search(q[None], 13, 0, 13)
        assert v.ds.counter("select_calls") - c0 == 1
        LB, UB = BI.select_records(v.ds, n)
        have = ~((LB == 0) & (UB == 0))
        lb, ub = BR.from_sortable(LB), BR.from_sortable(UB)
        with np.errstate(invalid="ignore"):
            maybe = have & ~(lb >= ms) & ~(ub < ms)
            sure = have & (lb >= ms)
        expected = int(maybe.sum())
        assert 1 <= expected < n, (expected, n)
        for m, want_settled in ((ms, expected), (NEG_INF, 0), (POS_INF, 0)):
            s0 = v.ds.counter("threshold_sq8_settled_rows")
            c0 = v.ds.counter("threshold_sq8_calls")
            d, s, c, t = v.ds.search_threshold(q, m, None, n)
            assert v.ds.counter("threshold_sq8_calls") - c0 == 1
            assert v.ds.counter("threshold_sq8_settled_rows") - s0 == want_settled, (sim, dim, float(m))
            assert_hits((d[0, 0], s[0, 0], c[0, 0], t[0, 0]), reference(scored, m), n, (sim, dim, float(m)))
        # the sure rows are hits, and every hit is sure or was a maybe
        hits = np.zeros(n, bool)
        hits[reference(scored, ms)[0]] = True
        assert np.all(hits[sure]) and not np.any(hits & ~sure & ~maybe)


def test_all_maybe_settles_every_visited_row():
    dim, sim, n = 384, SIM.MAXIMUM_INNER_PRODUCT, 4097
    rows = synth(n, dim, 1100, sim)
    q = synth(4, dim, 1101, sim)
    acc = np.random.default_rng(4).random(n) < 0.5
    with _lib.testing(), leaf1(rows, sim) as v:
        for accept, n_acc in ((None, n), ([acc], int(acc.sum()))):
            scored = [all_scores(("maybe", qi, accept is None), rows, q[qi], sim, None, None if accept is None else acc)
                      for qi in range(4)]
            ms = np.array([jth_best(scored[0], 10), NEG_INF, jth_best(scored[2], 500), np.nan], np.float32)
            plain = v.ds.search_threshold(q, ms, accept, n)
            with knob("thr_sq8_all_maybe", 1, 0):
                s0 = v.ds.counter("threshold_sq8_settled_rows")
                c0 = v.ds.counter("threshold_sq8_calls")
                forced = v.ds.search_threshold(q, ms, accept, n)
                assert v.ds.counter("threshold_sq8_calls") - c0 == 1
                assert v.ds.counter("threshold_sq8_settled_rows") - s0 == 4 * n_acc
            same_bits(plain, forced)
            for qi in range(4):
                assert_hits((forced[0][qi, 0], forced[1][qi, 0], forced[2][qi, 0], forced[3][qi, 0]),
                            reference(scored[qi], ms[qi]), n, qi)
