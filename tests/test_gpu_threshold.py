"""Exact similarity-threshold (radial) search on the device: every accepted vector scoring ≥ min_score, in doc
order, with the exact total ([L] AbstractVectorSimilarityQuery / FloatVectorSimilarityQuery /
ByteVectorSimilarityQuery on a flat field; OpenSearch's k-NN `min_score`).

Reference for every case: `oracle.exact_search(rows, q, k = n_rows, sim, ORDER_DEVICE, ord_to_doc, accept_bits)`
gives every accepted row's device-order score; keep `score >= min_score` as a numpy float32 comparison (NaN is
out), sort by doc.  Required: docs equal, score bits equal, total equal, visited equal.
"""

import numpy as np
import pytest

from opensearch_amd import _lib, dsl as Q, lucene as LU
from oracle import byte_reference as BR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIM = LU.VectorSimilarityFunction
F32, BYTE = LU.VectorEncoding.FLOAT32, LU.VectorEncoding.BYTE
NEG_INF = np.float32(-np.inf)
INT32_MAX = 2**31 - 1

_oracle_cache: dict = {}


def synth(n, dim, seed, enc=F32):
    return O.synth(0, n, dim, seed, _lib.DIST_INT8 if enc == BYTE else _lib.DIST_NORMALISH_UNIT)


def all_scores(key, rows, q, sim, o2d=None, accept=None):
    """Every accepted non-NaN row of one leaf as (docs, scores) in doc order, and visited.  One oracle call per
    `key`, shared by the tests."""
    if key not in _oracle_cache:
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


def thresholds(scored):
    """The issue's thresholds, taken from the reference itself."""
    mx = jth_best(scored, 1)
    return np.array([jth_best(scored, 1), jth_best(scored, 10), jth_best(scored, 500),
                     np.nextafter(mx, np.float32(np.inf)), NEG_INF, 0.0, -0.0, np.nan], np.float32)


# ------------------------------------------------------------------------------------------------
# lane configs and padding × similarities, 4097 rows: wave ranges that are no multiple of 64
# ------------------------------------------------------------------------------------------------
CASES = [(F32, dim, sim) for dim in (3, 96, 128, 768, 1030) for sim in SIM] + \
        [(BYTE, dim, sim) for dim in (16, 100, 768) for sim in (SIM.EUCLIDEAN, SIM.DOT_PRODUCT)]
# byte lane configs whose 4-query instantiation reads its query fragments from LDS (dims above 1024) or keeps them
# in registers (250), on the two similarities the cases above leave out; these corpora carry the byte edge set
# (byte_reference.edge_rows: all −128, all 127, alternating, all 0 — NaN under COSINE —, a duplicate, all 1)
BYTE_EDGE_CASES = [(BYTE, dim, sim) for dim in (250, 1100, 3000, 4096) for sim in (SIM.COSINE, SIM.MAXIMUM_INNER_PRODUCT)]
CASES += BYTE_EDGE_CASES


@pytest.mark.parametrize("enc,dim,sim", CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_lane_configs_and_thresholds(enc, dim, sim):
    n = 4097
    rows = synth(n, dim, 100 + dim, enc)
    q = synth(2, dim, 7 + dim, enc)[1]
    edges = (enc, dim, sim) in BYTE_EDGE_CASES
    if edges:
        BR.inject_edges(rows)
    r = LU.GpuFlatVectorsReader("v", rows, sim, enc)
    try:
        scored = all_scores(("lane", enc, dim, sim), rows, q, sim)
        ms = thresholds(scored)
        cap = n
        # one call, the same target under 8 thresholds (two corpus passes of the wide instantiation) ...
        d, s, c, t, v = r.search_threshold(np.repeat(q[None], len(ms), 0), ms, None, cap)
        for i, m in enumerate(ms):
            want = reference(scored, m)
            assert_hits((d[i], s[i], c[i], t[i]), want, cap, (enc, dim, sim, i, m))
            assert v[i] == want[2] == n
        assert t[3] == 0 and c[3] == 0 and t[7] == 0          # above the maximum; NaN threshold
        assert t[4] == t[5] == t[6] == len(scored[0])          # −inf, 0.0 and −0.0: every non-NaN row
        assert t[0] >= 1 and t[1] >= 10 and t[2] >= 500        # the row scoring exactly min_score is a hit
        # ... and a single-query call (the one-query instantiation) gives the same
        d1, s1, c1, t1, v1 = r.search_threshold(q, ms[1], None, cap)
        assert_hits((d1[0], s1[0], c1[0], t1[0]), reference(scored, ms[1]), cap)
        assert v1[0] == n
        if edges:
            # the oracle's scores are byte_reference's, row for row (the zero rows are the ones left out)
            ref = BR.scores(rows, q, int(sim))
            assert np.array_equal(np.flatnonzero(~np.isnan(ref)), scored[0])
            assert np.array_equal(ref[scored[0]].view(np.uint32), scored[1].view(np.uint32))
            assert (len(scored[0]) < n) == (sim == SIM.COSINE)
            # the edge queries: all −128, all 127, and all 0 (COSINE: every score NaN, no hit; MIP: every score 1)
            for j, fill in enumerate((-128, 127, 0)):
                qe = np.full(dim, fill, np.int8)
                se = all_scores(("lane-edge", dim, sim, j), rows, qe, sim)
                me = np.array([NEG_INF, jth_best(se, 10) if len(se[1]) else 0.0, 1.0, 0.5], np.float32)
                d, s, c, t, v = r.search_threshold(np.repeat(qe[None], len(me), 0), me, None, cap)
                for i, m in enumerate(me):
                    assert_hits((d[i], s[i], c[i], t[i]), reference(se, m), cap, (dim, sim, fill, m))
                    assert v[i] == n
                if fill == 0:
                    assert t[0] == (0 if sim == SIM.COSINE else n) and t[2] == t[0]
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# row counts at word and range edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc,dim", [(F32, 96), (BYTE, 16)], ids=["f32", "byte"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_row_counts_at_word_edges(n, enc, dim):
    sim = SIM.EUCLIDEAN
    rows = synth(n, dim, 300 + n, enc)
    q = synth(1, dim, 301, enc)[0]
    r = LU.GpuFlatVectorsReader("v", rows, sim, enc)
    try:
        scored = all_scores(("edge", enc, n), rows, q, sim)
        ms = np.array([NEG_INF, jth_best(scored, (n + 1) // 2), jth_best(scored, 1), jth_best(scored, n)], np.float32)
        for m in ms:
            d, s, c, t, v = r.search_threshold(q, m, None, 80)
            assert_hits((d[0], s[0], c[0], t[0]), reference(scored, m), 80, (n, m))
            assert v[0] == n
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# a view of 3 segments in 2 shards (sparse ord_to_doc, non-zero doc bases): the three entries agree,
# batches, the counter, and the k-NN neighbours
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def view3():
    dim, sim = 128, SIM.COSINE
    sizes = [5000, 1, 9000]
    rows = [synth(n, dim, 400 + i) for i, n in enumerate(sizes)]
    o2d = [None, None, np.sort(np.random.default_rng(5).choice(20000, sizes[2], replace=False)).astype(np.int32)]
    max_doc = [5000, 1, 20000]
    bases = [3, 5003 + 10, 17]                   # shard 0: segments 0, 1; shard 1: segment 2
    readers = [LU.GpuFlatVectorsReader("v", rows[i], sim, F32, ord_to_doc=o2d[i], max_doc=max_doc[i]) for i in range(3)]
    leaves = [[LU.LeafReaderContext(0, bases[0], readers[0]), LU.LeafReaderContext(1, bases[1], readers[1])],
              [LU.LeafReaderContext(0, bases[2], readers[2])]]
    ds = LU.DeviceShardSet(leaves, [0, 1])
    queries = synth(6, dim, 450)
    yield dict(dim=dim, sim=sim, rows=rows, o2d=o2d, max_doc=max_doc, bases=bases, readers=readers, leaves=leaves,
               ds=ds, queries=queries, shard_of=[0, 0, 1])
    ds.close()
    for r in readers:
        r.close()


def view_reference(v, qi, min_score, accept=None):
    """Per shard (docs, scores) in shard-local doc order + visited per segment."""
    per_shard, visited = [[], []], []
    for i in range(3):
        acc = None if accept is None else accept[i]
        akey = None if acc is None else acc.tobytes()
        scored = all_scores(("view3", i, qi, akey), v["rows"][i], v["queries"][qi], v["sim"], v["o2d"][i], acc)
        d, s, vis = reference(scored, min_score, v["bases"][i])
        per_shard[v["shard_of"][i]].append((d, s))
        visited.append(vis)
    return [(np.concatenate([p[0] for p in ps]), np.concatenate([p[1] for p in ps])) for ps in per_shard], visited


def view3_threshold(v, qi, j):
    """The j-th best score over the whole view for query qi."""
    s = np.concatenate([all_scores(("view3", i, qi, None), v["rows"][i], v["queries"][qi], v["sim"], v["o2d"][i])[1]
                        for i in range(3)])
    return np.sort(s)[::-1][j - 1]


def device_call(v, q, ms, cap):
    import torch
    ds = v["ds"]
    nq, S = len(q), ds.n_shards
    tq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    tms = torch.from_numpy(np.ascontiguousarray(ms, np.float32)).cuda()
    docs = torch.full((nq, S, cap), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((nq, S, cap), -7.0, dtype=torch.float32, device="cuda")
    count = torch.full((nq, S), -7, dtype=torch.int32, device="cuda")
    total = torch.full((nq, S), -7, dtype=torch.int64, device="cuda")
    visited = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        _lib.check(_lib.lib().osk_view_search_threshold_device(
            ds.handle, tq.data_ptr(), nq, tms.data_ptr(), None, cap,
            docs.data_ptr(), scores.data_ptr(), count.data_ptr(), total.data_ptr(), visited.data_ptr(), st.cuda_stream))
    st.synchronize()
    return docs.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy(), total.cpu().numpy(), visited.cpu().numpy()


def test_view_entries_agree(view3):
    v = view3
    cap = 600
    for qi, j in [(0, 500), (1, 10)]:
        m = view3_threshold(v, qi, j)
        want, visited = view_reference(v, qi, m)
        assert sum(len(w[0]) for w in want) >= j
        d, s, c, t = v["ds"].search_threshold(v["queries"][qi], m, None, cap)
        dd, sd, cd, td, vd = device_call(v, v["queries"][qi:qi + 1], [m], cap)
        for sh in range(2):
            assert_hits((d[0, sh], s[0, sh], c[0, sh], t[0, sh]), want[sh], cap, ("host", qi, sh))
            assert_hits((dd[0, sh], sd[0, sh], cd[0, sh], td[0, sh]), want[sh], cap, ("device", qi, sh))
        assert list(vd) == visited == [5000, 1, 9000]
        # the per-segment entry: segment-local docs
        for i in range(3):
            scored = all_scores(("view3", i, qi, None), v["rows"][i], v["queries"][qi], v["sim"], v["o2d"][i])
            ds_, ss, cs, ts, vs = v["readers"][i].search_threshold(v["queries"][qi], m, None, cap)
            assert_hits((ds_[0], ss[0], cs[0], ts[0]), reference(scored, m), cap, ("seg", qi, i))
            assert vs[0] == len(v["rows"][i])


@pytest.mark.parametrize("nq", [1, 5])
def test_batches_equal_single_queries(view3, nq):
    v = view3
    cap = 256
    ms = np.array([view3_threshold(v, qi, j) for qi, j in zip(range(nq), [40, 1, 200, 10, 3])][:nq], np.float32)
    d, s, c, t = v["ds"].search_threshold(v["queries"][:nq], ms, None, cap)
    for qi in range(nq):
        want, _ = view_reference(v, qi, ms[qi])
        d1, s1, c1, t1 = v["ds"].search_threshold(v["queries"][qi], ms[qi], None, cap)
        for sh in range(2):
            assert_hits((d[qi, sh], s[qi, sh], c[qi, sh], t[qi, sh]), want[sh], cap, ("batch", qi, sh))
            assert_hits((d1[0, sh], s1[0, sh], c1[0, sh], t1[0, sh]), want[sh], cap, ("single", qi, sh))


def test_counter_and_neighbours_undisturbed(view3):
    v = view3
    ds = v["ds"]
    before = ds.search(v["queries"][:3], 10, 0, 10)
    c0 = ds.counter("threshold_calls")
    ds.search_threshold(v["queries"][0], view3_threshold(v, 0, 10), None, 32)
    ds.search_threshold(v["queries"][:5], 0.0, None, 8)
    assert ds.counter("threshold_calls") - c0 == 2
    after = ds.search(v["queries"][:3], 10, 0, 10)
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    want, _ = view_reference(v, 0, view3_threshold(v, 0, 10))
    d, s, c, t = ds.search_threshold(v["queries"][0], view3_threshold(v, 0, 10), None, 32)
    for sh in range(2):
        assert_hits((d[0, sh], s[0, sh], c[0, sh], t[0, sh]), want[sh], 32)


# ------------------------------------------------------------------------------------------------
# ties, NaN scores
# ------------------------------------------------------------------------------------------------
def test_ties_all_copies_in_doc_order():
    dim, sim = 96, SIM.DOT_PRODUCT
    base = synth(300, dim, 500)
    rows = np.ascontiguousarray(np.tile(base, (4, 1)))          # row i, i + 300, i + 600, i + 900 are equal
    q = synth(1, dim, 501)[0]
    r = LU.GpuFlatVectorsReader("v", rows, sim)
    try:
        scored = all_scores(("ties",), rows, q, sim)
        m = jth_best(scored, 20)                                 # a tied score (ranks 17..20)
        want = reference(scored, m)
        at = want[0][want[1] == m]
        assert len(at) == 4 and len(set(at % 300)) == 1 and len(want[0]) == 20
        d, s, c, t, _ = r.search_threshold(q, m, None, 64)
        assert_hits((d[0], s[0], c[0], t[0]), want, 64)
        assert np.all(np.diff(d[0, :c[0]]) > 0)
    finally:
        r.close()


@pytest.mark.parametrize("enc,dim", [(F32, 96), (BYTE, 100)], ids=["f32", "byte"])
def test_nan_scores_are_never_hits(enc, dim):
    rows = synth(1000, dim, 600, enc)
    rows[::7] = 0                                                # zero rows: NaN under COSINE
    r = LU.GpuFlatVectorsReader("v", rows, SIM.COSINE, enc)
    try:
        zero = np.zeros(dim, rows.dtype)
        d, s, c, t, v = r.search_threshold(zero, NEG_INF, None, 16)
        assert t[0] == 0 and c[0] == 0 and v[0] == 1000
        assert np.all(d[0] == INT32_MAX) and np.all(np.isneginf(s[0]))
        q = synth(1, dim, 601, enc)[0]
        scored = all_scores(("nan", enc), rows, q, SIM.COSINE)
        assert len(scored[0]) == 1000 - len(rows[::7])
        d, s, c, t, v = r.search_threshold(q, NEG_INF, None, 1000)
        assert_hits((d[0], s[0], c[0], t[0]), reference(scored, NEG_INF), 1000)
        assert v[0] == 1000 and not np.isnan(s[0, :c[0]]).any()
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# filters: ≈ 1 % and 50 %, dense (the compacted walk) and sparse-doc segments, through the segment entry and
# through a view of the leaves; and a view's mixed accept table — a leaf without a bitset between two with one,
# at the smallest shape that can go wrong: 130, 64 and 1 rows, the first leaf's 200 docs no multiple of 64
# ------------------------------------------------------------------------------------------------
# a case: dim, similarity and, per leaf, (rows, max_doc when its docs are sparse, accepted % of its docs or None
# for a leaf without a bitset)
FILTERED = [pytest.param(96, SIM.EUCLIDEAN, [(4097, 3 * 4097 if sparse else None, pct)], id=f"{pct}-{name}")
            for name, sparse in (("dense", False), ("sparse", True)) for pct in (1, 50)]
FILTERED.append(pytest.param(8, SIM.COSINE, [(130, 200, 50), (64, None, None), (1, None, 100)], id="mixed-view"))


@pytest.mark.parametrize("dim,sim,leaves", FILTERED)
def test_filtered(dim, sim, leaves):
    q = synth(1, dim, 701)[0]
    rows, o2d, acc, bases, readers = [], [], [], [], []
    ds = None
    try:
        for i, (n, sparse_max_doc, pct) in enumerate(leaves):
            rng = np.random.default_rng(pct or 0)
            max_doc = sparse_max_doc or n
            rows.append(synth(n, dim, 700 + i))
            o2d.append(np.sort(rng.choice(max_doc, n, replace=False)).astype(np.int32) if sparse_max_doc else None)
            acc.append(None if pct is None else rng.random(max_doc) < pct / 100)
            bases.append(sum(r.max_doc for r in readers))
            readers.append(LU.GpuFlatVectorsReader("v", rows[i], sim, F32, ord_to_doc=o2d[i], max_doc=max_doc))
        ds = LU.DeviceShardSet([[LU.LeafReaderContext(i, bases[i], r) for i, r in enumerate(readers)]], [0])
        scored = [all_scores(("filt", dim, i) + leaves[i], rows[i], q, sim, o2d[i], acc[i]) for i in range(len(leaves))]
        n_acc = [len(rows[i]) if acc[i] is None else int((acc[i] if o2d[i] is None else acc[i][o2d[i]]).sum())
                 for i in range(len(leaves))]
        assert all(scored[i][2] == n_acc[i] > 0 for i in range(len(leaves)))
        whole = (None, np.concatenate([s[1] for s in scored]))
        cap = sum(len(r) for r in rows)
        for m in (NEG_INF, jth_best(whole, 5), jth_best(whole, max(1, sum(n_acc) // 2))):
            for i, r in enumerate(readers):
                bits = None if acc[i] is None else LU.bits_from_bool(acc[i])
                d, s, c, t, v = r.search_threshold(q, m, bits, cap)
                assert_hits((d[0], s[0], c[0], t[0]), reference(scored[i], m), cap, (leaves[i], m))
                assert v[0] == n_acc[i]
            want = [reference(scored[i], m, bases[i]) for i in range(len(leaves))]
            d, s, c, t = ds.search_threshold(q, m, acc, cap)
            assert_hits((d[0, 0], s[0, 0], c[0, 0], t[0, 0]),
                        (np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])), cap, ("view", m))
    finally:
        if ds is not None:
            ds.close()
        for r in readers:
            r.close()


# ------------------------------------------------------------------------------------------------
# capacity: the first cap hits in doc order, the exact total, nothing written past cap
# ------------------------------------------------------------------------------------------------
def test_capacity():
    dim, sim, n = 96, SIM.COSINE, 4097
    rows = synth(n, dim, 800)
    q = synth(1, dim, 801)[0]
    r = LU.GpuFlatVectorsReader("v", rows, sim)
    try:
        scored = all_scores(("cap",), rows, q, sim)
        m = np.array([jth_best(scored, 500)], np.float32)
        want = reference(scored, m[0])
        total = len(want[0])
        assert total >= 500
        for cap in (7, total):
            guard = 16
            docs = np.full(cap + guard, -7, np.int32)
            scores = np.full(cap + guard, -7, np.float32)
            count, tot, vis = np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.int64)
            qq = np.ascontiguousarray(q[None])
            _lib.check(_lib.lib().osk_seg_search_threshold(r.handle, qq.ctypes.data, 1, m.ctypes.data, None, cap,
                                                           docs.ctypes.data, scores.ctypes.data, count.ctypes.data,
                                                           tot.ctypes.data, vis.ctypes.data))
            assert count[0] == cap and tot[0] == total and vis[0] == n
            assert np.array_equal(docs[:cap], want[0][:cap])
            assert np.array_equal(scores[:cap].view(np.uint32), want[1][:cap].view(np.uint32))
            assert np.all(docs[cap:] == -7) and np.all(scores[cap:] == -7)      # the guard values
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# the Python query classes and the shard's query phase
# ------------------------------------------------------------------------------------------------
def test_query_classes(view3):
    v = view3
    leaves = v["leaves"][0]                      # shard 0: a 5000-row leaf and a 1-row leaf
    rng = np.random.default_rng(9)
    live = [rng.random(5000) < 0.9, None]
    for lf, l in zip(leaves, live):
        lf.live_docs = l
    try:
        flt = lambda leaf: (np.arange(leaf.max_doc) % 2 == 0) if leaf.max_doc > 1 else np.ones(1, bool)   # noqa: E731
        q = v["queries"][2]
        accept = [live[0] & flt(leaves[0]), flt(leaves[1])]
        scored = [all_scores(("qc", i), v["rows"][i], q, v["sim"], None, accept[i]) for i in range(2)]
        m = float(np.sort(np.concatenate([s[1] for s in scored]))[::-1][39])
        want_d = np.concatenate([reference(scored[i], m, v["bases"][i])[0] for i in range(2)])
        want_s = np.concatenate([reference(scored[i], m, v["bases"][i])[1] for i in range(2)])
        assert len(want_d) >= 40
        per_leaf = LU.FloatVectorSimilarityQuery("v", q, m, m, flt)
        gpu = LU.GpuFloatVectorSimilarityQuery("v", q, m, m, flt)
        per_leaf.DEFAULT_CAP = gpu.DEFAULT_CAP = 16     # below the total: both call again with cap = total
        a, b = per_leaf.rewrite(leaves), gpu.rewrite(leaves)
        for td in (a, b):
            assert td.total_hits.value == len(want_d)
            assert [h.doc for h in td.score_docs] == want_d.tolist()
            assert np.array_equal(np.array([h.score for h in td.score_docs], np.float32).view(np.uint32),
                                  want_s.view(np.uint32))
        # the shard's query phase: score desc, doc asc, cut to from+size; totalHits = every match
        order = np.lexsort((want_d, -want_s.astype(np.float64)))
        for query in (per_leaf, gpu):
            td = LU.shard_query_phase(query, leaves, 5, 10)
            assert td.total_hits.value == len(want_d) and td.total_hits.relation == LU.Relation.EQUAL_TO
            assert [h.doc for h in td.score_docs] == want_d[order][:15].tolist()
            assert td.score_docs[0].score == float(want_s.max())
        # through the DSL: min_score in place of k
        ctx = Q.QueryShardContext({"v": Q.parse_knn_vector_mapping(
            "v", {"type": "knn_vector", "dimension": v["dim"], "space_type": "cosinesimil"})})
        built = Q.KnnQueryBuilder("v", q.tolist(), min_score=m).do_to_query(ctx)
        assert isinstance(built, LU.FloatVectorSimilarityQuery)
        unfiltered = [all_scores(("qc-live", i), v["rows"][i], q, v["sim"], None, live[i]) for i in range(2)]
        n_live = sum(len(reference(unfiltered[i], np.float32(m))[0]) for i in range(2))
        assert LU.shard_query_phase(built, leaves, 0, 10).total_hits.value == n_live
    finally:
        for lf in leaves:
            lf.live_docs = None
        LU._GpuKnnVectorQuery.release_views()


def test_threshold_at_the_10th_best_equals_knn(view3):
    v = view3
    leaves = v["leaves"][1]                      # shard 1: the sparse-doc leaf
    q = v["queries"][3]
    scored = all_scores(("view3", 2, 3, None), v["rows"][2], q, v["sim"], v["o2d"][2])
    top = np.sort(scored[1])[::-1][:11]
    assert len(np.unique(top)) == 11             # distinct scores around the cut
    try:
        knn = LU.shard_query_phase(LU.GpuKnnFloatVectorQuery("v", q, 10), leaves, 0, 10)
        sim = LU.shard_query_phase(LU.GpuFloatVectorSimilarityQuery("v", q, float(top[9]), float(top[9])), leaves, 0, 10)
        assert sim.total_hits.value == 10
        assert [(h.doc, h.score) for h in sim.score_docs] == [(h.doc, h.score) for h in knn.score_docs]
    finally:
        LU._GpuKnnVectorQuery.release_views()


def test_byte_query_class():
    dim, n = 100, 2000
    rows = synth(n, dim, 900, BYTE)
    q = synth(1, dim, 901, BYTE)[0]
    r = LU.GpuFlatVectorsReader("v", rows, SIM.DOT_PRODUCT, BYTE)
    try:
        leaves = [LU.LeafReaderContext(0, 0, r)]
        scored = all_scores(("byteq",), rows, q, SIM.DOT_PRODUCT)
        m = float(jth_best(scored, 25))
        want = reference(scored, np.float32(m))
        for cls in (LU.ByteVectorSimilarityQuery, LU.GpuByteVectorSimilarityQuery):
            td = cls("v", q, m, m).rewrite(leaves)
            assert td.total_hits.value == len(want[0]) and [h.doc for h in td.score_docs] == want[0].tolist()
    finally:
        LU._GpuKnnVectorQuery.release_views()
        r.close()
