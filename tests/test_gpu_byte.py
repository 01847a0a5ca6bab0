"""Byte-vector search (VectorEncoding.BYTE) on the device, to the standard of the float paths: scan_i8 in every
lane config × batch width (query fragments in registers and in LDS, multi-launch batches), scan_i8_stream,
sel_keys_i8 (k > 64), thr_scan_i8 and nest_scan_i8, filtered and unfiltered, on segments and on views.

The bar, everywhere: docs equal, score bits equal, count equal, visited equal, unused slots −inf / INT32_MAX —
against `O.exact_search(..., ORDER_DEVICE)` AND against the independent numpy restatement
`oracle/byte_reference.py` (`reference()` below asserts the two agree before it returns either).  Byte sums are
exact int32, so there is no tolerance anywhere.  Views are checked per shard, then through `O.topdocs_merge`.

Every corpus carries the edge set E (byte_reference.edge_rows: all −128, all 127, alternating −128/127, all 0 —
NaN under COSINE: visited, never a hit —, a duplicate of row 0, all 1) at rows 0–5, from the middle on and at the
end; the queries include all −128, all 127, all 0 and alternating 127/−128.

Lane configs (units = ⌈dim/16⌉, cfg_index in osk_kernels.hip) and the batch widths NQ whose query fragments are
read from LDS (NQ·V·4 > 64):
    dims ≤128 (4,2) none | 129–256 (8,2) none | 257–512 (8,4) 8 | 513–1024 (16,4) 8 | 1025–2048 (16,8) 4, 8 |
    2049–3072 (16,12) 2, 4, 8 | 3073–4096 (32,8) 4, 8
"""
import numpy as np
import pytest

from opensearch_amd import _lib, lucene as LU
from oracle import byte_reference as BR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIM = LU.VectorSimilarityFunction
BYTE = LU.VectorEncoding.BYTE
SIMS = list(SIM)
EUC, DOT, COS, MIP = SIM.EUCLIDEAN, SIM.DOT_PRODUCT, SIM.COSINE, SIM.MAXIMUM_INNER_PRODUCT
INT32_MAX = 2**31 - 1
NEG_INF = np.float32(-np.inf)

_corpora: dict = {}      # key → (rows, queries), read-only
_scores: dict = {}       # (corpus key, query index, sim) → byte_reference scores of every row, read-only


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def sim_id(v):
    return getattr(v, "name", str(v))


def corpus(key, n, dim, nq, seed):
    """DIST_INT8 rows with E injected and nq queries with the edge queries among them; built once per key."""
    if key not in _corpora:
        rows = BR.inject_edges(O.synth(0, n, dim, seed, _lib.DIST_INT8))
        queries = BR.edge_queries(O.synth(0, nq, dim, seed + 1, _lib.DIST_INT8))
        rows.setflags(write=False)
        queries.setflags(write=False)
        _corpora[key] = (rows, queries)
    return _corpora[key]


def ref_scores(ckey, rows, qi, q, sim):
    key = (ckey, qi, int(sim))
    if key not in _scores:
        s = BR.scores(rows, q, int(sim))
        s.setflags(write=False)
        _scores[key] = s
    return _scores[key]


def reference(ckey, rows, qi, q, k, sim, o2d=None, accept=None):
    """One leaf's exact top k → (scores, docs, visited): the oracle's, after it is found equal to byte_reference's
    (docs, score bits, visited)."""
    ab = None if accept is None else O.bits_from_bool(accept)
    os_, od, ov = O.exact_search(rows, q, k, int(sim), O.ORDER_DEVICE, ord_to_doc=o2d, accept_bits=ab)
    rs, rd, rv = BR.top_k_of(ref_scores(ckey, rows, qi, q, sim), k, o2d, accept)
    assert ov == rv, (ckey, qi, ov, rv)
    assert np.array_equal(od, rd), (ckey, qi)
    assert np.array_equal(bits(os_), bits(rs)), (ckey, qi)
    return os_, od, ov


def assert_hits(s, d, c, want, k, ctx=""):
    ws, wd = want[0], want[1]
    n = len(wd)
    assert int(c) == n, (ctx, int(c), n)
    assert np.array_equal(d[:n], wd), (ctx, d[:n][:8], wd[:8])
    assert np.array_equal(bits(s[:n]), bits(ws)), ctx
    assert np.all(np.isneginf(s[n:k])) and np.all(d[n:k] == INT32_MAX), ctx


def check_segment(r, ckey, rows, queries, qidx, k, sim, o2d=None, accept=None, got=None):
    """The segment entry for queries[qidx] in one call against the reference; → what the device returned."""
    ab = None if accept is None else LU.bits_from_bool(accept)
    s, d, c, v = got if got is not None else r.search_batch(queries[qidx], k, ab)
    for j, qi in enumerate(qidx):
        want = reference(ckey, rows, qi, queries[qi], k, sim, o2d, accept)
        assert_hits(s[j], d[j], c[j], want, k, (ckey, sim_id(sim), k, qi))
        assert v[j] == want[2], (ckey, qi, v[j], want[2])
    return s, d, c, v


# ------------------------------------------------------------------------------------------------
# (a) batch widths × lane configs: one reader per case; batches of 2, 3, 5, 8, 9 and 17 queries run
# NQ = 2, 4, 8, 8, 8+1 and 8+8+1 (q0 > 0 in scan_i8; the 9th query alone on scan_i8_stream, or under a filter on
# scan_i8<·,·,1>, with q0 = 8).  Every batched result equals the same query searched alone, bit for bit.
# ------------------------------------------------------------------------------------------------
A_DIMS = [100, 250, 300, 1000, 1100, 3000, 4096]
BATCHES = (2, 3, 5, 8, 9, 17)


def run_batch_widths(dim, sim, filtered):
    n = 3000 + dim % 13
    ckey = ("a", dim)
    rows, queries = corpus(ckey, n, dim, 17, 2100 + dim)
    accept = None
    if filtered:
        accept = np.random.default_rng(dim).random(n) < 0.5
        accept[:6] = True                                    # E stays in
    ab = None if accept is None else LU.bits_from_bool(accept)
    r = LU.GpuFlatVectorsReader("v", rows, sim, BYTE)
    try:
        for k in (10, 64):
            alone = []
            for qi in range(17):
                s, d, c, v = check_segment(r, ckey, rows, queries, [qi], k, sim, None, accept)
                alone.append((s[0].copy(), d[0].copy(), int(c[0]), int(v[0])))
            for nq in BATCHES:
                s, d, c, v = check_segment(r, ckey, rows, queries, list(range(nq)), k, sim, None, accept)
                for qi in range(nq):
                    a = alone[qi]
                    assert np.array_equal(bits(s[qi]), bits(a[0])) and np.array_equal(d[qi], a[1]), (nq, qi)
                    assert (int(c[qi]), int(v[qi])) == a[2:], (nq, qi)
            assert ab is None or alone[0][3] == int(accept.sum())
    finally:
        r.close()


@pytest.mark.parametrize("dim", A_DIMS)
@pytest.mark.parametrize("sim", SIMS, ids=sim_id)
def test_batch_widths_and_lane_configs(dim, sim):
    run_batch_widths(dim, sim, False)


@pytest.mark.parametrize("dim", [300, 1100, 3000])
@pytest.mark.parametrize("sim", SIMS, ids=sim_id)
def test_batch_widths_filtered(dim, sim):
    run_batch_widths(dim, sim, True)


# ------------------------------------------------------------------------------------------------
# (b) filters on one segment: nothing accepted, exactly one row, 7 rows (fewer than k, one of them a zero row),
# 1 %, 50 % and an all-ones bitset; dense (the compacted walk) and sparse (max_doc 20000)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("dim", [100, 1100])
@pytest.mark.parametrize("sim", [EUC, COS], ids=sim_id)
def test_filters_on_one_segment(dim, sim, sparse):
    n, k = 6000, 10
    ckey = ("b", dim)
    rows, queries = corpus(ckey, n, dim, 5, 2300 + dim)
    rng = np.random.default_rng(dim + sparse)
    max_doc = 20000 if sparse else n
    o2d = np.sort(rng.choice(max_doc, n, replace=False)).astype(np.int32) if sparse else None
    doc_of = o2d if sparse else np.arange(n)
    stray = np.setdiff1d(np.arange(max_doc), doc_of)[:50]     # docs without a vector: accepting them changes nothing

    def mask(row_idx):
        m = np.zeros(max_doc, bool)
        m[doc_of[np.asarray(row_idx, int)]] = True
        m[stray] = True
        return m

    levels = {
        "none": mask([]),
        "one": mask([int(rng.integers(6, n))]),
        "seven": mask([3] + list(rng.choice(np.arange(6, n), 6, replace=False))),     # row 3 is E's zero row
        "1pct": mask(np.flatnonzero(rng.random(n) < 0.01)),
        "50pct": mask(np.flatnonzero(rng.random(n) < 0.5)),
        "all": np.ones(max_doc, bool),
    }
    r = LU.GpuFlatVectorsReader("v", rows, sim, BYTE, ord_to_doc=o2d, max_doc=max_doc)
    try:
        for name, acc in levels.items():
            n_acc = int(acc[doc_of].sum())
            for qidx in ([2], [0, 1, 2, 3, 4]):
                s, d, c, v = check_segment(r, ckey, rows, queries, qidx, k, sim, o2d, acc)
                assert np.all(v == n_acc), (name, v, n_acc)
                assert np.all(c <= min(k, n_acc))
            if name == "none":
                assert np.all(c == 0)
            if name == "seven":
                assert n_acc == 7 and c[2] == (6 if sim == COS else 7)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# (c) views: 3 shards over 7 segments of 1, 63, 0, 64, 65, 4097 and 2500 rows, two of them sparse, non-zero doc
# bases.  The 0-row segment (a leaf where no doc has the field) is ordinary: osk_view_create gives it no tile,
# so no kernel ever sees it, and its accept bitset is copied but never read.
# ------------------------------------------------------------------------------------------------
VIEW_ROWS = [1, 63, 0, 64, 65, 4097, 2500]
VIEW_SHARD = [0, 0, 0, 0, 1, 1, 2]
VIEW_SPARSE = {1: 200, 5: 9000}          # segment → max_doc
VIEW_SHARD_INDEX = [2, 0, 1]


class ByteView:
    def __init__(self, dim, sim, nq=9):
        self.dim, self.sim = dim, sim
        self.ckeys, self.rows, self.o2d, self.max_doc, self.base, self.readers = [], [], [], [], [], []
        self.shard_leaves = [[], [], []]
        next_base = [5, 11, 17]
        rng = np.random.default_rng(dim)
        self.queries = corpus(("c-q", dim), 18, dim, nq, 2500 + dim)[1]
        for i, n in enumerate(VIEW_ROWS):
            if n >= 18:
                rows = corpus(("c", dim, i), n, dim, 0, 2400 + dim + i)[0]
            else:
                rows = BR.inject_edges(O.synth(0, n, dim, 2400 + dim + i, _lib.DIST_INT8)) if n else np.zeros((0, dim), np.int8)
            md = VIEW_SPARSE.get(i, 40 if n == 0 else n)
            o2d = np.sort(rng.choice(md, n, replace=False)).astype(np.int32) if i in VIEW_SPARSE else None
            rd = LU.GpuFlatVectorsReader("v", rows, sim, BYTE, ord_to_doc=o2d, max_doc=md)
            sh = VIEW_SHARD[i]
            self.shard_leaves[sh].append(LU.LeafReaderContext(len(self.shard_leaves[sh]), next_base[sh], rd))
            self.ckeys.append(("c", dim, i))
            self.rows.append(rows)
            self.o2d.append(o2d)
            self.max_doc.append(md)
            self.base.append(next_base[sh])
            self.readers.append(rd)
            next_base[sh] += md + 3
        self.ds = LU.DeviceShardSet(self.shard_leaves, VIEW_SHARD_INDEX)
        # an accept table that mixes None and bitsets (all-ones, random, and the 0-row leaf's)
        self.mixed = [np.ones(1, bool), None, rng.random(40) < 0.5, rng.random(64) < 0.5, None,
                      rng.random(9000) < 0.3, rng.random(2500) < 0.02]

    def close(self):
        self.ds.close()
        for r in self.readers:
            r.close()

    def leaf_ref(self, i, qi, k, accept):
        acc = None if accept is None else accept[i]
        return reference(self.ckeys[i], self.rows[i], qi, self.queries[qi], k, self.sim, self.o2d[i], acc)

    def shard_lists(self, qi, k, accept):
        """Each shard's top k: its leaves' hits with docBase added, [L] TopDocs.merge(k, perLeaf)."""
        out = []
        for sh in range(3):
            per_leaf = []
            for i in range(len(VIEW_ROWS)):
                if VIEW_SHARD[i] == sh:
                    s, d, _ = self.leaf_ref(i, qi, k, accept)
                    per_leaf.append((s, d + self.base[i]))
            ms, md, _, _, _ = O.topdocs_merge(per_leaf, 0, k, shard_index=[0] * len(per_leaf))
            out.append((ms, md))
        return out

    def check_search(self, qidx, k, from_, size, accept):
        s, d, sh, c, t, mx = self.ds.search(self.queries[qidx], k, from_, size, accept=accept)
        for j, qi in enumerate(qidx):
            lists = self.shard_lists(qi, k, accept)
            es, ed, esh, etot, emx = O.topdocs_merge(lists, from_, size, shard_index=VIEW_SHARD_INDEX)
            ctx = (self.dim, sim_id(self.sim), qi, k, from_, size)
            assert_hits(s[j], d[j], c[j], (es, ed), size, ctx)
            assert np.array_equal(sh[j, :len(ed)], esh) and np.all(sh[j, len(ed):] == -1), ctx
            assert t[j] == etot == sum(len(l[1]) for l in lists), ctx
            if etot:
                assert bits([mx[j]])[0] == bits([emx])[0] == bits([max(l[0][0] for l in lists if len(l[0]))])[0], ctx
            else:
                assert np.isnan(mx[j]), ctx

    def check_per_shard(self, qidx, k, accept):
        """from 0, size 3k: nothing is cut, so the hits carrying a shard's index are that shard's whole list."""
        s, d, sh, c, t, _ = self.ds.search(self.queries[qidx], k, 0, 3 * k, accept=accept)
        for j, qi in enumerate(qidx):
            lists = self.shard_lists(qi, k, accept)
            assert c[j] == t[j] == sum(len(l[1]) for l in lists)
            for shard, (ws, wd) in enumerate(lists):
                at = np.flatnonzero(sh[j, :c[j]] == VIEW_SHARD_INDEX[shard])
                assert np.array_equal(d[j, at], wd), (qi, shard)
                assert np.array_equal(bits(s[j, at]), bits(ws)), (qi, shard)


@pytest.fixture(scope="module", params=[DOT, EUC], ids=sim_id)
def view300(request):
    v = ByteView(300, request.param)
    yield v
    v.close()


@pytest.mark.parametrize("filtered", [False, True], ids=["unfiltered", "mixed-accept"])
def test_view_search(view300, filtered):
    v = view300
    accept = v.mixed if filtered else None
    v.check_per_shard([2], 10, accept)
    v.check_per_shard(list(range(9)), 10, accept)
    v.check_search([3], 10, 0, 10, accept)
    v.check_search(list(range(9)), 10, 3, 7, accept)
    v.check_search(list(range(5)), 64, 0, 64, accept)


@pytest.mark.parametrize("filtered", [False, True], ids=["unfiltered", "mixed-accept"])
def test_view_segment_entry_per_leaf(view300, filtered):
    v = view300
    for i, r in enumerate(v.readers):
        acc = v.mixed[i] if filtered else None
        for k, qidx in ((10, [0, 1, 2, 3, 4, 5, 6, 7, 8]), (64, [5])):
            s, d, c, vis = check_segment(r, v.ckeys[i], v.rows[i], v.queries, qidx, k, v.sim, v.o2d[i], acc)
            n_acc = VIEW_ROWS[i] if acc is None else int(acc[v.o2d[i] if v.o2d[i] is not None else np.arange(VIEW_ROWS[i])].sum())
            assert np.all(vis == n_acc), (i, vis, n_acc)
            assert np.all(c == min(k, n_acc))                   # DOT_PRODUCT / EUCLIDEAN: no NaN


def test_view_query_rewrite(view300):
    """GpuKnnByteVectorQuery.rewrite (one view call per shard) == KnnByteVectorQuery.rewrite (one reader call per
    leaf + TopDocs.merge) == the reference, with live docs on two leaves and a filter on all."""
    v = view300
    leaves = v.shard_leaves[1]                                  # 65 dense rows and 4097 sparse rows
    segs = [i for i in range(len(VIEW_ROWS)) if VIEW_SHARD[i] == 1]
    rng = np.random.default_rng(77)
    flt = lambda leaf: np.arange(leaf.max_doc) % 3 != 0          # noqa: E731
    live = [rng.random(lf.max_doc) < 0.8 for lf in leaves]
    try:
        for use_live, use_filter in ((False, False), (True, True)):
            for lf, l in zip(leaves, live):
                lf.live_docs = l if use_live else None
            accept = {i: ((live[j] & flt(leaves[j])) if use_live else None) for j, i in enumerate(segs)}
            for qi, k in ((0, 10), (6, 64)):
                q = v.queries[qi]
                per_leaf = []
                for i in segs:
                    s, d, _ = reference(v.ckeys[i], v.rows[i], qi, q, k, v.sim, v.o2d[i], accept[i])
                    per_leaf.append((s, d + v.base[i]))
                ws, wd, _, _, _ = O.topdocs_merge(per_leaf, 0, k, shard_index=[0] * len(per_leaf))
                f = flt if use_filter else None
                a = LU.KnnByteVectorQuery("v", q, k, f).rewrite(leaves)
                b = LU.GpuKnnByteVectorQuery("v", q, k, f).rewrite(leaves)
                for td in (a, b):
                    assert [h.doc for h in td.score_docs] == wd.tolist(), (qi, k)
                    assert np.array_equal(bits([h.score for h in td.score_docs]), bits(ws)), (qi, k)
                assert b.total_hits.value == len(wd)
    finally:
        for lf in leaves:
            lf.live_docs = None
        LU._GpuKnnVectorQuery.release_views()


# ------------------------------------------------------------------------------------------------
# (d) the select path (k > 64): one dim per sel_keys_i8 instantiation (sel_bounds_cfg of the row's 16-byte units:
# ≤4, ≤8, ≤16, ≤32, ≤48, ≤64, ≤128, ≤256), filtered and sparse and on a view
# ------------------------------------------------------------------------------------------------
D_DIMS = [40, 100, 250, 500, 768, 1000, 2000, 4096]
D_CASES = [(dim, sim) for dim in D_DIMS for sim in (SIMS if dim in (250, 2000) else (EUC, COS))]


def select_corpus(dim):
    return corpus(("d", dim), 6000 + dim % 13, dim, 2, 2600 + dim)


def check_select_view(ds, reader, ckey, rows, queries, k, sim, o2d=None, accept=None):
    """One single-segment view call (the counters) and the segment entry (visited) for both queries."""
    before = ds.counter("select_calls")
    s, d, sh, c, t, _ = ds.search(queries, k, 0, k, accept=None if accept is None else [accept])
    assert ds.counter("select_calls") == before + 1 and ds.counter("sq8_calls") == 0
    for qi in range(len(queries)):
        want = reference(ckey, rows, qi, queries[qi], k, sim, o2d, accept)
        assert_hits(s[qi], d[qi], c[qi], want, k, (ckey, sim_id(sim), k, qi))
        assert t[qi] == len(want[1])
    check_segment(reader, ckey, rows, queries, list(range(len(queries))), k, sim, o2d, accept)


@pytest.mark.parametrize("dim,sim", D_CASES, ids=sim_id)
def test_select_lane_configs(dim, sim):
    rows, queries = select_corpus(dim)
    r = LU.GpuFlatVectorsReader("v", rows, sim, BYTE)
    ds = LU.DeviceShardSet([[LU.LeafReaderContext(0, 0, r)]], [0])
    try:
        for k in (65, 100, 1000):
            check_select_view(ds, r, ("d", dim), rows, queries, k, sim)
    finally:
        ds.close()
        r.close()


@pytest.mark.parametrize("dim", [100, 2000])
@pytest.mark.parametrize("sim", [EUC, COS], ids=sim_id)
def test_select_filtered_sparse_and_beyond_rows(dim, sim):
    rows, queries = select_corpus(dim)
    n = len(rows)
    rng = np.random.default_rng(dim)
    max_doc = 15000
    o2d = np.sort(rng.choice(max_doc, n, replace=False)).astype(np.int32)
    dense = LU.GpuFlatVectorsReader("v", rows, sim, BYTE)
    sparse = LU.GpuFlatVectorsReader("v", rows, sim, BYTE, ord_to_doc=o2d, max_doc=max_doc)
    dv = LU.DeviceShardSet([[LU.LeafReaderContext(0, 0, dense)]], [0])
    sv = LU.DeviceShardSet([[LU.LeafReaderContext(0, 0, sparse)]], [0])
    try:
        for pct in (0.1, 5, 50):
            acc = rng.random(n) < pct / 100
            acc[:6] = True
            # 0.1 %: fewer accepted rows than k — the shard takes every one of them
            check_select_view(dv, dense, ("d", dim), rows, queries, 100, sim, None, acc)
        live = rng.random(max_doc) < 0.7
        check_select_view(sv, sparse, ("d", dim), rows, queries, 100, sim, o2d, live)
        check_select_view(sv, sparse, ("d", dim), rows, queries, 1000, sim, o2d, None)
        # k beyond the row count: every non-NaN row comes back, the rest of the k slots stay empty
        for ds, rd, od in ((dv, dense, None), (sv, sparse, o2d)):
            s, d, c, v = check_segment(rd, ("d", dim), rows, queries, [0, 1], _lib.OSK_MAX_K, sim, od)
            nan_rows = int((~rows.any(axis=1)).sum()) if sim == COS else 0
            assert nan_rows >= 3 or sim != COS
            assert np.all(c == n - nan_rows) and np.all(v == n)
        check_select_view(dv, dense, ("d", dim), rows, queries, n + 1, sim)
    finally:
        dv.close()
        sv.close()
        dense.close()
        sparse.close()


@pytest.mark.parametrize("dim", [100, 2000])
@pytest.mark.parametrize("sim", [EUC, COS], ids=sim_id)
def test_select_on_the_view(dim, sim):
    v = ByteView(dim, sim, nq=2)
    try:
        for accept in (None, v.mixed):
            before = v.ds.counter("select_calls")
            v.check_search([0, 1], 1000, 100, 900, accept)
            assert v.ds.counter("select_calls") == before + 1 and v.ds.counter("sq8_calls") == 0
        v.check_per_shard([1], 100, v.mixed)
    finally:
        v.close()


# ------------------------------------------------------------------------------------------------
# (e) ties: a dim-1 corpus of 5000 rows (at most 256 distinct scores) and a dim-64 corpus in which every row
# appears 3 times (adjacent copies, and copies a third of the corpus apart)
# ------------------------------------------------------------------------------------------------
def tie_corpus(kind):
    key = ("e", kind)
    if key not in _corpora:
        if kind == "dim1":
            rows = BR.inject_edges(O.synth(0, 5000, 1, 2700, _lib.DIST_INT8))
            queries = BR.edge_queries(O.synth(0, 5, 1, 2701, _lib.DIST_INT8))
            queries[2], queries[4] = 0, 3                     # −128, 127, 0 (COSINE: no hit at all), a random value, 3
        else:
            base = BR.inject_edges(O.synth(0, 1000, 64, 2710, _lib.DIST_INT8))
            rows = np.ascontiguousarray(np.concatenate([np.repeat(base[:500], 3, axis=0), np.tile(base[500:], (3, 1))]))
            queries = BR.edge_queries(O.synth(0, 5, 64, 2711, _lib.DIST_INT8))
            queries[2] = base[700]                            # equals three rows
            queries[3] = base[10]
        rows.setflags(write=False)
        queries.setflags(write=False)
        _corpora[key] = (rows, queries)
    return key, _corpora[key][0], _corpora[key][1]


TIE_KINDS = ["dim1", "dim64x3"]


@pytest.mark.parametrize("kind", TIE_KINDS)
@pytest.mark.parametrize("sim", SIMS, ids=sim_id)
def test_ties_knn_and_select(kind, sim):
    ckey, rows, queries = tie_corpus(kind)
    n = len(rows)
    acc = np.random.default_rng(5).random(n) < 0.5
    r = LU.GpuFlatVectorsReader("v", rows, sim, BYTE)
    try:
        for k in (10, 64, 100):
            for accept in (None, acc):
                s, d, c, _ = check_segment(r, ckey, rows, queries, [0, 1, 2, 3, 4], k, sim, None, accept)
                check_segment(r, ckey, rows, queries, [3], k, sim, None, accept)
                for j in range(5):                             # score desc, ties by doc asc
                    sj, dj = s[j, :c[j]], d[j, :c[j]]
                    assert np.all((sj[:-1] > sj[1:]) | ((sj[:-1] == sj[1:]) & (dj[:-1] < dj[1:])))
        s, d, c, _ = r.search_batch(queries[3:4], 64)
        assert len(np.unique(s[0, :c[0]])) < c[0]               # there are ties inside the list
    finally:
        r.close()


@pytest.mark.parametrize("kind", TIE_KINDS)
@pytest.mark.parametrize("sim", SIMS, ids=sim_id)
def test_ties_threshold_at_a_tied_score(kind, sim):
    """min_score equal to a score several rows share: every copy is a hit, in doc order, with the exact total."""
    ckey, rows, queries = tie_corpus(kind)
    n = len(rows)
    r = LU.GpuFlatVectorsReader("v", rows, sim, BYTE)
    try:
        for qi in (1, 3):
            q = queries[qi]
            s_all, d_all, vis = reference(ckey, rows, qi, q, n, sim)
            assert vis == n and len(s_all) >= 12
            m = s_all[11]                                      # the 12th best score
            tied = int((s_all == m).sum())
            assert tied >= 3
            keep = s_all >= m
            order = np.argsort(d_all[keep], kind="stable")
            wd, ws = d_all[keep][order], s_all[keep][order]
            assert len(wd) == int((s_all >= m).sum()) >= 12
            cap = n
            for batch in (q[None], np.repeat(q[None], 5, 0)):
                d, s, c, t, v = r.search_threshold(batch, m, None, cap)
                for j in range(len(batch)):
                    assert t[j] == c[j] == len(wd) and v[j] == n, (qi, j, t[j], len(wd))
                    assert np.array_equal(d[j, :c[j]], wd) and np.array_equal(bits(s[j, :c[j]]), bits(ws))
                    assert np.all(d[j, c[j]:] == INT32_MAX) and np.all(np.isneginf(s[j, c[j]:]))
                    assert int((s[j, :c[j]] == m).sum()) == tied
    finally:
        r.close()


@pytest.mark.parametrize("kind", TIE_KINDS)
@pytest.mark.parametrize("sim", SIMS, ids=sim_id)
def test_ties_nested_lowest_child_wins(kind, sim):
    """Families of 4 children followed by their parent doc: tied best children inside a family → the lowest child
    doc represents it; tied families → the lower child doc first."""
    ckey, rows, queries = tie_corpus(kind)
    n = len(rows)
    o2d = (np.arange(n) + np.arange(n) // 4).astype(np.int32)
    max_doc = int(o2d[-1]) + 2
    parents = np.append(np.arange(4, max_doc - 1, 5), max_doc - 1)
    parents = np.unique(parents[parents > 0])
    pm = np.zeros(max_doc, bool)
    pm[parents] = True
    assert not pm[o2d].any() and pm[max_doc - 1]
    r = LU.GpuFlatVectorsReader("v", rows, sim, BYTE, ord_to_doc=o2d, max_doc=max_doc)
    try:
        r.set_parents(pm)
        for k in (10, 64):
            s, d, c, v = r.search_nested(queries, k)
            s1, d1, c1, v1 = r.search_nested(queries[3], k)
            for qi in range(5):
                s_all, d_all, vis = reference(ckey, rows, qi, queries[qi], n, sim, o2d)
                pid = np.searchsorted(parents, d_all, side="left")
                # s_all / d_all are already (score desc, doc asc): a parent's first row there is its best child
                _, first = np.unique(pid, return_index=True)
                first.sort()
                wd, ws = d_all[first][:k], s_all[first][:k]
                assert_hits(s[qi], d[qi], c[qi], (ws, wd), k, (kind, sim_id(sim), k, qi))
                assert v[qi] == vis == n
                if qi == 3:
                    assert_hits(s1[0], d1[0], c1[0], (ws, wd), k)
                    best = s_all[0]
                    top_family = d_all[(s_all == best) & (pid == pid[0])]
                    assert len(wd) == 0 or wd[0] == top_family.min()
    finally:
        r.close()
