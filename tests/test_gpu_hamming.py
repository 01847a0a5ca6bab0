"""Binary vectors (OSK_BYTE / OSK_HAMMING) on the device, to test_gpu_byte.py's bar: docs equal, score bits equal,
count equal, visited equal, unused slots −inf / INT32_MAX, against the numpy restatement tests/hamming_reference.py
(itself held to the oracle by test_hamming_reference_cpu.py).  Distances are exact integers and the score is one
float division, so there is no tolerance anywhere.

Every corpus carries the edge set (hamming_reference.edge_rows: all 0x00, all 0xFF, alternating 0xAA/0x55 and a
duplicate of the first) at rows 0–3, from the middle on and at the end; the first four queries are all 0x00, all
0xFF, a copy of corpus row 7 (distance 0, score exactly 1.0) and its complement (distance 8·dim).

Lane configs of osk_hamming.hip (all three kernels), by bytes per vector:
    ≤16 (1,1) | ≤32 (2,1) | ≤64 (4,1) | ≤128 (8,1) | ≤256 (16,1) | ≤512 (16,2) | ≤768 (16,3) | ≤1024 (16,4) |
    ≤2048 (32,4) | ≤4096 (64,4);  scan_ham reads its query fragments from LDS at NQ = 8 with V ≥ 3 (> 512 bytes).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import hamming_reference as HR
from opensearch_amd import _lib, distributed as D, lucene as LU
from opensearch_amd._lib import lib
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HAM = LU.BinarySimilarity.HAMMING
INT32_MAX = 2**31 - 1

_corpora: dict = {}      # key → (rows uint8, queries uint8), read-only
_dist: dict = {}         # (corpus key, query index) → distances of every row, read-only


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def corpus(key, n, dim, nq, seed):
    if key not in _corpora:
        rows = HR.inject_edges(O.synth(0, n, dim, seed, _lib.DIST_INT8))
        queries = HR.edge_queries(O.synth(0, max(nq, 4), dim, seed + 1, _lib.DIST_INT8), rows)
        rows.setflags(write=False)
        queries.setflags(write=False)
        _corpora[key] = (rows, queries)
    return _corpora[key]


def reference(ckey, rows, qi, q, k, o2d=None, accept=None):
    """One leaf's exact top k → (scores, docs, visited); the distances of (corpus, query) are computed once."""
    if (ckey, qi) not in _dist:
        d = HR.distances(rows, q)
        d.setflags(write=False)
        _dist[(ckey, qi)] = d
    s, d, vis, _ = HR.top_k(rows, q, k, o2d, accept, _dist[(ckey, qi)])
    return s, d, vis


def assert_hits(s, d, c, want, k, ctx=""):
    ws, wd = want[0], want[1]
    n = len(wd)
    assert int(c) == n, (ctx, int(c), n)
    assert np.array_equal(d[:n], wd), (ctx, d[:n][:8], wd[:8])
    assert np.array_equal(bits(s[:n]), bits(ws)), ctx
    assert np.all(np.isneginf(s[n:k])) and np.all(d[n:k] == INT32_MAX), ctx
    assert not np.any(np.isnan(s[:n])) and np.all(s[:n] > 0) and np.all(s[:n] <= 1), ctx


def check_segment(r, ckey, rows, queries, qidx, k, o2d=None, accept=None):
    """The segment entry for queries[qidx] in one call against the reference; → what the device returned."""
    ab = None if accept is None else LU.bits_from_bool(accept)
    s, d, c, v = r.search_batch(queries[qidx], k, ab)
    for j, qi in enumerate(qidx):
        want = reference(ckey, rows, qi, queries[qi], k, o2d, accept)
        assert_hits(s[j], d[j], c[j], want, k, (ckey, k, qi))
        assert v[j] == want[2], (ckey, qi, v[j], want[2])
    return s, d, c, v


@pytest.fixture(params=[1, 0], ids=["scan_ham_stream", "scan_ham"])
def stream_knob(request):
    """One unfiltered query runs on scan_ham_stream (1) or, the knob off, on scan_ham<·,·,1> (0)."""
    _lib.tune("ham_stream", request.param)
    yield request.param
    _lib.tune("ham_stream", 1)


# ------------------------------------------------------------------------------------------------
# (a) lane configs: byte lengths on both sides of every boundary of the table, one query at a time
# ------------------------------------------------------------------------------------------------
LENGTHS = [1, 2, 8, 15, 16, 17, 32, 33, 64, 65, 96, 100, 128, 129, 256, 257, 512, 513, 768, 769, 1000, 1024, 1025,
           2048, 2049, 4096]


@pytest.mark.parametrize("dim", LENGTHS)
def test_lane_configs(dim, stream_knob):
    n = 3000 + dim % 13
    ckey = ("a", dim)
    rows, queries = corpus(ckey, n, dim, 6, 5100 + dim)
    r = LU.GpuBinaryVectorsReader("v", rows)
    try:
        assert (r.dim, r.size, r.encoding, r.similarity) == (dim, n, LU.VectorEncoding.BYTE, HAM)
        for k in (1, 10, 64):
            for qi in range(6):
                s, d, c, v = check_segment(r, ckey, rows, queries, [qi], k)
                assert v[0] == n and c[0] == k
                if qi == 2:                                        # the copy of row 7
                    assert s[0, 0] == np.float32(1.0)
                if qi == 3 and k == 64:                            # its complement: row 7 is the farthest of all
                    far = r.search_batch(queries[3], n)[0][0, n - 1]
                    assert far == np.float32(1.0) / np.float32(1 + 8 * dim)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# (b) batch widths 2, 3, 5, 8, 9 and 17 (NQ = 2, 4, 8, 8, 8+1, 8+8+1; q0 > 0), unfiltered and under a 50 % filter:
# every batched result equals the same query searched alone, bit for bit.  One length per lane config.
# ------------------------------------------------------------------------------------------------
B_LENGTHS = [16, 32, 50, 100, 200, 300, 700, 1000, 2000, 4096]
BATCHES = (2, 3, 5, 8, 9, 17)


@pytest.mark.parametrize("filtered", [False, True], ids=["unfiltered", "half"])
@pytest.mark.parametrize("dim", B_LENGTHS)
def test_batch_widths(dim, filtered):
    n = 3000 + dim % 13
    ckey = ("b", dim)
    rows, queries = corpus(ckey, n, dim, 17, 5300 + dim)
    accept = None
    if filtered:
        accept = np.random.default_rng(dim).random(n) < 0.5
        accept[:4] = True
    r = LU.GpuBinaryVectorsReader("v", rows)
    try:
        for k in (10, 64) if dim in (16, 700) else (10,):
            alone = []
            for qi in range(17):
                s, d, c, v = check_segment(r, ckey, rows, queries, [qi], k, None, accept)
                alone.append((s[0].copy(), d[0].copy(), int(c[0]), int(v[0])))
            for nq in BATCHES:
                s, d, c, v = check_segment(r, ckey, rows, queries, list(range(nq)), k, None, accept)
                for qi in range(nq):
                    a = alone[qi]
                    assert np.array_equal(bits(s[qi]), bits(a[0])) and np.array_equal(d[qi], a[1]), (nq, qi)
                    assert (int(c[qi]), int(v[qi])) == a[2:], (nq, qi)
            assert accept is None or alone[0][3] == int(accept.sum())
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# (c) ties: 1-byte and 2-byte corpora (9 and 17 distinct scores over 5000 rows: every cut falls inside a tie) and a
# corpus of one repeated vector (all rows tie: the order is purely by doc)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2])
def test_ties_narrow_corpora(dim, stream_knob):
    n = 5000
    ckey = ("c", dim)
    rows, queries = corpus(ckey, n, dim, 5, 5500 + dim)
    acc = np.random.default_rng(5).random(n) < 0.5
    r = LU.GpuBinaryVectorsReader("v", rows)
    try:
        for k in (10, 64, 100):
            for accept in (None, acc):
                s, d, c, _ = check_segment(r, ckey, rows, queries, [0, 1, 2, 3, 4], k, None, accept)
                for qi in range(5):
                    check_segment(r, ckey, rows, queries, [qi], k, None, accept)
                    sj, dj = s[qi, :c[qi]], d[qi, :c[qi]]
                    assert np.all((sj[:-1] > sj[1:]) | ((sj[:-1] == sj[1:]) & (dj[:-1] < dj[1:])))
                    assert len(np.unique(sj)) <= 8 * dim + 1
                    assert k < 64 or len(np.unique(sj)) < len(sj)     # ties inside the list
    finally:
        r.close()


@pytest.mark.parametrize("dim", [16, 100])
def test_ties_one_repeated_vector(dim, stream_knob):
    n = 5000
    one = O.synth(0, 1, dim, 5600 + dim, _lib.DIST_INT8).view(np.uint8)
    rows = np.ascontiguousarray(np.repeat(one, n, axis=0))
    queries = np.stack([one[0], ~one[0], np.zeros(dim, np.uint8)])
    r = LU.GpuBinaryVectorsReader("v", rows)
    try:
        for k in (10, 64, 100):
            for batch in ([0], [1], [0, 1, 2]):
                s, d, c, v = r.search_batch(queries[batch], k)
                for j, qi in enumerate(batch):
                    dist = int(np.unpackbits(one[0] ^ queries[qi]).sum())
                    assert c[j] == k and v[j] == n
                    assert np.array_equal(d[j], np.arange(k))          # purely by doc
                    assert np.all(bits(s[j]) == bits(HR.scores_of([dist]))[0])
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# (d) filters: dense with accept (walk_rows' compaction) at 1 % and 50 %, sparse ord_to_doc with and without
# accept, nothing accepted, exactly one row, fewer accepted rows than k
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("dim", [16, 32, 100, 1000])
def test_filters_on_one_segment(dim, sparse):
    n, k = 5000, 10
    ckey = ("d", dim)
    rows, queries = corpus(ckey, n, dim, 5, 5700 + dim)
    rng = np.random.default_rng(dim + sparse)
    max_doc = 17000 if sparse else n
    o2d = np.sort(rng.choice(max_doc, n, replace=False)).astype(np.int32) if sparse else None
    doc_of = o2d if sparse else np.arange(n)
    stray = np.setdiff1d(np.arange(max_doc), doc_of)[:50]     # docs without a vector: accepting them changes nothing

    def mask(row_idx):
        m = np.zeros(max_doc, bool)
        m[doc_of[np.asarray(row_idx, int)]] = True
        m[stray] = True
        return m

    levels = {
        "unfiltered": None,
        "none": mask([]),
        "one": mask([int(rng.integers(4, n))]),
        "seven": mask([1] + list(rng.choice(np.arange(4, n), 6, replace=False))),
        "1pct": mask(np.flatnonzero(rng.random(n) < 0.01)),
        "50pct": mask(np.flatnonzero(rng.random(n) < 0.5)),
        "all": np.ones(max_doc, bool),
    }
    r = LU.GpuBinaryVectorsReader("v", rows, ord_to_doc=o2d, max_doc=max_doc)
    try:
        for name, acc in levels.items():
            n_acc = n if acc is None else int(acc[doc_of].sum())
            for qidx in ([2], [0, 1, 2, 3, 4]):
                s, d, c, v = check_segment(r, ckey, rows, queries, qidx, k, o2d, acc)
                assert np.all(v == n_acc), (name, v, n_acc)
                assert np.all(c == min(k, n_acc)), (name, c)
            if name == "none":
                assert np.all(c == 0) and np.all(v == 0)
            if name == "seven":
                assert n_acc == 7
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# (e) large k through sel_keys_ham: 65, 1000 and 10000 (above n: count = n), filtered and not, one length per
# lane config
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 16, 32, 50, 100, 200, 300, 700, 1000, 2000, 4096])
def test_large_k_select_path(dim):
    n = 5000 + dim % 13
    ckey = ("e", dim)
    rows, queries = corpus(ckey, n, dim, 4, 5900 + dim)
    rng = np.random.default_rng(dim)
    max_doc = 12000
    o2d = np.sort(rng.choice(max_doc, n, replace=False)).astype(np.int32)
    half = rng.random(n) < 0.5
    few = np.zeros(n, bool)
    few[rng.choice(n, 40, replace=False)] = True                # fewer accepted rows than k
    dense = LU.GpuBinaryVectorsReader("v", rows)
    sparse = LU.GpuBinaryVectorsReader("v", rows, ord_to_doc=o2d, max_doc=max_doc)
    ds = LU.DeviceShardSet([[LU.LeafReaderContext(0, 0, dense)]], [0])
    try:
        for k in (65, 1000, _lib.OSK_MAX_K):
            before = ds.counter("select_calls")
            s, d, sh, c, t, _ = ds.search(queries[[2, 3]].view(np.int8), k, 0, k)
            assert ds.counter("select_calls") == before + 1
            for j, qi in enumerate((2, 3)):
                want = reference(ckey, rows, qi, queries[qi], k)
                assert_hits(s[j], d[j], c[j], want, k, (dim, k, qi))
                assert c[j] == t[j] == min(k, n)
            for accept in (None, half, few):
                s, d, c, v = check_segment(dense, ckey, rows, queries, [0, 1, 2, 3], k, None, accept)
                assert np.all(c == min(k, n if accept is None else int(accept.sum())))
        live = rng.random(max_doc) < 0.7
        check_segment(sparse, ckey, rows, queries, [1, 3], 1000, o2d, live)
        check_segment(sparse, ckey, rows, queries, [2], 100, o2d, None)
    finally:
        ds.close()
        dense.close()
        sparse.close()


# ------------------------------------------------------------------------------------------------
# (f) views: 3 shards × 2 segments with doc bases and a permuted shard_index — osk_view_search with from / size
# paging against O.topdocs_merge of the per-shard references, the device entry's keys decoded with
# osk_decode_keys, and a world-1 ShardSearchMerge
# ------------------------------------------------------------------------------------------------
VIEW_ROWS = [3000, 65, 4097, 1000, 2500, 3001]
VIEW_SPARSE = {2: 9000, 4: 4000}
VIEW_SHARD_INDEX = [2, 0, 1]


class HamView:
    def __init__(self, dim, nq=9):
        self.dim = dim
        self.ckeys, self.rows, self.o2d, self.base, self.readers = [], [], [], [], []
        self.shard_leaves = [[], [], []]
        next_base = [5, 11, 17]
        rng = np.random.default_rng(dim)
        self.queries = corpus(("f-q", dim), 64, dim, nq, 6100 + dim)[1]
        for i, n in enumerate(VIEW_ROWS):
            ckey = ("f", dim, i)
            rows = corpus(ckey, n, dim, 0, 6000 + dim + i)[0]
            md = VIEW_SPARSE.get(i, n)
            o2d = np.sort(rng.choice(md, n, replace=False)).astype(np.int32) if i in VIEW_SPARSE else None
            rd = LU.GpuBinaryVectorsReader("v", rows, ord_to_doc=o2d, max_doc=md)
            sh = i // 2
            self.shard_leaves[sh].append(LU.LeafReaderContext(len(self.shard_leaves[sh]), next_base[sh], rd))
            self.ckeys.append(ckey)
            self.rows.append(rows)
            self.o2d.append(o2d)
            self.base.append(next_base[sh])
            self.readers.append(rd)
            next_base[sh] += md + 3
        self.ds = LU.DeviceShardSet(self.shard_leaves, VIEW_SHARD_INDEX)
        self.mixed = [rng.random(3000) < 0.5, None, rng.random(9000) < 0.3, np.ones(1000, bool), rng.random(4000) < 0.02,
                      None]

    def close(self):
        self.ds.close()
        for r in self.readers:
            r.close()

    def shard_lists(self, qi, k, accept):
        """Each shard's top k: its leaves' hits with docBase added, [L] TopDocs.merge(k, perLeaf)."""
        out = []
        for sh in range(3):
            per_leaf = []
            for i in (2 * sh, 2 * sh + 1):
                acc = None if accept is None else accept[i]
                s, d, _ = reference(self.ckeys[i], self.rows[i], qi, self.queries[qi], k, self.o2d[i], acc)
                per_leaf.append((s, d + self.base[i]))
            ms, md, _, _, _ = O.topdocs_merge(per_leaf, 0, k, shard_index=[0, 0])
            out.append((ms, md))
        return out

    def check_search(self, qidx, k, from_, size, accept):
        s, d, sh, c, t, mx = self.ds.search(self.queries[qidx].view(np.int8), k, from_, size, accept=accept)
        for j, qi in enumerate(qidx):
            lists = self.shard_lists(qi, k, accept)
            es, ed, esh, etot, emx = O.topdocs_merge(lists, from_, size, shard_index=VIEW_SHARD_INDEX)
            ctx = (self.dim, qi, k, from_, size)
            n = len(ed)
            assert c[j] == n and np.array_equal(d[j, :n], ed) and np.array_equal(bits(s[j, :n]), bits(es)), ctx
            assert np.all(np.isneginf(s[j, n:])) and np.all(d[j, n:] == INT32_MAX), ctx
            assert np.array_equal(sh[j, :n], esh) and np.all(sh[j, n:] == -1), ctx
            assert t[j] == etot == sum(len(l[1]) for l in lists), ctx
            assert bits([mx[j]])[0] == bits([emx])[0], ctx


@pytest.fixture(scope="module", params=[16, 100], ids=["16B", "100B"])
def view(request):
    v = HamView(request.param)
    yield v
    v.close()


@pytest.mark.parametrize("filtered", [False, True], ids=["unfiltered", "mixed-accept"])
def test_view_search_and_paging(view, filtered):
    accept = view.mixed if filtered else None
    view.check_search([2], 10, 0, 10, accept)
    view.check_search(list(range(9)), 10, 3, 7, accept)
    view.check_search(list(range(5)), 64, 0, 64, accept)
    view.check_search([0, 3], 64, 50, 100, accept)
    view.check_search([1, 2], 1000, 100, 900, accept)             # the select path on a view


def test_view_device_entry_keys(view):
    v = view
    nq, k, S = 9, 10, 3
    q = torch.from_numpy(np.ascontiguousarray(v.queries[:nq]).view(np.int8).copy()).cuda()
    keys = torch.zeros((nq, S, k), dtype=torch.int64, device="cuda")
    cnt = torch.zeros((nq, S), dtype=torch.int32, device="cuda")
    vis = torch.zeros(len(VIEW_ROWS), dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    _lib.check(lib().osk_view_search_device(v.ds.handle, q.data_ptr(), nq, k, None, keys.data_ptr(), cnt.data_ptr(),
                                            vis.data_ptr(), st.cuda_stream))
    st.synchronize()
    s, d = LU.decode_keys(keys.cpu().numpy().view(np.uint64))
    cnt = cnt.cpu().numpy()
    assert vis.cpu().numpy().tolist() == VIEW_ROWS
    for qi in range(nq):
        for sh, (ws, wd) in enumerate(v.shard_lists(qi, k, None)):
            assert_hits(s[qi, sh], d[qi, sh], cnt[qi, sh], (ws, wd), k, (qi, sh))


def test_query_rewrite_routes(view):
    """KnnByteVectorQuery (one reader call per leaf + TopDocs.merge) == GpuKnnByteVectorQuery (one view call)."""
    v = view
    leaves = v.shard_leaves[1]
    try:
        for qi, k in ((2, 10), (5, 64)):
            q = v.queries[qi].view(np.int8)
            per_leaf = []
            for i in (2, 3):
                s, d, _ = reference(v.ckeys[i], v.rows[i], qi, v.queries[qi], k, v.o2d[i])
                per_leaf.append((s, d + v.base[i]))
            ws, wd, _, _, _ = O.topdocs_merge(per_leaf, 0, k, shard_index=[0, 0])
            for td in (LU.KnnByteVectorQuery("v", q, k).rewrite(leaves), LU.GpuKnnByteVectorQuery("v", q, k).rewrite(leaves)):
                assert [h.doc for h in td.score_docs] == wd.tolist(), (qi, k)
                assert np.array_equal(bits([h.score for h in td.score_docs]), bits(ws)), (qi, k)
    finally:
        LU._GpuKnnVectorQuery.release_views()


def test_shards_search_merge_world1(view):
    v = view
    nq, k, from_, size, spr = 3, 10, 2, 8, 4                     # spr 4 > 3 shards: the padded layout
    comm = D.DeviceComm.init_rank(0, 0, 1, D.DeviceComm.unique_id())
    try:
        step = D.ShardSearchMerge(comm, v.ds.handle, spr, nq, k, from_, size, device=0)
        st = torch.cuda.Stream()
        dq = torch.from_numpy(np.ascontiguousarray(v.queries[:nq]).view(np.int8).copy()).cuda()
        torch.cuda.synchronize()
        res = step(dq.data_ptr(), st.cuda_stream)
        st.synchronize()
        out = [t.cpu().numpy() for t in res]
        want = v.ds.search(v.queries[:nq].view(np.int8), k, from_, size)
        for w, g in zip(want, out):
            assert np.array_equal(bits(w), bits(g)) if w.dtype == np.float32 else np.array_equal(w, g)
        v.check_search(list(range(nq)), k, from_, size, None)
    finally:
        comm.close()


# ------------------------------------------------------------------------------------------------
# (g) the device cross-check: packed bits under HAMMING and the same bits expanded to 0/1 bytes under byte
# EUCLIDEAN (d² = the Hamming distance; the score's float operations are the same) give identical docs and bits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 16, 33, 100, 512])
def test_device_cross_check_against_byte_euclidean(dim):
    n = 3000
    rows, queries = corpus(("g", dim), n, dim, 6, 6300 + dim)
    acc = LU.bits_from_bool(np.random.default_rng(dim).random(n) < 0.3)
    ham = LU.GpuBinaryVectorsReader("v", rows)
    euc = LU.GpuFlatVectorsReader("v", HR.expand_bits(rows), LU.VectorSimilarityFunction.EUCLIDEAN, LU.VectorEncoding.BYTE)
    try:
        for k in (10, 100):
            for ab in (None, acc):
                a = ham.search_batch(queries, k, ab)
                b = euc.search_batch(HR.expand_bits(queries), k, ab)
                assert np.array_equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))
                assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    finally:
        ham.close()
        euc.close()


# ------------------------------------------------------------------------------------------------
# (h) size: 1M × 16 bytes generated on the device (full-size tiles), one query and a batch of 8
# ------------------------------------------------------------------------------------------------
def test_one_million_rows_synthetic():
    n, dim, seed, k = 1_000_000, 16, 6400, 10
    rows = O.synth(0, n, dim, seed, _lib.DIST_INT8).view(np.uint8)
    queries = HR.edge_queries(O.synth(0, 8, dim, seed + 1, _lib.DIST_INT8), rows)
    r = LU.GpuBinaryVectorsReader.synthetic("v", n, dim, seed=seed)
    try:
        assert (r.size, r.dim, r.similarity) == (n, dim, HAM)
        dist = [HR.distances(rows, q) for q in queries]
        for qidx in ([2], list(range(8))):
            s, d, c, v = r.search_batch(queries[qidx], k)
            for j, qi in enumerate(qidx):
                want = HR.top_k(rows, queries[qi], k, d=dist[qi])
                assert_hits(s[j], d[j], c[j], want, k, qi)
                assert v[j] == n
        s, d, c, v = r.search_batch(queries[2], 100)               # the select path over full-size tiles
        assert_hits(s[0], d[0], c[0], HR.top_k(rows, queries[2], 100, d=dist[2]), 100)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# (i) contract: the footprint, the refused entries, a failed call leaves the reader usable, padding
# ------------------------------------------------------------------------------------------------
def footprint(r):
    b = C.c_int64()
    _lib.check(lib().osk_seg_footprint(r.handle, C.byref(b)))
    return b.value


@pytest.mark.parametrize("dim,n", [(16, 4000), (100, 3001), (1, 5000)])
def test_footprint_has_no_norms(dim, n):
    rows = corpus(("i", dim, n), n, dim, 4, 6500 + dim)[0]
    ham = LU.GpuBinaryVectorsReader("v", rows)
    euc = LU.GpuFlatVectorsReader("v", rows.view(np.int8), LU.VectorSimilarityFunction.EUCLIDEAN, LU.VectorEncoding.BYTE)
    try:
        assert footprint(euc) - footprint(ham) == 4 * n
        assert footprint(ham) == n * ((dim + 15) // 16) * 16
        _lib.check(lib().osk_seg_warm(ham.handle, _lib.OSK_WARM_ALL))       # a no-op, as for byte fields
        assert footprint(ham) == n * ((dim + 15) // 16) * 16
    finally:
        ham.close()
        euc.close()


def test_threshold_and_nested_are_refused_and_the_reader_stays_usable():
    n, dim = 3000, 16
    ckey = ("i", dim, n, "r")
    rows, queries = corpus(ckey, n, dim, 4, 6600)
    r = LU.GpuBinaryVectorsReader("v", rows)
    ds = LU.DeviceShardSet([[LU.LeafReaderContext(0, 0, r)]], [0])
    try:
        pm = np.zeros(n, bool)
        r_parents = LU.GpuBinaryVectorsReader("v", rows[: n - 1], max_doc=n)
        pm[n - 1] = True
        r_parents.set_parents(pm)                                  # allowed: it does not look at the vectors
        assert r_parents.n_parents() == 1
        calls = [lambda: r.search_threshold(queries[:2], 0.5), lambda: r.search_nested(queries[:2], 10),
                 lambda: r_parents.search_nested(queries[:2], 10), lambda: ds.search_threshold(queries[:2], 0.5),
                 lambda: ds.search_nested(queries[:2], 10, 0, 10)]
        for call in calls:
            with pytest.raises(_lib.OskError) as e:
                call()
            assert e.value.code == _lib.OSK_ERR_UNSUPPORTED and "Hamming" in str(e.value), str(e.value)
            check_segment(r, ckey, rows, queries, [0, 1, 2, 3], 10)   # still usable
        r_parents.close()
        # the device entries refuse too, before touching their (null) buffers' contents
        one = torch.zeros(64, dtype=torch.int64, device="cuda")
        p = one.data_ptr()
        rc = lib().osk_view_search_threshold_device(ds.handle, p, 1, p, None, 8, p, p, p, p, None, None)
        assert rc == _lib.OSK_ERR_UNSUPPORTED and b"Hamming" in lib().osk_last_error()
        rc = lib().osk_view_search_nested_device(ds.handle, p, 1, 10, None, p, p, None, None)
        assert rc == _lib.OSK_ERR_UNSUPPORTED and b"Hamming" in lib().osk_last_error()
        # other failed calls: k out of range, a query of the wrong length
        with pytest.raises(_lib.OskError):
            r.search_batch(queries[:1], _lib.OSK_MAX_K + 1)
        with pytest.raises(ValueError):
            r.search_batch(np.zeros((1, dim + 1), np.int8), 10)
        check_segment(r, ckey, rows, queries, [0, 1, 2, 3], 64)
        s, d, sh, c, t, _ = ds.search(queries[:2].view(np.int8), 10, 0, 10)
        assert np.all(c == 10)
    finally:
        ds.close()
        r.close()


def test_stage_from_files_with_the_similarity_override(tmp_path):
    """A byte field written by Lucene carries a Lucene ordinal; staged with the override it is a Hamming field
    (osk_seg_stage_file), equal to the same bytes staged from memory; without it, it stays what the file says."""
    from opensearch_amd import flatfiles as FF
    sid = bytes(range(16))
    n, dim, max_doc = 3000, 50, 7000
    ckey = ("i-files", dim)
    rows, queries = corpus(ckey, n, dim, 4, 6800)
    docs = np.sort(np.random.default_rng(8).choice(max_doc, n, replace=False)).astype(np.int32)
    FF.write_segment(str(tmp_path), "_h", sid, max_doc, [(3, rows.view(np.int8), int(LU.VectorSimilarityFunction.EUCLIDEAN),
                                                          docs)])
    readers = [LU.GpuBinaryVectorsReader.from_files("v", str(tmp_path), "_h", sid, max_doc, 3),
               LU.GpuFlatVectorsReader.from_files("v", str(tmp_path), "_h", sid, max_doc, 3, similarity=HAM)]
    plain = LU.GpuFlatVectorsReader.from_files("v", str(tmp_path), "_h", sid, max_doc, 3)
    try:
        assert plain.similarity == LU.VectorSimilarityFunction.EUCLIDEAN and not isinstance(plain, LU.GpuBinaryVectorsReader)
        acc = np.random.default_rng(9).random(max_doc) < 0.4
        for r in readers:
            assert isinstance(r, LU.GpuBinaryVectorsReader)
            assert (r.dim, r.size, r.similarity, r.encoding, r.max_doc) == (dim, n, HAM, LU.VectorEncoding.BYTE, max_doc)
            for k in (10, 100):
                check_segment(r, ckey, rows, queries, [0, 1, 2, 3], k, docs, None)
                check_segment(r, ckey, rows, queries, [2], k, docs, acc)
    finally:
        for r in readers + [plain]:
            r.close()


@pytest.mark.parametrize("dim", [17, 100])
def test_padding_adds_nothing(dim, stream_knob):
    """The all-0xFF query against rows whose last unit is partly padding: a padding byte that counted would add
    8 to every distance.  Also alone vs in a batch (scan_ham), and through the select path."""
    n = 3000
    ckey = ("i-pad", dim)
    rows, queries = corpus(ckey, n, dim, 4, 6700 + dim)
    assert np.all(queries[1] == 0xFF)
    r = LU.GpuBinaryVectorsReader("v", rows)
    try:
        for k in (10, 100):
            s, d, c, v = check_segment(r, ckey, rows, queries, [1], k)
            assert d[0, 0] in (1, n // 2 + 1, n - 3) and s[0, 0] == np.float32(1.0)      # an all-0xFF edge row
            check_segment(r, ckey, rows, queries, [0, 1, 2, 3], k)
        worst = r.search_batch(queries[1], n)[0][0, n - 1]       # the all-0x00 rows: every real bit differs
        assert worst == np.float32(1.0) / np.float32(1 + 8 * dim)
    finally:
        r.close()
