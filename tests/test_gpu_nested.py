"""Exact nested k-NN on the device: the k best parents, each represented by its best accepted child
([L] DiversifyingChildrenFloatKnnVectorQuery / DiversifyingChildrenByteKnnVectorQuery.exactSearch; what
OpenSearch k-NN builds for a `knn` query inside a `nested` query).

Reference for every case, here in the test file: `oracle.exact_search(rows, q, k = n_rows, sim, ORDER_DEVICE,
ord_to_doc, accept_bits)` gives every accepted non-NaN row's device-order score; the parent of a doc is
`np.searchsorted(parent_docs, doc, side="left")`; per parent keep the row with (max score, then min doc); sort
those by (−score, doc) and cut to k.  Required: docs equal, score bits equal, count equal, visited equal, unused
slots -inf / INT32_MAX.
"""

import ctypes as C

import numpy as np
import pytest

from opensearch_amd import _lib, dsl as Q, lucene as LU
from oracle import byte_reference as BR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIM = LU.VectorSimilarityFunction
F32, BYTE = LU.VectorEncoding.FLOAT32, LU.VectorEncoding.BYTE
INT32_MAX = 2**31 - 1
FAMILY_SIZES = (1, 2, 3, 5, 17, 64, 65, 300)

_oracle_cache: dict = {}


def synth(n, dim, seed, enc=F32):
    return O.synth(0, n, dim, seed, _lib.DIST_INT8 if enc == BYTE else _lib.DIST_NORMALISH_UNIT)


def all_scores(key, rows, q, sim, o2d=None, accept=None):
    """Every accepted non-NaN row of one leaf as (docs, scores), and visited.  One oracle call per `key`, shared
    by the tests and left unchanged."""
    if key not in _oracle_cache:
        ab = None if accept is None else O.bits_from_bool(accept)
        s, d, vis = O.exact_search(rows, q, len(rows), int(sim), O.ORDER_DEVICE, o2d, ab)
        _oracle_cache[key] = (d.copy(), s.copy(), vis)
        for a in _oracle_cache[key][:2]:
            a.setflags(write=False)
    return _oracle_cache[key]


def nested_reference(docs, scores, parent_docs, k):
    """The k best families of one leaf as (child docs, scores): per parent the row with (max score, then min
    doc), those by (score desc, doc asc), cut to k."""
    docs, scores = np.asarray(docs), np.asarray(scores, np.float32)
    keep = ~np.isnan(scores)
    docs, scores = docs[keep], scores[keep]
    pid = np.searchsorted(np.asarray(parent_docs), docs, side="left")
    order = np.lexsort((docs, -scores.astype(np.float64)))      # score desc, then doc asc
    d, s, p = docs[order], scores[order], pid[order]
    _, first = np.unique(p, return_index=True)                  # a parent's first row in that order = its best child
    first.sort()                                                # ... and the best children stay in that order
    return d[first][:k], s[first][:k]


def families(n, seed, sizes=FAMILY_SIZES):
    """n child rows in families of sizes drawn from `sizes`; every family's children are followed by their parent
    doc, which has no vector → (ord_to_doc, parent_docs, max_doc)."""
    rng = np.random.default_rng(seed)
    o2d, parents, doc, left = [], [], 0, n
    while left > 0:
        f = min(int(rng.choice(sizes)), left)
        o2d.extend(range(doc, doc + f))
        doc += f
        parents.append(doc)
        doc += 1
        left -= f
    return np.asarray(o2d, np.int32), np.asarray(parents, np.int32), doc


def parent_mask(parent_docs, max_doc):
    m = np.zeros(max_doc, bool)
    m[parent_docs] = True
    return m


def assert_result(got, want, k, ctx=""):
    scores, docs, count = got
    wd, ws = want
    assert int(count) == len(wd), (ctx, int(count), len(wd))
    n = len(wd)
    assert np.array_equal(docs[:n], wd), (ctx, docs[:n], wd)
    assert np.array_equal(scores[:n].view(np.uint32), ws.view(np.uint32)), ctx
    assert np.all(docs[n:k] == INT32_MAX) and np.all(np.isneginf(scores[n:k])), ctx


def nested_reader(rows, sim, enc, o2d, parents, max_doc):
    r = LU.GpuFlatVectorsReader("v", rows, sim, enc, ord_to_doc=o2d, max_doc=max_doc)
    r.set_parents(parent_mask(parents, max_doc))
    return r


# ------------------------------------------------------------------------------------------------
# lane configs × similarities: 4097 rows of a sparse field (parents have no vectors), families that straddle
# steps, waves and tiles; a 9-query call (two passes, the second with one query) and a single-query call
# ------------------------------------------------------------------------------------------------
CASES = [(F32, dim, sim) for dim in (3, 96, 128, 768, 1030) for sim in SIM] + \
        [(BYTE, dim, sim) for dim in (16, 100, 768) for sim in (SIM.EUCLIDEAN, SIM.DOT_PRODUCT)]
# byte lane configs whose 8-query instantiation reads its query fragments from LDS (dims above 256), and 250 which
# keeps them in registers, on the two similarities the cases above leave out; these corpora carry the byte edge
# set (byte_reference.edge_rows: a zero child — NaN under COSINE — among them) and the queries all −128, all 127
# and all 0
BYTE_EDGE_CASES = [(BYTE, dim, sim) for dim in (250, 1100, 3000, 4096) for sim in (SIM.COSINE, SIM.MAXIMUM_INNER_PRODUCT)]
CASES += BYTE_EDGE_CASES


@pytest.mark.parametrize("enc,dim,sim", CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_lane_configs(enc, dim, sim):
    n = 4097
    rows = synth(n, dim, 100 + dim, enc)
    qs = synth(9, dim, 7 + dim, enc)
    edges = (enc, dim, sim) in BYTE_EDGE_CASES
    if edges:
        BR.inject_edges(rows)
        BR.edge_queries(qs)          # 0: all −128, 1: all 127, 4: all 0, 8 (the second pass's only query): alternating
    o2d, parents, max_doc = families(n, 11)
    assert {int(f) for f in np.diff(np.concatenate([[-1], parents])) - 1} >= {1, 17, 65, 300}
    r = nested_reader(rows, sim, enc, o2d, parents, max_doc)
    try:
        assert r.n_parents() == len(parents)
        scored = [all_scores(("lane", enc, dim, sim, i), rows, qs[i], sim, o2d) for i in range(9)]
        for k in (1, 10, 64):
            s, d, c, v = r.search_nested(qs, k)
            for i in range(9):
                assert_result((s[i], d[i], c[i]), nested_reference(scored[i][0], scored[i][1], parents, k), k,
                              (enc, dim, sim, k, i))
                assert v[i] == scored[i][2] == n
            if edges:     # (a family whose only child is a zero vector is absent under COSINE)
                assert c[0] == min(k, len(np.unique(np.searchsorted(parents, scored[0][0], side="left"))))
            else:
                assert c[0] == min(k, len(parents))
            s1, d1, c1, v1 = r.search_nested(qs[3], k)
            assert_result((s1[0], d1[0], c1[0]), nested_reference(scored[3][0], scored[3][1], parents, k), k)
            assert v1[0] == n
            if edges:
                # one 8-query call: a single pass of the 8-query instantiation
                s8, d8, c8, v8 = r.search_nested(qs[:8], k)
                for i in range(8):
                    assert_result((s8[i], d8[i], c8[i]), nested_reference(scored[i][0], scored[i][1], parents, k), k,
                                  ("8-query", dim, sim, k, i))
                    assert v8[i] == n
                assert c[4] == (0 if sim == SIM.COSINE else min(k, len(parents)))     # the zero query
        if edges:
            # the oracle's scores are byte_reference's, row for row (COSINE: the zero children are the ones left out)
            for i in (0, 1, 3, 8):
                ref = BR.scores(rows, qs[i], int(sim))
                order = np.argsort(scored[i][0], kind="stable")
                assert np.array_equal(o2d[~np.isnan(ref)], scored[i][0][order])
                assert np.array_equal(ref[~np.isnan(ref)].view(np.uint32), scored[i][1][order].view(np.uint32))
                assert (len(scored[i][0]) < n) == (sim == SIM.COSINE)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# degenerate families
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc,dim", [(F32, 96), (BYTE, 100)], ids=["f32", "byte"])
def test_every_row_its_own_parent_equals_knn(enc, dim):
    n, sim = 4097, SIM.EUCLIDEAN
    rows = synth(n, dim, 200, enc)
    qs = synth(3, dim, 201, enc)
    r = LU.GpuFlatVectorsReader("v", rows, sim, enc)
    try:
        r.set_parents(np.ones(n, bool))
        for k in (1, 10, 64):
            a, b = r.search_nested(qs, k), r.search_batch(qs, k)
            for x, y in zip(a, b):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
    finally:
        r.close()


def test_one_family_of_all_rows():
    n, dim, sim = 4097, 96, SIM.COSINE
    rows = synth(n, dim, 210)
    q = synth(1, dim, 211)[0]
    r = nested_reader(rows, sim, F32, np.arange(n, dtype=np.int32), np.array([n], np.int32), n + 1)
    try:
        scored = all_scores(("onefam",), rows, q, sim)
        for k in (1, 10, 64):
            s, d, c, v = r.search_nested(q, k)
            assert c[0] == 1 and v[0] == n
            assert_result((s[0], d[0], c[0]), nested_reference(scored[0], scored[1], [n], k), k)
        assert s[0, 0] == scored[1].max()
    finally:
        r.close()


def test_fewer_families_than_k():
    n, dim, sim = 700, 96, SIM.MAXIMUM_INNER_PRODUCT
    rows = synth(n, dim, 220)
    q = synth(1, dim, 221)[0]
    o2d, parents, max_doc = families(n, 3, sizes=(65, 300))
    assert 1 < len(parents) < 10
    r = nested_reader(rows, sim, F32, o2d, parents, max_doc)
    try:
        scored = all_scores(("fewer",), rows, q, sim, o2d)
        s, d, c, v = r.search_nested(q, 10)
        assert c[0] == len(parents) < 10 and v[0] == n
        assert_result((s[0], d[0], c[0]), nested_reference(scored[0], scored[1], parents, 10), 10)
    finally:
        r.close()


@pytest.mark.parametrize("enc,dim", [(F32, 96), (BYTE, 16)], ids=["f32", "byte"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_row_counts_at_edges(n, enc, dim):
    sim = SIM.EUCLIDEAN
    rows = synth(n, dim, 300 + n, enc)
    q = synth(1, dim, 301, enc)[0]
    o2d, parents, max_doc = families(n, n, sizes=(1, 2, 3, 5))
    r = nested_reader(rows, sim, enc, o2d, parents, max_doc)
    try:
        scored = all_scores(("edge", enc, n), rows, q, sim, o2d)
        for k in (1, 10, 64):
            s, d, c, v = r.search_nested(q, k)
            assert_result((s[0], d[0], c[0]), nested_reference(scored[0], scored[1], parents, k), k, (n, k))
            assert v[0] == n
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# ties: equal scores inside a family → the lower child doc; the same row in two families → both, lower doc first
# ------------------------------------------------------------------------------------------------
def test_ties():
    dim, sim, n = 96, SIM.DOT_PRODUCT, 64
    rows = synth(n, dim, 500)
    q = rows[3].copy()                       # unit rows: row 3 and its copies score highest
    rows[1] = rows[5] = rows[6] = rows[3]    # families of 4: rows 1, 3 in family 0, rows 5, 6 in family 1
    o2d, parents, max_doc = families(n, 0, sizes=(4,))
    r = nested_reader(rows, sim, F32, o2d, parents, max_doc)
    try:
        scored = all_scores(("ties",), rows, q, sim, o2d)
        top = np.sort(scored[1])[::-1]
        assert top[3] == top[0] > top[4]
        for k, want_docs in ((1, [o2d[1]]), (2, [o2d[1], o2d[5]])):
            s, d, c, _ = r.search_nested(q, k)
            assert d[0, :k].tolist() == want_docs and c[0] == k
            assert_result((s[0], d[0], c[0]), nested_reference(scored[0], scored[1], parents, k), k)
            assert np.all(s[0, :k] == top[0])
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# NaN: a COSINE zero vector is visited but never a best child; a family of only zero vectors is absent
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc,dim", [(F32, 96), (BYTE, 100)], ids=["f32", "byte"])
def test_nan_children(enc, dim):
    n = 200
    rows = synth(n, dim, 600, enc)
    rows[::7] = 0
    rows[8:12] = 0                            # family 2 entirely
    o2d, parents, max_doc = families(n, 0, sizes=(4,))
    r = nested_reader(rows, SIM.COSINE, enc, o2d, parents, max_doc)
    try:
        s, d, c, v = r.search_nested(np.zeros(dim, rows.dtype), 10)
        assert c[0] == 0 and v[0] == n and np.all(d[0] == INT32_MAX) and np.all(np.isneginf(s[0]))
        q = synth(1, dim, 601, enc)[0]
        scored = all_scores(("nan", enc), rows, q, SIM.COSINE, o2d)
        assert len(scored[0]) == n - len(set(range(0, n, 7)) | set(range(8, 12)))
        s, d, c, v = r.search_nested(q, 64)
        assert_result((s[0], d[0], c[0]), nested_reference(scored[0], scored[1], parents, 64), 64)
        assert c[0] == len(parents) - 1 == 49 and v[0] == n and not np.isnan(s[0, :c[0]]).any()
        assert not set(d[0, :c[0]].tolist()) & set(o2d[8:12].tolist())
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# filters: ≈ 1 % and 50 %; a sparse field, and a dense one (the compacted walk with multi-row families: every doc
# has a vector, every 5th doc and the last one are parents)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("pct", [1, 50])
def test_filtered(pct, sparse):
    dim, sim, n = 96, SIM.EUCLIDEAN, 4097
    rows = synth(n, dim, 700)
    qs = synth(2, dim, 701)
    rng = np.random.default_rng(pct)
    if sparse:
        o2d, parents, max_doc = families(n, 12)
    else:
        o2d, max_doc = None, n
        parents = np.union1d(np.arange(4, n, 5), [n - 1]).astype(np.int32)
    acc = rng.random(max_doc) < pct / 100
    lo = 0
    for p in parents[:40:4]:                                  # some families rejected entirely
        acc[lo:p + 1] = False
        lo = p + 1
    r = nested_reader(rows, sim, F32, o2d, parents, max_doc)
    try:
        n_acc = int(acc[o2d].sum()) if sparse else int(acc.sum())
        for qi in range(2):
            scored = all_scores(("filt", pct, sparse, qi), rows, qs[qi], sim, o2d, acc)
            assert scored[2] == n_acc > 0
            for k in (1, 10, 64):
                s, d, c, v = r.search_nested(qs[qi], k, LU.bits_from_bool(acc))
                assert_result((s[0], d[0], c[0]), nested_reference(scored[0], scored[1], parents, k), k, (pct, sparse, k))
                assert v[0] == n_acc
        s, d, c, v = r.search_nested(qs, 10, LU.bits_from_bool(acc))          # both in one pass
        for qi in range(2):
            scored = all_scores(("filt", pct, sparse, qi), rows, qs[qi], sim, o2d, acc)
            assert_result((s[qi], d[qi], c[qi]), nested_reference(scored[0], scored[1], parents, 10), 10)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# a view of 3 segments in 2 shards (non-zero doc bases, one segment of 1 row): the three entries agree
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def view3():
    dim, sim = 128, SIM.COSINE
    sizes = [5000, 1, 9000]
    rows = [synth(n, dim, 400 + i) for i, n in enumerate(sizes)]
    rng = np.random.default_rng(5)
    o2d = [None, None, np.sort(rng.choice(19999, sizes[2], replace=False)).astype(np.int32)]
    max_doc = [5000, 1, 20000]
    free = np.setdiff1d(np.arange(19999), o2d[2])
    parents = [np.union1d(np.arange(4, 5000, 5), [4999]).astype(np.int32), np.array([0], np.int32),
               np.union1d(rng.choice(free, 1500, replace=False), [19999]).astype(np.int32)]
    bases = [3, 5003 + 10, 17]                   # shard 0: segments 0, 1; shard 1: segment 2
    readers = [LU.GpuFlatVectorsReader("v", rows[i], sim, F32, ord_to_doc=o2d[i], max_doc=max_doc[i]) for i in range(3)]
    leaves = [[LU.LeafReaderContext(0, bases[0], readers[0]), LU.LeafReaderContext(1, bases[1], readers[1])],
              [LU.LeafReaderContext(0, bases[2], readers[2])]]
    ds = LU.DeviceShardSet(leaves, [0, 1])
    queries = synth(9, dim, 450)
    yield dict(dim=dim, sim=sim, rows=rows, o2d=o2d, max_doc=max_doc, bases=bases, readers=readers, leaves=leaves,
               ds=ds, queries=queries, shard_of=[0, 0, 1], parents=parents)
    ds.close()
    for r in readers:
        r.close()


def register(v):
    for r, p, m in zip(v["readers"], v["parents"], v["max_doc"]):
        r.set_parents(parent_mask(p, m))


def shard_reference(v, qi, k, accept=None):
    """Per shard the k best families (shard-local child docs, scores) + visited per segment."""
    per_shard, visited = [[], []], []
    for i in range(3):
        acc = None if accept is None else accept[i]
        akey = None if acc is None else acc.tobytes()
        d, s, vis = all_scores(("view3", i, qi, akey), v["rows"][i], v["queries"][qi], v["sim"], v["o2d"][i], acc)
        bd, bs = nested_reference(d, s, v["parents"][i], k)
        per_shard[v["shard_of"][i]].append((bd + v["bases"][i], bs))
        visited.append(vis)
    out = []
    for ps in per_shard:
        d, s = np.concatenate([p[0] for p in ps]), np.concatenate([p[1] for p in ps])
        order = np.lexsort((d, -s.astype(np.float64)))[:k]
        out.append((d[order], s[order]))
    return out, visited


def test_search_before_parents_is_invalid(view3):
    """(first in the file's view tests: nothing is registered yet)"""
    v = view3
    assert v["readers"][0].n_parents() == 0
    with pytest.raises(_lib.OskError) as e:
        v["readers"][0].search_nested(v["queries"][0], 10)
    assert e.value.code == _lib.OSK_ERR_INVALID and "parents" in str(e.value)
    with pytest.raises(_lib.OskError) as e:
        v["ds"].search_nested(v["queries"][0], 10)
    assert e.value.code == _lib.OSK_ERR_INVALID
    v["readers"][0].set_parents(parent_mask(v["parents"][0], v["max_doc"][0]))
    with pytest.raises(_lib.OskError) as e:                     # one segment of the view still has none
        v["ds"].search_nested(v["queries"][0], 10)
    assert e.value.code == _lib.OSK_ERR_INVALID


def device_call(v, q, k):
    import torch
    ds = v["ds"]
    nq, S = len(q), ds.n_shards
    tq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    keys = torch.full((nq, S, k), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((nq, S), -7, dtype=torch.int32, device="cuda")
    visited = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        _lib.check(_lib.lib().osk_view_search_nested_device(ds.handle, tq.data_ptr(), nq, k, None, keys.data_ptr(),
                                                            counts.data_ptr(), visited.data_ptr(), st.cuda_stream))
    st.synchronize()
    s, d = LU.decode_keys(keys.cpu().numpy().view(np.uint64))
    return s, d, counts.cpu().numpy(), visited.cpu().numpy()


def test_view_entries_agree(view3):
    v = view3
    register(v)
    ds, k = v["ds"], 10
    c0 = ds.counter("nested_calls")
    before = ds.search(v["queries"][:3], 10, 0, 10)
    calls = 0
    for qi in (0, 1):
        want, visited = shard_reference(v, qi, k)
        # the device entry: per-shard keys in the k-NN layout
        s, d, c, vis = device_call(v, v["queries"][qi:qi + 1], k)
        calls += 1
        for sh in range(2):
            assert_result((s[0, sh], d[0, sh], c[0, sh]), want[sh], k, ("device", qi, sh))
        assert list(vis) == visited == [5000, 1, 9000]
        # the host entry: the coordinator reduce of those lists
        for from_, size in ((0, 10), (3, 5)):
            ws, wd, wsh, wtot, wmax = O.topdocs_merge([(w[1], w[0]) for w in want], from_, size, [0, 1])
            hs, hd, hsh, hc, htot, hmax = ds.search_nested(v["queries"][qi], k, from_, size)
            calls += 1
            n = len(wd)
            assert hc[0] == n == size and htot[0] == wtot and hmax[0] == np.float32(wmax)
            assert np.array_equal(hd[0, :n], wd) and np.array_equal(hsh[0, :n], wsh)
            assert np.array_equal(hs[0, :n].view(np.uint32), ws.view(np.uint32))
        # the segment entry: segment-local docs
        for i in range(3):
            d_, s_, vis_ = all_scores(("view3", i, qi, None), v["rows"][i], v["queries"][qi], v["sim"], v["o2d"][i])
            ss, sd, sc, sv = v["readers"][i].search_nested(v["queries"][qi], k)
            assert_result((ss[0], sd[0], sc[0]), nested_reference(d_, s_, v["parents"][i], k), k, ("seg", qi, i))
            assert sv[0] == len(v["rows"][i])
    assert ds.counter("nested_calls") - c0 == calls          # (segment entries run on the segments' own views)
    after = ds.search(v["queries"][:3], 10, 0, 10)
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_view_batch_and_filter(view3):
    v = view3
    register(v)
    rng = np.random.default_rng(21)
    accept = [rng.random(5000) < 0.3, None, rng.random(20000) < 0.5]
    k = 64
    s, d, c, vis = None, None, None, None
    hs, hd, hsh, hc, htot, hmax = v["ds"].search_nested(v["queries"], k, 0, 100, accept=accept)   # 9 queries: 2 passes
    for qi in range(9):
        want, _ = shard_reference(v, qi, k, accept)
        ws, wd, wsh, wtot, wmax = O.topdocs_merge([(w[1], w[0]) for w in want], 0, 100, [0, 1])
        n = len(wd)
        assert hc[qi] == n and htot[qi] == wtot
        assert np.array_equal(hd[qi, :n], wd) and np.array_equal(hsh[qi, :n], wsh), qi
        assert np.array_equal(hs[qi, :n].view(np.uint32), ws.view(np.uint32)), qi


# ------------------------------------------------------------------------------------------------
# the Python query classes and the block-join step of the shard's query phase
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
        pf = lambda leaf: parent_mask(v["parents"][0 if leaf.max_doc > 1 else 1], leaf.max_doc)             # noqa: E731
        q, k = v["queries"][2], 10
        accept = [live[0] & flt(leaves[0]), flt(leaves[1])]
        best = []
        for i in range(2):
            d, s, _ = all_scores(("qc", i), v["rows"][i], q, v["sim"], None, accept[i])
            bd, bs = nested_reference(d, s, v["parents"][i], k)
            best.append((bd + v["bases"][i], bs))
        wd, ws = np.concatenate([b[0] for b in best]), np.concatenate([b[1] for b in best])
        order = np.lexsort((wd, -ws.astype(np.float64)))[:k]
        wd, ws = wd[order], ws[order]
        per_leaf = LU.DiversifyingChildrenFloatKnnVectorQuery("v", q, flt, k, pf)
        gpu = LU.GpuDiversifyingChildrenFloatKnnVectorQuery("v", q, flt, k, pf)
        for td in (per_leaf.rewrite(leaves), gpu.rewrite(leaves)):
            assert [h.doc for h in td.score_docs] == wd.tolist()
            assert np.array_equal(np.array([h.score for h in td.score_docs], np.float32).view(np.uint32), ws.view(np.uint32))
        # the block join: each child hit becomes its parent, once, scored by the child, the child kept
        for query in (per_leaf, gpu):
            td = LU.shard_nested_query_phase(query, leaves, pf, 2, 5)
            assert td.total_hits.value == k and len(td.score_docs) == 7
            pdocs = [h.doc for h in td.score_docs]
            assert len(set(pdocs)) == len(pdocs)
            for h in td.score_docs:
                i = 0 if h.doc < v["bases"][1] else 1
                local_child = h.child_doc - v["bases"][i]
                parent = v["parents"][i][np.searchsorted(v["parents"][i], local_child, side="left")] + v["bases"][i]
                assert h.doc == parent and h.child_doc in wd.tolist()
                assert h.score == float(ws[wd.tolist().index(h.child_doc)])
            assert [h.score for h in td.score_docs] == sorted((h.score for h in td.score_docs), reverse=True)
        # through the DSL: knn inside nested
        ctx = Q.QueryShardContext({"v": Q.parse_knn_vector_mapping(
            "v", {"type": "knn_vector", "dimension": v["dim"], "space_type": "cosinesimil"})},
            parent_docs=lambda leaf, path: pf(leaf))
        built = Q.parse_nested_query({"nested": {"path": "chunks", "query": {"knn": {"v": {"vector": q.tolist(), "k": k}}}}}
                                     ).do_to_query(ctx)
        assert isinstance(built, LU.DiversifyingChildrenFloatKnnVectorQuery)
        unfiltered = LU.DiversifyingChildrenFloatKnnVectorQuery("v", q, None, k, pf).rewrite(leaves)
        assert [(h.doc, h.score) for h in built.rewrite(leaves).score_docs] == [(h.doc, h.score) for h in unfiltered.score_docs]
    finally:
        for lf in leaves:
            lf.live_docs = None
        LU._GpuKnnVectorQuery.release_views()


def test_byte_query_classes():
    dim, n, k = 100, 2000, 10
    rows = synth(n, dim, 900, BYTE)
    q = synth(1, dim, 901, BYTE)[0]
    o2d, parents, max_doc = families(n, 5)
    r = LU.GpuFlatVectorsReader("v", rows, SIM.DOT_PRODUCT, BYTE, ord_to_doc=o2d, max_doc=max_doc)
    try:
        leaves = [LU.LeafReaderContext(0, 0, r)]
        d, s, _ = all_scores(("byteq",), rows, q, SIM.DOT_PRODUCT, o2d)
        wd, ws = nested_reference(d, s, parents, k)
        pf = lambda leaf: parent_mask(parents, max_doc)   # noqa: E731
        for cls in (LU.DiversifyingChildrenByteKnnVectorQuery, LU.GpuDiversifyingChildrenByteKnnVectorQuery):
            td = cls("v", q, None, k, pf).rewrite(leaves)
            assert [h.doc for h in td.score_docs] == wd.tolist()
            assert [h.score for h in td.score_docs] == [float(x) for x in ws]
    finally:
        LU._GpuKnnVectorQuery.release_views()
        r.close()


# ------------------------------------------------------------------------------------------------
# errors
# ------------------------------------------------------------------------------------------------
def test_registration_errors():
    n, dim = 100, 16
    rows = synth(n, dim, 950)
    o2d, parents, max_doc = families(n, 1, sizes=(5,))
    r = LU.GpuFlatVectorsReader("v", rows, SIM.EUCLIDEAN, F32, ord_to_doc=o2d, max_doc=max_doc)
    try:
        L = _lib.lib()
        got = C.c_int64(-1)
        _lib.check(L.osk_seg_parents(r.handle, C.byref(got)))
        assert got.value == 0
        fp0 = C.c_int64()
        _lib.check(L.osk_seg_footprint(r.handle, C.byref(fp0)))
        short = LU.bits_from_bool(parent_mask(parents[:-1], max_doc))          # the last family has no parent
        assert L.osk_seg_set_parents(r.handle, short.ctypes.data) == _lib.OSK_ERR_INVALID
        assert "after the last parent" in L.osk_last_error().decode()
        empty = LU.bits_from_bool(np.zeros(max_doc, bool))
        assert L.osk_seg_set_parents(r.handle, empty.ctypes.data) == _lib.OSK_ERR_INVALID
        assert L.osk_seg_set_parents(r.handle, None) == _lib.OSK_ERR_INVALID
        _lib.check(L.osk_seg_parents(r.handle, C.byref(got)))
        assert got.value == 0                                                   # a refused call registers nothing
        good = LU.bits_from_bool(parent_mask(parents, max_doc))
        _lib.check(L.osk_seg_set_parents(r.handle, good.ctypes.data))
        _lib.check(L.osk_seg_parents(r.handle, C.byref(got)))
        assert got.value == len(parents) == 20
        fp1 = C.c_int64()
        _lib.check(L.osk_seg_footprint(r.handle, C.byref(fp1)))
        assert fp1.value - fp0.value == 4 * n                                   # the row→parent table
        assert L.osk_seg_set_parents(r.handle, good.ctypes.data) == _lib.OSK_ERR_INVALID   # a second call
        assert "already" in L.osk_last_error().decode()
        with pytest.raises(_lib.OskError) as e:
            r.search_nested(rows[0], 65)
        assert e.value.code == _lib.OSK_ERR_UNSUPPORTED and "64" in str(e.value)
        s, d, c, v = r.search_nested(rows[0], 64)
        assert c[0] == 20 and d[0, 0] == o2d[0] and v[0] == n
        # the Python reader: the same mask again is accepted, another one is refused
        r2 = LU.GpuFlatVectorsReader("v", rows, SIM.EUCLIDEAN, F32, ord_to_doc=o2d, max_doc=max_doc)
        try:
            r2.set_parents(parent_mask(parents, max_doc))
            r2.set_parents(parent_mask(parents, max_doc))
            other = parent_mask(parents, max_doc)
            other[0] = True
            with pytest.raises(ValueError):
                r2.set_parents(other)
        finally:
            r2.close()
    finally:
        r.close()
