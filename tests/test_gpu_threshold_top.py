"""Radial search collected by score on the device: each shard's best k matches of a similarity threshold, in the
k-NN entries' layout, with the exact number of matches (osk_seg_search_threshold_top, osk_view_search_threshold_top,
osk_view_search_threshold_top_device — the shard's TopScoreDocCollector over [L] AbstractVectorSimilarityQuery).

Reference for every case: `oracle.exact_search(rows, q, k = n_rows, sim, ORDER_DEVICE, ord_to_doc, accept_bits)` gives
every accepted non-NaN row's device-order score; keep `score >= np.float32(min_score)`, sort by (−score, doc), cut to
k; the length before the cut is the total.  No tolerance anywhere: docs, score bits (as uint32), counts, totals and
visited are compared for equality.
"""
import contextlib

import numpy as np
import pytest
import torch

from opensearch_amd import _lib, lucene as LU
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
    """Every accepted non-NaN row of one leaf as (docs, scores) by (−score, doc), and visited.  One oracle call per
    `key`, shared by the tests and left unchanged."""
    if key not in _oracle_cache:
        ab = None if accept is None else O.bits_from_bool(accept)
        s, d, vis = O.exact_search(rows, q, len(rows), int(sim), O.ORDER_DEVICE, o2d, ab)
        order = np.lexsort((d, -s.astype(np.float64)))
        _oracle_cache[key] = (d[order].copy(), s[order].copy(), vis)
        for a in _oracle_cache[key][:2]:
            a.setflags(write=False)
    return _oracle_cache[key]


def matches(scored, min_score, doc_base=0):
    """The reference's matches, best first: (docs, scores)."""
    d, s, _ = scored
    keep = s >= np.float32(min_score)          # float32 comparison: NaN on either side is False
    return d[keep] + doc_base, s[keep]


def jth_best(scored, j):
    return scored[1][min(j, len(scored[1])) - 1]


def thresholds(scored):
    """The issue's thresholds, taken from the reference itself: the 1st, 10th and 500th best score, just above the
    maximum, −inf, 0.0 and NaN."""
    mx = jth_best(scored, 1)
    return np.array([mx, jth_best(scored, 10), jth_best(scored, 500), np.nextafter(mx, np.float32(np.inf)), NEG_INF,
                     0.0, np.nan], np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_top(got, want, k, ctx=""):
    """got = (scores[k], docs[k], count, total) of one (query, shard); want = every match, best first."""
    scores, docs, count, total = got
    wd, ws = want
    assert int(total) == len(wd), (ctx, int(total), len(wd))
    n = min(len(wd), k)
    assert int(count) == n, (ctx, int(count), n)
    assert np.array_equal(docs[:n], wd[:n]), (ctx, docs[:n], wd[:n])
    assert np.array_equal(bits(scores[:n]), bits(ws[:n])), ctx
    assert np.all(docs[n:k] == INT32_MAX) and np.all(np.isneginf(scores[n:k])), ctx


def decode(keys):
    return LU.decode_keys(keys)


@contextlib.contextmanager
def knob(key, value, default):
    _lib.tune(key, value)
    try:
        yield
    finally:
        _lib.tune(key, default)


def device_call(ds, q, ms, k, n_segs):
    """osk_view_search_threshold_top_device on a stream of its own: (keys[nq,S,k], counts[nq,S], totals[nq,S],
    visited[n_segs])."""
    q = np.ascontiguousarray(q)
    nq, S = len(q), ds.n_shards
    tq = torch.from_numpy(q).cuda()
    tms = torch.from_numpy(np.ascontiguousarray(ms, np.float32)).cuda()
    keys = torch.full((nq, S, k), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((nq, S), -7, dtype=torch.int32, device="cuda")
    totals = torch.full((nq, S), -7, dtype=torch.int64, device="cuda")
    visited = torch.full((n_segs,), -7, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        _lib.check(_lib.lib().osk_view_search_threshold_top_device(
            ds.handle, tq.data_ptr(), nq, tms.data_ptr(), k, None, keys.data_ptr(), counts.data_ptr(),
            totals.data_ptr(), visited.data_ptr(), st.cuda_stream))
    st.synchronize()
    return (keys.cpu().numpy().view(np.uint64), counts.cpu().numpy(), totals.cpu().numpy(), visited.cpu().numpy())


# ------------------------------------------------------------------------------------------------
# lane configs and padding × similarities, 4097 rows: wave ranges that are no multiple of 64
# ------------------------------------------------------------------------------------------------
CASES = [(F32, dim, sim) for dim in (3, 96, 128, 768, 1030) for sim in SIM] + \
        [(BYTE, dim, sim) for dim in (16, 100, 768, 1100, 4096) for sim in SIM]


@pytest.mark.parametrize("enc,dim,sim", CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_lane_configs_and_thresholds(enc, dim, sim):
    n = 4097
    rows = synth(n, dim, 100 + dim, enc)
    q = synth(2, dim, 7 + dim, enc)[1]
    if enc == BYTE and sim in (SIM.COSINE, SIM.MAXIMUM_INNER_PRODUCT):
        BR.inject_edges(rows)                  # all −128, all 127, alternating, all 0 (NaN under COSINE), a duplicate
    r = LU.GpuFlatVectorsReader("v", rows, sim, enc)
    try:
        scored = all_scores(("lane", enc, dim, sim), rows, q, sim)
        ms = thresholds(scored)
        want = [matches(scored, m) for m in ms]
        # the thresholds' totals: the row scoring exactly min_score is a match; above the maximum and NaN: none;
        # −inf: every non-NaN row; 0.0: every row with a non-negative score
        assert len(want[0][0]) >= 1 and len(want[1][0]) >= 10 and len(want[2][0]) >= 500
        assert len(want[3][0]) == 0 and len(want[6][0]) == 0 and len(want[4][0]) == len(scored[0])
        assert len(want[5][0]) == int((scored[1] >= 0).sum())
        for k in (1, 10, 64):
            # one call, the same target under 7 thresholds: two corpus passes ...
            s, d, c, t, v = r.search_threshold_top(np.repeat(q[None], len(ms), 0), ms, k)
            for i in range(len(ms)):
                assert_top((s[i], d[i], c[i], t[i]), want[i], k, (enc, dim, sim, k, i))
                assert v[i] == scored[2] == n
            # ... and a single-query call gives the same
            s1, d1, c1, t1, v1 = r.search_threshold_top(q, ms[1], k)
            assert_top((s1[0], d1[0], c1[0], t1[0]), want[1], k, (enc, dim, sim, k, "single"))
            assert v1[0] == n
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# the k boundary: wave lists up to 64, the select path's tail above; every row a match, and nearly none
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc,dim,sim", [(F32, 96, SIM.COSINE), (BYTE, 100, SIM.DOT_PRODUCT)], ids=["f32", "byte"])
def test_k_boundary_and_select_hook(enc, dim, sim):
    n = 4097
    rows = synth(n, dim, 1200, enc)
    q = synth(1, dim, 1201, enc)[0]
    r = LU.GpuFlatVectorsReader("v", rows, sim, enc)
    ds = LU.DeviceShardSet([[LU.LeafReaderContext(0, 0, r)]], [0])
    try:
        scored = all_scores(("kb", enc), rows, q, sim)
        for k in (64, 65, 500, 4097, 10000):
            for m in (NEG_INF, jth_best(scored, 10)):
                want = matches(scored, m)
                assert len(want[0]) == n or 10 <= len(want[0]) < 64
                c0, s0 = ds.counter("threshold_top_calls"), ds.counter("threshold_top_select_calls")
                s, d, sh, c, t, mx = ds.search_threshold_top(q, m, k, 0, k)
                assert ds.counter("threshold_top_calls") - c0 == 1
                assert ds.counter("threshold_top_select_calls") - s0 == (1 if k > 64 else 0)
                assert_top((s[0], d[0], c[0], t[0]), want, k, (enc, k, m, "view"))
                assert c[0] == min(len(want[0]), k) and np.all(sh[0, :c[0]] == 0) and np.all(sh[0, c[0]:] == -1)
                assert bits(mx)[0] == bits(want[1][:1])[0]
                s, d, c, t, v = r.search_threshold_top(q, m, k)
                assert_top((s[0], d[0], c[0], t[0]), want, k, (enc, k, m, "seg"))
                assert v[0] == n
    finally:
        ds.close()
        r.close()


# ------------------------------------------------------------------------------------------------
# ties: among equal scores the lowest docs win the cut
# ------------------------------------------------------------------------------------------------
def test_ties_the_cut_falls_inside_200_copies():
    dim, sim, n = 96, SIM.COSINE, 1500
    rows = synth(n, dim, 500)
    copies = np.arange(3, n, 7)[:200]
    rows[copies] = rows[copies[0]]
    q = rows[copies[0]].copy()                                    # the copies score highest: ranks 1..200
    r = LU.GpuFlatVectorsReader("v", rows, sim)
    try:
        scored = all_scores(("ties",), rows, q, sim)
        assert np.array_equal(np.sort(scored[0][:200]), copies) and len(np.unique(scored[1][:200])) == 1
        assert scored[1][200] < scored[1][0]
        for m in (NEG_INF, scored[1][0]):
            want = matches(scored, m)
            for k in (10, 70):
                s, d, c, t, _ = r.search_threshold_top(q, m, k)
                assert_top((s[0], d[0], c[0], t[0]), want, k, (m, k))
                assert np.array_equal(d[0], copies[:k])
    finally:
        r.close()


def test_ties_every_byte_row_identical():
    dim, n = 100, 300
    rows = np.ascontiguousarray(np.tile(synth(1, dim, 510, BYTE), (n, 1)))
    q = synth(1, dim, 511, BYTE)[0]
    r = LU.GpuFlatVectorsReader("v", rows, SIM.EUCLIDEAN, BYTE)
    try:
        scored = all_scores(("ties-byte",), rows, q, SIM.EUCLIDEAN)
        assert len(np.unique(scored[1])) == 1
        for k in (1, 64, 65):
            s, d, c, t, _ = r.search_threshold_top(q, scored[1][0], k)
            assert_top((s[0], d[0], c[0], t[0]), matches(scored, scored[1][0]), k, k)
            assert t[0] == n and np.array_equal(d[0], np.arange(k))
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
        for m in (NEG_INF, jth_best(scored, (n + 1) // 2), jth_best(scored, 1), jth_best(scored, n)):
            for k in (1, 64, 65):
                s, d, c, t, v = r.search_threshold_top(q, m, k)
                assert_top((s[0], d[0], c[0], t[0]), matches(scored, m), k, (n, m, k))
                assert v[0] == n
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# filters: ≈ 1 % and 50 %, dense (the compacted walk) and sparse-doc segments; an accept set without a match
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("pct", [1, 50])
def test_filtered(pct, sparse):
    dim, sim, n = 96, SIM.EUCLIDEAN, 4097
    rng = np.random.default_rng(pct)
    max_doc = 3 * n if sparse else n
    rows = synth(n, dim, 700)
    q = synth(1, dim, 701)[0]
    o2d = np.sort(rng.choice(max_doc, n, replace=False)).astype(np.int32) if sparse else None
    acc = rng.random(max_doc) < pct / 100
    r = LU.GpuFlatVectorsReader("v", rows, sim, F32, ord_to_doc=o2d, max_doc=max_doc)
    try:
        scored = all_scores(("filt", pct, sparse), rows, q, sim, o2d, acc)
        n_acc = int((acc if o2d is None else acc[o2d]).sum())
        assert scored[2] == n_acc > 0
        ab = LU.bits_from_bool(acc)
        for m in (NEG_INF, jth_best(scored, 5), jth_best(scored, max(1, n_acc // 2))):
            for k in (10, 100):
                s, d, c, t, v = r.search_threshold_top(q, m, k, ab)
                assert_top((s[0], d[0], c[0], t[0]), matches(scored, m), k, (pct, sparse, m, k))
                assert v[0] == n_acc
        # every match of the unfiltered corpus at its 10th best score is filtered out: no hit, the rest visited
        unf = all_scores(("filt-all", pct, sparse), rows, q, sim, o2d)     # (a sparse leaf's docs depend on pct)
        m = jth_best(unf, 10)
        none = np.ones(max_doc, bool)
        none[matches(unf, m)[0]] = False
        for k in (10, 100):
            s, d, c, t, v = r.search_threshold_top(q, m, k, LU.bits_from_bool(none))
            assert t[0] == 0 and c[0] == 0 and v[0] == n - len(matches(unf, m)[0])
            assert np.all(d[0] == INT32_MAX) and np.all(np.isneginf(s[0]))
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# NaN scores are never hits and never keys: totals leave them out, visited counts them
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc,dim", [(F32, 96), (BYTE, 100)], ids=["f32", "byte"])
def test_nan_scores_are_never_hits(enc, dim):
    rows = synth(1000, dim, 600, enc)
    rows[::7] = 0                                                # zero rows: NaN under COSINE
    r = LU.GpuFlatVectorsReader("v", rows, SIM.COSINE, enc)
    try:
        q = synth(1, dim, 601, enc)[0]
        scored = all_scores(("nan", enc), rows, q, SIM.COSINE)
        assert len(scored[0]) == 1000 - len(rows[::7])
        for k in (16, 1000):
            s, d, c, t, v = r.search_threshold_top(np.zeros(dim, rows.dtype), NEG_INF, k)   # a zero query
            assert t[0] == 0 and c[0] == 0 and v[0] == 1000
            assert np.all(d[0] == INT32_MAX) and np.all(np.isneginf(s[0]))
            s, d, c, t, v = r.search_threshold_top(q, NEG_INF, k)
            assert_top((s[0], d[0], c[0], t[0]), matches(scored, NEG_INF), k, k)
            assert v[0] == 1000 and not np.isnan(s[0, :c[0]]).any()
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------
# a view of 3 shards with 2–3 leaves each (sparse docs, docBases, a non-identity shardIndex): the host entry
# against the oracle's TopDocs.merge, the device entry per shard, and its keys through osk_merge_device
# ------------------------------------------------------------------------------------------------
SHARD_INDEX = [2, 0, 1]


@pytest.fixture(scope="module")
def view7():
    dim, sim = 128, SIM.COSINE
    sizes = [[700, 1, 300], [1200, 500], [64, 900]]
    segs, leaves, readers = [], [], []
    rng = np.random.default_rng(5)
    for sh, ns in enumerate(sizes):
        base, shard_leaves = 11 * sh, []
        for j, n in enumerate(ns):
            i = len(segs)
            sparse = i in (2, 4)
            max_doc = 2 * n if sparse else n
            o2d = np.sort(rng.choice(max_doc, n, replace=False)).astype(np.int32) if sparse else None
            rows = synth(n, dim, 400 + i)
            rd = LU.GpuFlatVectorsReader("v", rows, sim, F32, ord_to_doc=o2d, max_doc=max_doc)
            readers.append(rd)
            segs.append(dict(rows=rows, o2d=o2d, base=base, shard=sh, n=n))
            shard_leaves.append(LU.LeafReaderContext(j, base, rd))
            base += max_doc + 5
        leaves.append(shard_leaves)
    ds = LU.DeviceShardSet(leaves, SHARD_INDEX)
    yield dict(dim=dim, sim=sim, segs=segs, leaves=leaves, readers=readers, ds=ds, queries=synth(6, dim, 450))
    ds.close()
    for rd in readers:
        rd.close()


def shard_matches(v, qi, m):
    """Per shard every match, best first by (−score, shard-local doc)."""
    out = []
    for sh in range(3):
        d, s = [], []
        for i, sg in enumerate(v["segs"]):
            if sg["shard"] == sh:
                scored = all_scores(("view7", i, qi), sg["rows"], v["queries"][qi], v["sim"], sg["o2d"])
                dd, ss = matches(scored, m, sg["base"])
                d.append(dd)
                s.append(ss)
        d, s = np.concatenate(d), np.concatenate(s)
        order = np.lexsort((d, -s.astype(np.float64)))
        out.append((d[order], s[order]))
    return out


def view7_threshold(v, qi, j):
    s = np.concatenate([all_scores(("view7", i, qi), sg["rows"], v["queries"][qi], v["sim"], sg["o2d"])[1]
                        for i, sg in enumerate(v["segs"])])
    return np.sort(s)[::-1][j - 1]


@pytest.mark.parametrize("from_,size", [(0, 10), (5, 10), (60, 10)])
def test_view_host_entry_against_topdocs_merge(view7, from_, size):
    v = view7
    k = from_ + size
    qi = 0
    above = np.nextafter(view7_threshold(v, qi, 1), np.float32(np.inf))
    for m in (view7_threshold(v, qi, 200), view7_threshold(v, qi, 8), NEG_INF, above):
        want = shard_matches(v, qi, m)
        es, ed, esh, _, emx = O.topdocs_merge([(w[1][:k], w[0][:k]) for w in want], from_, size, SHARD_INDEX)
        s, d, sh, c, t, mx = v["ds"].search_threshold_top(v["queries"][qi], m, k, from_, size)
        n = len(ed)
        assert c[0] == n, (m, c[0], n)
        assert np.array_equal(d[0, :n], ed) and np.array_equal(sh[0, :n], esh)
        assert np.array_equal(bits(s[0, :n]), bits(es))
        assert np.all(d[0, n:] == INT32_MAX) and np.all(np.isneginf(s[0, n:])) and np.all(sh[0, n:] == -1)
        assert t[0] == sum(len(w[0]) for w in want)               # Σ of the exact totals, not of the keys returned
        if t[0] == 0:
            assert np.isnan(mx[0])
        else:
            assert bits(mx)[0] == bits(np.float32(emx)) == bits(max(w[1][0] for w in want if len(w[1])))
    assert t[0] == 0 and c[0] == 0                                # the last threshold: above the maximum


@pytest.mark.parametrize("k", [10, 70])
def test_view_device_entry_and_merge_device(view7, k):
    v = view7
    ds = v["ds"]
    qi = 1
    for m in (view7_threshold(v, qi, 150), view7_threshold(v, qi, 5), NEG_INF):
        want = shard_matches(v, qi, m)
        keys, counts, totals, visited = device_call(ds, v["queries"][qi:qi + 1], [m], k, len(v["segs"]))
        assert list(visited) == [sg["n"] for sg in v["segs"]]
        s, d = decode(keys)
        for sh in range(3):
            assert_top((s[0, sh], d[0, sh], counts[0, sh], totals[0, sh]), want[sh], k, (m, k, sh))
            assert np.all(keys[0, sh, counts[0, sh]:] == 0)
        # the keys and counts go into osk_merge_device unchanged and reproduce the host entry's page
        from_, size = 3, k - 3
        hs, hd, hsh, hc, ht, hmx = ds.search_threshold_top(v["queries"][qi], m, k, from_, size)
        d_keys = torch.from_numpy(keys.view(np.int64)).cuda()
        d_counts = torch.from_numpy(counts).cuda()
        d_si = torch.tensor(SHARD_INDEX, dtype=torch.int32, device="cuda")
        o_s = torch.empty((1, size), dtype=torch.float32, device="cuda")
        o_d = torch.empty((1, size), dtype=torch.int32, device="cuda")
        o_sh = torch.empty((1, size), dtype=torch.int32, device="cuda")
        o_c = torch.empty(1, dtype=torch.int32, device="cuda")
        o_t = torch.empty(1, dtype=torch.int64, device="cuda")
        o_m = torch.empty(1, dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().osk_merge_device(0, d_keys.data_ptr(), d_counts.data_ptr(), d_si.data_ptr(), 1, 3, k,
                                               from_, size, o_s.data_ptr(), o_d.data_ptr(), o_sh.data_ptr(),
                                               o_c.data_ptr(), o_t.data_ptr(), o_m.data_ptr(), None))
        torch.cuda.synchronize()
        assert int(o_c.item()) == hc[0]
        assert np.array_equal(o_d.cpu().numpy(), hd) and np.array_equal(o_sh.cpu().numpy(), hsh)
        assert np.array_equal(bits(o_s.cpu().numpy()), bits(hs))
        assert int(o_t.item()) == int(counts.sum()) and ht[0] == int(totals.sum())   # returned hits vs matches


@pytest.mark.parametrize("k", [10, 70])
@pytest.mark.parametrize("nq", [1, 5])
def test_batches_equal_single_queries(view7, nq, k):
    v = view7
    ds = v["ds"]
    ms = np.array([view7_threshold(v, qi, j) for qi, j in zip(range(nq), [40, 1, 200, 10, 3])], np.float32)
    got = device_call(ds, v["queries"][:nq], ms, k, len(v["segs"]))
    host = ds.search_threshold_top(v["queries"][:nq], ms, k, 0, k)
    for qi in range(nq):
        one = device_call(ds, v["queries"][qi:qi + 1], ms[qi:qi + 1], k, len(v["segs"]))
        for a, b in zip(got[:3], one[:3]):
            assert np.array_equal(a[qi], b[0]), (nq, k, qi)
        assert np.array_equal(got[3], one[3])
        want = shard_matches(v, qi, ms[qi])
        s, d = decode(got[0][qi])
        for sh in range(3):
            assert_top((s[sh], d[sh], got[1][qi, sh], got[2][qi, sh]), want[sh], k, (nq, k, qi, sh))
        host1 = ds.search_threshold_top(v["queries"][qi], ms[qi], k, 0, k)
        for a, b in zip(host, host1):
            assert np.array_equal(np.ascontiguousarray(a[qi:qi + 1]).view(np.uint8), b.view(np.uint8)), (nq, k, qi)


def test_old_entries_are_undisturbed(view7):
    v = view7
    ds = v["ds"]
    q = v["queries"][:3]
    before = ds.search(q, 10, 0, 10)
    m = view7_threshold(v, 2, 30)
    thr_before = ds.search_threshold(v["queries"][2], m, None, 64)
    c0, t0 = ds.counter("threshold_calls"), ds.counter("threshold_top_calls")
    ds.search_threshold_top(q, m, 10, 0, 10)
    ds.search_threshold_top(q, NEG_INF, 100, 0, 10)
    device_call(ds, q, [m] * 3, 10, len(v["segs"]))
    assert ds.counter("threshold_calls") == c0 and ds.counter("threshold_top_calls") - t0 == 3
    after = ds.search(q, 10, 0, 10)
    thr_after = ds.search_threshold(v["queries"][2], m, None, 64)
    for a, b in list(zip(before, after)) + list(zip(thr_before, thr_after)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert ds.counter("threshold_calls") - c0 == 1
    # ...and equal their references: the positional entry's hits in doc order, the k-NN entry's merged top 10
    want = shard_matches(v, 2, m)
    d, s, c, t = thr_after
    for sh in range(3):
        by_doc = np.argsort(want[sh][0])
        assert t[0, sh] == c[0, sh] == len(by_doc) and np.array_equal(d[0, sh, :c[0, sh]], want[sh][0][by_doc])
        assert np.array_equal(bits(s[0, sh, :c[0, sh]]), bits(want[sh][1][by_doc]))
    for qi in range(3):
        every = shard_matches(v, qi, NEG_INF)
        es, ed, esh, _, _ = O.topdocs_merge([(w[1][:10], w[0][:10]) for w in every], 0, 10, SHARD_INDEX)
        assert np.array_equal(after[1][qi], ed) and np.array_equal(after[2][qi], esh)
        assert np.array_equal(bits(after[0][qi]), bits(es))


# ------------------------------------------------------------------------------------------------
# the certified int8 first pass of float32 views serves the new entries too, with the same keys and totals
# ------------------------------------------------------------------------------------------------
def _int8_case(ds, q, ms, k):
    keys, counts, totals, _ = device_call(ds, q, ms, k, 1)
    return keys, counts, totals


@pytest.mark.parametrize("k", [10, 100])
def test_int8_first_pass(k):
    dim, sim, n = 768, SIM.COSINE, 4097
    rows = synth(n, dim, 1300)
    q = synth(3, dim, 1301)
    scored = [all_scores(("int8", i), rows, q[i], sim) for i in range(3)]
    ms = np.array([jth_best(scored[0], 10), jth_best(scored[1], 500), jth_best(scored[2], 1)], np.float32)
    results = []
    for testing, all_maybe in ((False, 0), (True, 1)):
        with (_lib.testing() if testing else contextlib.nullcontext()):
            r = LU.GpuFlatVectorsReader("v", rows, sim)
            ds = LU.DeviceShardSet([[LU.LeafReaderContext(0, 0, r)]], [0])
            try:
                c0 = ds.counter("threshold_sq8_calls")
                with (knob("thr_sq8_all_maybe", 1, 0) if all_maybe else contextlib.nullcontext()):
                    s0 = ds.counter("threshold_sq8_settled_rows")
                    results.append(_int8_case(ds, q, ms, k))
                    if all_maybe:                                 # the settle, not the int8 pass, decided the rows
                        assert ds.counter("threshold_sq8_settled_rows") - s0 >= int(results[0][2].sum())
                assert ds.counter("threshold_sq8_calls") - c0 == 1
                if not testing:
                    with knob("thr_sq8", 0, 1):
                        results.append(_int8_case(ds, q, ms, k))
                    assert ds.counter("threshold_sq8_calls") - c0 == 1
            finally:
                ds.close()
                r.close()
    for got in results:
        for a, b in zip(got, results[0]):
            assert np.array_equal(a, b)
    keys, counts, totals = results[0]
    s, d = decode(keys)
    for i in range(3):
        assert_top((s[i, 0], d[i, 0], counts[i, 0], totals[i, 0]), matches(scored[i], ms[i]), k, i)


# ------------------------------------------------------------------------------------------------
# the Python query classes: the shard's query phase collects on the device
# ------------------------------------------------------------------------------------------------
def _view_of(query, leaves):
    e = LU._GpuKnnVectorQuery._acquire_view(query, leaves)
    LU._GpuKnnVectorQuery._release_view(e)
    return e.view


@pytest.mark.parametrize("enc,dim,sim", [(F32, 128, SIM.COSINE), (BYTE, 100, SIM.DOT_PRODUCT)], ids=["f32", "byte"])
def test_query_classes(enc, dim, sim):
    sizes = [2000, 1, 700]
    rows = [synth(n, dim, 900 + i, enc) for i, n in enumerate(sizes)]
    q = synth(1, dim, 950, enc)[0]
    readers = [LU.GpuFlatVectorsReader("v", rw, sim, enc) for rw in rows]
    bases = [3, 2010, 2020]
    leaves = [LU.LeafReaderContext(i, bases[i], readers[i]) for i in range(3)]
    cpu_cls, gpu_cls = ((LU.FloatVectorSimilarityQuery, LU.GpuFloatVectorSimilarityQuery) if enc == F32 else
                        (LU.ByteVectorSimilarityQuery, LU.GpuByteVectorSimilarityQuery))
    knn_cls = LU.GpuKnnFloatVectorQuery if enc == F32 else LU.GpuKnnByteVectorQuery
    live = [np.random.default_rng(9).random(2000) < 0.9, None, None]
    for lf, l in zip(leaves, live):
        lf.live_docs = l
    try:
        flt = lambda leaf: (np.arange(leaf.max_doc) % 2 == 0) if leaf.max_doc > 1 else np.ones(1, bool)   # noqa: E731
        accept = [live[0] & flt(leaves[0]), flt(leaves[1]), flt(leaves[2])]
        scored = [all_scores(("qc", enc, i), rows[i], q, sim, None, accept[i]) for i in range(3)]
        every = np.sort(np.concatenate([s[1] for s in scored]))[::-1]
        for j in (40, 7):                                          # more matches than the window; fewer (k > total)
            m = float(every[j - 1])
            total = int((every >= np.float32(m)).sum())
            for from_, size in ((0, 10), (5, 10)):
                gpu = gpu_cls("v", q, m, m, flt)
                view = _view_of(gpu, leaves)
                c0, t0 = view.counter("threshold_calls"), view.counter("threshold_top_calls")
                a = LU.shard_query_phase(cpu_cls("v", q, m, m, flt), leaves, from_, size)
                b = LU.shard_query_phase(gpu, leaves, from_, size)
                assert view.counter("threshold_top_calls") - t0 == 1 and view.counter("threshold_calls") == c0
                assert a.total_hits.value == b.total_hits.value == total
                assert b.total_hits.relation == LU.Relation.EQUAL_TO
                assert len(b.score_docs) == min(total, from_ + size)
                assert [h.doc for h in a.score_docs] == [h.doc for h in b.score_docs]
                assert np.array_equal(bits(np.array([h.score for h in a.score_docs], np.float32)),
                                      bits(np.array([h.score for h in b.score_docs], np.float32)))
        # a window above OSK_MAX_K takes the old route: rewrite (the positional entry) and a host sort
        m = float(every[39])
        gpu = gpu_cls("v", q, m, m, flt)
        view = _view_of(gpu, leaves)
        c0, t0 = view.counter("threshold_calls"), view.counter("threshold_top_calls")
        b = LU.shard_query_phase(gpu, leaves, 1, _lib.OSK_MAX_K)
        a = LU.shard_query_phase(cpu_cls("v", q, m, m, flt), leaves, 1, _lib.OSK_MAX_K)
        assert view.counter("threshold_calls") - c0 >= 1 and view.counter("threshold_top_calls") == t0
        assert [(h.doc, h.score) for h in a.score_docs] == [(h.doc, h.score) for h in b.score_docs]
        assert a.total_hits.value == b.total_hits.value == int((every >= np.float32(m)).sum())
        # a threshold at the 10th best score is the k-NN query's top 10 (distinct scores around the cut)
        if len(np.unique(every[:11])) == 11:
            m = float(every[9])
            knn = LU.shard_query_phase(knn_cls("v", q, 10, flt), leaves, 0, 10)
            sim_ = LU.shard_query_phase(gpu_cls("v", q, m, m, flt), leaves, 0, 10)
            assert sim_.total_hits.value == 10
            assert [(h.doc, h.score) for h in sim_.score_docs] == [(h.doc, h.score) for h in knn.score_docs]
        else:
            assert enc == BYTE                                     # (integer dot products tie; float32 must not)
    finally:
        for lf in leaves:
            lf.live_docs = None
        LU._GpuKnnVectorQuery.release_views()
        for rd in readers:
            rd.close()


# ------------------------------------------------------------------------------------------------
# Hamming fields are refused by all three entries, before the device is touched, and stay usable
# ------------------------------------------------------------------------------------------------
def test_hamming_is_refused_and_stays_usable():
    n, dim = 3000, 16
    rows = np.random.default_rng(66).integers(-128, 128, (n, dim), dtype=np.int8)
    queries = rows[:2].copy()
    r = LU.GpuBinaryVectorsReader("v", rows)
    ds = LU.DeviceShardSet([[LU.LeafReaderContext(0, 0, r)]], [0])
    try:
        before = r.search_batch(queries, 10)
        for call in (lambda: r.search_threshold_top(queries, 0.5, 10),
                     lambda: ds.search_threshold_top(queries, 0.5, 10, 0, 10)):
            with pytest.raises(_lib.OskError) as e:
                call()
            assert e.value.code == _lib.OSK_ERR_UNSUPPORTED and "Hamming" in str(e.value), str(e.value)
        one = torch.zeros(64, dtype=torch.int64, device="cuda")
        p = one.data_ptr()
        rc = _lib.lib().osk_view_search_threshold_top_device(ds.handle, p, 1, p, 10, None, p, p, p, None, None)
        assert rc == _lib.OSK_ERR_UNSUPPORTED and b"Hamming" in _lib.lib().osk_last_error()
        torch.cuda.synchronize()
        assert int(one.abs().sum().item()) == 0                    # nothing written
        after = r.search_batch(queries, 10)
        for a, b in zip(before, after):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert np.all(after[1][:, 0] == [0, 1])                   # each query is its own row: distance 0
        s, d, sh, c, t, _ = ds.search(queries, 10, 0, 10)
        assert np.all(c == 10) and np.array_equal(d, after[1])
    finally:
        ds.close()
        r.close()
