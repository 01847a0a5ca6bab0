"""Nested k-NN of float32 views through the certified int8 first pass: `nest_scan_sq8` reads the
int8 copy once and leaves every accepted row's upper bound and every family's best lower bound LBp; the shard's
floor T is its k-th best LBp; `nest_settle_f32` re-scores exactly the rows with ub ≥ T and ub ≥ LBp of their
family.  Results must not change: docs, score bits, counts, visited and the unused-slot sentinels equal the fp32
path's and the reference's, with no tolerance.

Reference, as test_gpu_nested.py states it (its helpers are imported): `oracle.exact_search(k = n_rows,
ORDER_DEVICE)`, best row per parent, sorted, cut to k.  Every case runs with the knob `nest_sq8` at 1 and at 0, the
two must agree bit for bit, and the delta of the view's `nested_sq8_calls` says which path ran (a silent fallback
to the fp32 scan would pass everything else).
"""
import contextlib

import numpy as np
import pytest

import bounds_inputs as BI
from opensearch_amd import _lib, lucene as LU
from oracle import bounds_reference as BR
from oracle import oracle as O
from test_gpu_nested import all_scores, assert_result, families, nested_reference, parent_mask, synth

pytestmark = pytest.mark.gpu

SIM = LU.VectorSimilarityFunction
F32 = LU.VectorEncoding.FLOAT32
INT32_MAX = 2**31 - 1


@contextlib.contextmanager
def knob(key, value, default):
    _lib.tune(key, value)
    try:
        yield
    finally:
        _lib.tune(key, default)


def same_bits(a, b, ctx=""):
    for x, y in zip(a, b):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), ctx


def both_paths(ds, fn, new_path=True, ctx=""):
    """fn() with nest_sq8 = 1 and = 0: the results agree bit for bit; the view's counter says which path ran."""
    c0 = ds.counter("nested_sq8_calls")
    got = fn()
    took = ds.counter("nested_sq8_calls") - c0
    assert (took == 1) if new_path else (took == 0), (ctx, took)
    with knob("nest_sq8", 0, 1):
        old = fn()
        assert ds.counter("nested_sq8_calls") - c0 == took, ctx
    same_bits(got, old, ctx)
    return got


def device_call(ds, q, k, accept=None):
    """osk_view_search_nested_device: (scores[nq, S, k], docs, counts[nq, S], visited[n_segs])."""
    import torch
    q = np.ascontiguousarray(np.atleast_2d(q), np.float32)
    nq, S, n_segs = len(q), ds.n_shards, len(ds.leaves)
    tq = torch.from_numpy(q).cuda()
    keys = torch.full((nq, S, k), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((nq, S), -7, dtype=torch.int32, device="cuda")
    visited = torch.full((n_segs,), -7, dtype=torch.int64, device="cuda")
    keep, table = [], None
    if accept is not None:
        for a in accept:
            keep.append(None if a is None else torch.from_numpy(LU.bits_from_bool(a).view(np.int64)).cuda())
        table = torch.tensor([0 if t is None else t.data_ptr() for t in keep], dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        _lib.check(_lib.lib().osk_view_search_nested_device(
            ds.handle, tq.data_ptr(), nq, k, None if table is None else table.data_ptr(), keys.data_ptr(),
            counts.data_ptr(), visited.data_ptr(), st.cuda_stream))
    st.synchronize()
    s, d = LU.decode_keys(keys.cpu().numpy().view(np.uint64))
    return s, d, counts.cpu().numpy(), visited.cpu().numpy()


class Leaf1:
    """One reader with its parents and the single-leaf view over it (the view carries the counters)."""

    def __init__(self, rows, sim, o2d, parents, max_doc):
        self.r = LU.GpuFlatVectorsReader("v", rows, sim, F32, ord_to_doc=o2d, max_doc=max_doc)
        self.r.set_parents(parent_mask(parents, max_doc))
        self.ds = LU.DeviceShardSet([[LU.LeafReaderContext(0, 0, self.r)]], [0])

    def close(self):
        self.ds.close()
        self.r.close()

    def search(self, q, k, accept=None, new_path=True, ctx=""):
        """The device entry on both paths: (scores[nq, k], docs[nq, k], counts[nq], visited)."""
        acc = None if accept is None else [accept]
        s, d, c, v = both_paths(self.ds, lambda: device_call(self.ds, q, k, acc), new_path, ctx)
        return s[:, 0], d[:, 0], c[:, 0], int(v[0])

    def settled(self):
        return self.ds.counter("nested_sq8_settled_rows")


@contextlib.contextmanager
def leaf1(*a):
    v = Leaf1(*a)
    try:
        yield v
    finally:
        v.close()


def check_queries(v, qs, k, scored, parents, n_vis, accept=None, new_path=True, ctx=()):
    s, d, c, vis = v.search(qs, k, accept, new_path, ctx)
    for i in range(len(scored)):
        assert_result((s[i], d[i], c[i]), nested_reference(scored[i][0], scored[i][1], parents, k), k, ctx + (k, i))
    assert vis == n_vis, (ctx, vis, n_vis)
    return s, d, c


# ------------------------------------------------------------------------------------------------
# 1. every pair of float32 and int8 lane config (50, 1000 and 2048 are the dims whose rows per step differ), four
#    similarities, a sparse field with families of 1 … 300 rows, k ∈ {1, 10, 64}, a 9-query call (passes of 4, 4
#    and 1) and a single query.
# 9. the certificate is worth having: on these unit-norm rows at k = 10, dims ≤ 1030, a query settles at most 10 %
#    of the rows (tests/test_nested_sq8_cpu.py derives the bound on the input from the inequality alone).
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", list(SIM), ids=lambda s: s.name)
@pytest.mark.parametrize("dim", [7, 50, 96, 128, 768, 1000, 1030, 2048, 4096])
def test_lane_config_pairs(dim, sim):
    n = 4097
    rows = synth(n, dim, 100 + dim)
    qs = synth(9, dim, 7 + dim)
    o2d, parents, max_doc = families(n, 11)
    assert {int(f) for f in np.diff(np.concatenate([[-1], parents])) - 1} >= {1, 2, 3, 5, 17, 64, 65, 300}
    scored = [all_scores(("sq8lane", dim, sim, i), rows, qs[i], sim, o2d) for i in range(9)]
    with leaf1(rows, sim, o2d, parents, max_doc) as v:
        for k in (1, 10, 64):
            check_queries(v, qs, k, scored, parents, n, ctx=(dim, sim))
            check_queries(v, qs[3], k, scored[3:4], parents, n, ctx=(dim, sim, "single"))
        if dim <= 1030:
            for i in range(9):
                s0 = v.settled()
                device_call(v.ds, qs[i], 10)
                settled = v.settled() - s0
                print(f"dim {dim} {sim.name} query {i}: settled {settled} of {n} rows")
                assert 10 <= settled <= 0.10 * n, (dim, sim, i, settled)


# ------------------------------------------------------------------------------------------------
# 2. row counts at the edges of a 64-row window and of one wave's range (256 rows: 64 per wave in every lane
#    config), degenerate families
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 129, 255, 256, 257])
def test_row_counts_at_edges(n):
    dim, sim = 96, SIM.EUCLIDEAN
    rows = synth(n, dim, 300 + n)
    qs = synth(2, dim, 301)
    o2d, parents, max_doc = families(n, n, sizes=(1, 2, 3, 5))
    scored = [all_scores(("sq8edge", n, i), rows, qs[i], sim, o2d) for i in range(2)]
    with leaf1(rows, sim, o2d, parents, max_doc) as v:
        for k in (1, 10, 64):
            check_queries(v, qs, k, scored, parents, n, ctx=(n,))
            check_queries(v, qs[1], k, scored[1:], parents, n, ctx=(n, "single"))


def test_every_row_its_own_parent_equals_knn():
    n, dim, sim = 4097, 96, SIM.EUCLIDEAN
    rows = synth(n, dim, 200)
    qs = synth(3, dim, 201)
    with leaf1(rows, sim, None, np.arange(n), n) as v:
        for k in (1, 10, 64):
            s, d, c, vis = v.search(qs, k)
            bs, bd, bc, bv = v.r.search_batch(qs, k)
            same_bits((s, d, c), (bs, bd, bc), k)
            assert vis == n and np.all(bv == n)


def test_one_family_of_all_rows():
    n, dim, sim = 4097, 96, SIM.COSINE
    rows = synth(n, dim, 210)
    q = synth(1, dim, 211)
    scored = [all_scores(("sq8onefam",), rows, q[0], sim)]
    with leaf1(rows, sim, np.arange(n, dtype=np.int32), np.array([n], np.int32), n + 1) as v:
        for k in (1, 10, 64):
            s, d, c = check_queries(v, q, k, scored, [n], n)
            assert c[0] == 1 and s[0, 0] == scored[0][1].max()


def test_fewer_families_than_k():
    """T = 0: the floor rejects nothing, a row is settled when its ub reaches its own family's LBp."""
    n, dim, sim = 700, 96, SIM.MAXIMUM_INNER_PRODUCT
    rows = synth(n, dim, 220)
    q = synth(1, dim, 221)
    o2d, parents, max_doc = families(n, 3, sizes=(65, 300))
    assert 1 < len(parents) < 10
    scored = [all_scores(("sq8fewer",), rows, q[0], sim, o2d)]
    with leaf1(rows, sim, o2d, parents, max_doc) as v:
        s, d, c = check_queries(v, q, 10, scored, parents, n)
        assert c[0] == len(parents)
        s0 = v.settled()
        device_call(v.ds, q, 10)
        assert len(parents) <= v.settled() - s0 <= n


# ------------------------------------------------------------------------------------------------
# 3. ties
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [SIM.EUCLIDEAN, SIM.DOT_PRODUCT], ids=lambda s: s.name)
def test_duplicates_inside_a_family_and_across_families_at_rank_k(sim):
    dim, n = 96, 640
    rows = synth(n, dim, 500)
    q = rows[3].copy()                       # unit rows: row 3 and its copies score highest
    rows[1] = rows[5] = rows[6] = rows[3]    # families of 4: rows 1, 3 in family 0, rows 5, 6 in family 1
    o2d, parents, max_doc = families(n, 0, sizes=(4,))
    scored = [all_scores(("sq8ties", sim), rows, q, sim, o2d)]
    top = np.sort(scored[0][1])[::-1]
    assert top[3] == top[0] > top[4]
    with leaf1(rows, sim, o2d, parents, max_doc) as v:
        for k, want_docs in ((1, [o2d[1]]), (2, [o2d[1], o2d[5]]), (10, None)):
            s, d, c = check_queries(v, q[None], k, scored, parents, n, ctx=(sim,))
            if want_docs:                    # the lower doc of a family, the families in doc order
                assert d[0, :k].tolist() == want_docs and np.all(s[0, :k] == top[0])
    # the same row in families 7 and 30, placed so that it is the k-th best family's child: the k-th place goes to
    # the lower doc, the (k + 1)-th to the other
    rows2 = synth(n, dim, 501)
    q2 = synth(1, dim, 502)[0]
    sc = all_scores(("sq8ties2pre", sim), rows2, q2, sim, o2d)
    bd, bs = nested_reference(sc[0], sc[1], parents, 10)
    dup = rows2[np.searchsorted(o2d, bd[9])].copy()
    taken = set(np.searchsorted(parents, bd, side="left").tolist())
    free = [p for p in range(len(parents)) if p not in taken][:1]
    rows2[4 * free[0] + 2] = dup
    scored2 = [all_scores(("sq8ties2", sim), rows2, q2, sim, o2d)]
    wd, ws = nested_reference(scored2[0][0], scored2[0][1], parents, 11)
    assert ws[9] == ws[10] and wd[9] < wd[10]
    with leaf1(rows2, sim, o2d, parents, max_doc) as v:
        for k in (10, 11):
            check_queries(v, q2[None], k, scored2, parents, n, ctx=(sim, "rank k"))


@pytest.mark.parametrize("sim", [SIM.EUCLIDEAN, SIM.DOT_PRODUCT], ids=lambda s: s.name)
def test_the_whole_corpus_one_repeated_row(sim):
    dim, n = 96, 4097
    row = synth(1, dim, 510)
    rows = np.repeat(row, n, axis=0)
    qs = synth(2, dim, 511)
    o2d, parents, max_doc = families(n, 13)
    scored = [all_scores(("sq8same", sim, i), rows, qs[i], sim, o2d) for i in range(2)]
    with leaf1(rows, sim, o2d, parents, max_doc) as v:
        for k in (1, 10, 64):
            s, d, c = check_queries(v, qs, k, scored, parents, n, ctx=(sim,))
            first = np.concatenate([[0], parents[:-1] + 1])[:k]       # every family's first child, in doc order
            assert c[0] == len(first) and d[0, :c[0]].tolist() == first.tolist()


# ------------------------------------------------------------------------------------------------
# 4. COSINE with degenerate norms: a zero child is visited, never a best child; a family whose only child is zero
#    is absent; a zero query has no hit
# ------------------------------------------------------------------------------------------------
def test_cosine_zero_children_and_zero_query():
    n, dim, sim = 4097, 96, SIM.COSINE
    rows = synth(n, dim, 600)
    rows[::7] = 0
    rows[8:12] = 0                            # family 2 entirely
    o2d, parents, max_doc = families(n, 0, sizes=(4,))
    qs = synth(2, dim, 601)
    scored = [all_scores(("sq8nan", i), rows, qs[i], sim, o2d) for i in range(2)]
    assert len(scored[0][0]) == n - len(set(range(0, n, 7)) | set(range(8, 12)))
    with leaf1(rows, sim, o2d, parents, max_doc) as v:
        for k in (1, 10, 64):
            s, d, c = check_queries(v, qs, k, scored, parents, n)
            assert not np.isnan(s[0, :c[0]]).any()
        s, d, c, vis = v.search(qs[0], len(parents) if len(parents) <= 64 else 64)
        assert not set(d[0, :c[0]].tolist()) & set(o2d[8:12].tolist())
        s, d, c, vis = v.search(np.zeros((1, dim), np.float32), 10)
        assert c[0] == 0 and vis == n and np.all(d[0] == INT32_MAX) and np.all(np.isneginf(s[0]))
        mixed = np.stack([qs[0], np.zeros(dim, np.float32), qs[1]])         # a zero query inside a pass
        s, d, c, vis = v.search(mixed, 10)
        assert c[1] == 0
        assert_result((s[0], d[0], c[0]), nested_reference(scored[0][0], scored[0][1], parents, 10), 10)
        assert_result((s[2], d[2], c[2]), nested_reference(scored[1][0], scored[1][1], parents, 10), 10)
    small_n = 200                             # fewer families than 64: the family of zeros is the one that is absent
    o2d, parents, max_doc = families(small_n, 0, sizes=(4,))
    sc = [all_scores(("sq8nan-small",), rows[:small_n], qs[0], sim, o2d)]
    with leaf1(rows[:small_n], sim, o2d, parents, max_doc) as v:
        s, d, c = check_queries(v, qs[:1], 64, sc, parents, small_n)
        assert c[0] == len(parents) - 1 == 49


# ------------------------------------------------------------------------------------------------
# 5. filters: ≈ 1 %, 50 %, nothing, all ones; a sparse field and a dense one (the compacted walk); some families
#    rejected entirely
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("pct", [1, 50, 0, 100])
def test_filtered(pct, sparse):
    dim, sim, n = 96, SIM.EUCLIDEAN, 4097
    rows = synth(n, dim, 700)
    qs = synth(5, dim, 701)
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
    n_acc = int(acc[o2d].sum()) if sparse else int(acc.sum())
    with leaf1(rows, sim, o2d, parents, max_doc) as v:
        if pct == 0:
            s, d, c, vis = v.search(qs, 10, acc)
            assert vis == 0 and np.all(c == 0) and np.all(d == INT32_MAX) and np.all(np.isneginf(s))
            return
        scored = [all_scores(("sq8filt", pct, sparse, i), rows, qs[i], sim, o2d, acc) for i in range(5)]
        assert scored[0][2] == n_acc > 0
        for k in (1, 10, 64):
            check_queries(v, qs, k, scored, parents, n_acc, acc, ctx=(pct, sparse))
            check_queries(v, qs[2], k, scored[2:3], parents, n_acc, acc, ctx=(pct, sparse, "single"))
        # an unfiltered call after a filtered one, and back: no record of the other call survives
        plain = [all_scores(("sq8filt-plain", sparse, i), rows, qs[i], sim, o2d) for i in range(2)]
        check_queries(v, qs[:2], 10, plain, parents, n, ctx=("after a filter",))
        check_queries(v, qs[:2], 10, scored[:2], parents, n_acc, acc, ctx=("filter again",))


# ------------------------------------------------------------------------------------------------
# 6. a view of 4 segments in 2 shards (one sparse segment, one 0-row segment, non-zero doc bases) through the
#    segment, host and device entries, against oracle.topdocs_merge with from / size; a mixed accept table
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def view4():
    dim, sim = 200, SIM.COSINE
    sizes = [3000, 0, 1, 4097]
    shard_of = [0, 0, 0, 1]
    max_doc = [3000, 40, 1, 9000]
    rows = [synth(n, dim, 400 + i) if n else np.zeros((0, dim), np.float32) for i, n in enumerate(sizes)]
    rng = np.random.default_rng(5)
    o2d = [None, None, None, np.sort(rng.choice(8999, sizes[3], replace=False)).astype(np.int32)]
    free = np.setdiff1d(np.arange(8999), o2d[3])
    parents = [np.union1d(np.arange(4, 3000, 5), [2999]).astype(np.int32), np.array([39], np.int32),
               np.array([0], np.int32), np.union1d(rng.choice(free, 1200, replace=False), [8999]).astype(np.int32)]
    bases = [3, 3013, 3060, 17]
    readers = [LU.GpuFlatVectorsReader("v", rows[i], sim, F32, ord_to_doc=o2d[i], max_doc=max_doc[i]) for i in range(4)]
    for r, p, m in zip(readers, parents, max_doc):
        r.set_parents(parent_mask(p, m))
    leaves = [[LU.LeafReaderContext(i, bases[i], readers[i]) for i in range(3)], [LU.LeafReaderContext(0, bases[3], readers[3])]]
    ds = LU.DeviceShardSet(leaves, [0, 1])
    accepts = {None: None, "mixed": [rng.random(3000) < 0.5, None, None, None],
               "mixed2": [None, None, None, rng.random(9000) < 0.3]}
    yield dict(dim=dim, sim=sim, rows=rows, o2d=o2d, max_doc=max_doc, bases=bases, readers=readers, ds=ds,
               queries=synth(9, dim, 450), shard_of=shard_of, parents=parents, accepts=accepts)
    ds.close()
    for r in readers:
        r.close()


def view4_reference(v, qi, k, aname=None):
    """Per shard the k best families (shard-local child docs, scores) + visited per segment."""
    accept = v["accepts"][aname]
    per_shard, visited = [[], []], []
    for i in range(4):
        acc = None if accept is None else accept[i]
        if len(v["rows"][i]) == 0:
            visited.append(0)
            continue
        d, s, vis = all_scores(("sq8view4", i, qi, aname if acc is not None else None), v["rows"][i], v["queries"][qi],
                               v["sim"], v["o2d"][i], acc)
        bd, bs = nested_reference(d, s, v["parents"][i], k)
        per_shard[v["shard_of"][i]].append((bd + v["bases"][i], bs))
        visited.append(vis)
    out = []
    for ps in per_shard:
        d, s = np.concatenate([p[0] for p in ps]), np.concatenate([p[1] for p in ps])
        order = np.lexsort((d, -s.astype(np.float64)))[:k]
        out.append((d[order], s[order]))
    return out, visited


@pytest.mark.parametrize("aname", [None, "mixed", "mixed2"])
def test_view_entries(view4, aname):
    v, ds = view4, view4["ds"]
    accept = v["accepts"][aname]
    for qi, k in ((0, 10), (1, 64), (2, 1)):
        want, visited = view4_reference(v, qi, k, aname)
        ctx = (aname, qi, k)
        q = v["queries"][qi]
        s, d, c, vis = both_paths(ds, lambda: device_call(ds, q, k, accept), True, ctx)
        for sh in range(2):
            assert_result((s[0, sh], d[0, sh], c[0, sh]), want[sh], k, ("device", sh) + ctx)
        assert list(vis) == visited
        for from_, size in ((0, 10), (3, 5)):
            ws, wd, wsh, wtot, wmax = O.topdocs_merge([(w[1], w[0]) for w in want], from_, size, [0, 1])
            hs, hd, hsh, hc, htot, hmax = both_paths(ds, lambda: ds.search_nested(q, k, from_, size, accept=accept), True, ctx)
            n = len(wd)
            assert hc[0] == n and htot[0] == wtot and (n == 0 or hmax[0] == np.float32(wmax))
            assert np.array_equal(hd[0, :n], wd) and np.array_equal(hsh[0, :n], wsh)
            assert np.array_equal(hs[0, :n].view(np.uint32), ws.view(np.uint32))
        for i in (0, 3):                                    # the dense and the sparse segment's own entry
            acc = None if accept is None else accept[i]
            d_, s_, vis_ = all_scores(("sq8view4", i, qi, aname if acc is not None else None), v["rows"][i], q, v["sim"],
                                      v["o2d"][i], acc)
            bits = None if acc is None else LU.bits_from_bool(acc)
            got = v["readers"][i].search_nested(q, k, bits)
            with knob("nest_sq8", 0, 1):
                same_bits(got, v["readers"][i].search_nested(q, k, bits), ("seg",) + ctx)
            assert_result((got[0][0], got[1][0], got[2][0]), nested_reference(d_, s_, v["parents"][i], k), k, ("seg", i) + ctx)
            assert got[3][0] == vis_


def test_view_batch_of_nine(view4):
    v, ds, k = view4, view4["ds"], 10
    hs, hd, hsh, hc, htot, hmax = both_paths(ds, lambda: ds.search_nested(v["queries"], k, 0, 20))
    for qi in range(9):
        want, _ = view4_reference(v, qi, k)
        ws, wd, wsh, wtot, wmax = O.topdocs_merge([(w[1], w[0]) for w in want], 0, 20, [0, 1])
        n = len(wd)
        assert hc[qi] == n and htot[qi] == wtot
        assert np.array_equal(hd[qi, :n], wd) and np.array_equal(hsh[qi, :n], wsh), qi
        assert np.array_equal(hs[qi, :n].view(np.uint32), ws.view(np.uint32)), qi


# ------------------------------------------------------------------------------------------------
# 7. the certificate's range
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [SIM.EUCLIDEAN, SIM.COSINE], ids=lambda s: s.name)
def test_a_row_out_of_range_keeps_the_fp32_kernels(sim):
    n, dim = 4097, 96
    rows = synth(n, dim, 800)
    rows[1234] *= np.float32(2.0 ** 60)
    q = synth(1, dim, 801)
    o2d, parents, max_doc = families(n, 14)
    scored = [all_scores(("sq8rowrange", sim), rows, q[0], sim, o2d)]
    with leaf1(rows, sim, o2d, parents, max_doc) as v:
        # the first call builds the int8 copy and finds the row: no call of this view takes the int8 pass
        c0, s0 = v.ds.counter("nested_sq8_calls"), v.settled()
        for k in (1, 10):
            check_queries(v, q, k, scored, parents, n, new_path=False, ctx=(sim,))
        assert v.ds.counter("nested_sq8_calls") == c0 and v.settled() == s0


@pytest.mark.parametrize("sim", list(SIM), ids=lambda s: s.name)
def test_a_query_out_of_range_settles_every_accepted_row(sim):
    n, dim = 4097, 96
    rows = synth(n, dim, 810)
    qs = synth(2, dim, 811)
    qs[1] *= np.float32(2.0 ** 60)
    o2d, parents, max_doc = families(n, 15)
    acc = np.random.default_rng(8).random(max_doc) < 0.5
    with leaf1(rows, sim, o2d, parents, max_doc) as v:
        for accept, n_acc in ((None, n), (acc, int(acc[o2d].sum()))):
            scored = [all_scores(("sq8qrange", sim, accept is None), rows, qs[1], sim, o2d, accept)]
            check_queries(v, qs[1:], 10, scored, parents, n_acc, accept, ctx=(sim,))
            s0, c0 = v.settled(), v.ds.counter("nested_sq8_calls")
            device_call(v.ds, qs[1], 10, None if accept is None else [accept])
            assert v.ds.counter("nested_sq8_calls") - c0 == 1
            assert v.settled() - s0 == n_acc
            # in one pass with an in-range query: that one still settles few rows
            s0 = v.settled()
            device_call(v.ds, qs, 10, None if accept is None else [accept])
            assert n_acc < v.settled() - s0 < 2 * n_acc


# ------------------------------------------------------------------------------------------------
# 8. the settle earns its result (testing build): with nest_sq8_all_settle every row that has a record is
#    re-scored and nothing changes; without it the rows re-scored are exactly those the three conditions name,
#    computed here from the pass's records, and every winner of the reference is among them
# ------------------------------------------------------------------------------------------------
def records(ds, n_rows, n_parents):
    ub = BI.debug_copy(ds, "nest_ub", n_rows, np.uint32)
    lbkey = BI.debug_copy(ds, "nest_lbkey", n_parents, np.uint64)
    return ub, (lbkey >> np.uint64(32)).astype(np.uint32)


@pytest.mark.parametrize("filtered", [False, True], ids=["all", "filtered"])
def test_all_settle_changes_nothing(filtered):
    n, dim, sim = 4097, 384, SIM.MAXIMUM_INNER_PRODUCT
    rows = synth(n, dim, 1100)
    qs = synth(4, dim, 1101)
    o2d, parents, max_doc = families(n, 16)
    acc = np.random.default_rng(4).random(max_doc) < 0.5 if filtered else None
    n_acc = int(acc[o2d].sum()) if filtered else n
    scored = [all_scores(("sq8allsettle", filtered, i), rows, qs[i], sim, o2d, acc) for i in range(4)]
    with _lib.testing(), leaf1(rows, sim, o2d, parents, max_doc) as v:
        table = None if acc is None else [acc]
        plain = device_call(v.ds, qs, 10, table)
        with knob("nest_sq8_all_settle", 1, 0):
            s0, c0 = v.settled(), v.ds.counter("nested_sq8_calls")
            forced = device_call(v.ds, qs, 10, table)
            assert v.ds.counter("nested_sq8_calls") - c0 == 1
            assert v.settled() - s0 == 4 * n_acc          # (no NaN bound among these rows)
            ub, _ = records(v.ds, n, len(parents))
            assert int((ub != 0).sum()) == n_acc
        same_bits(plain, forced)
        for i in range(4):
            assert_result((forced[0][i, 0], forced[1][i, 0], forced[2][i, 0]),
                          nested_reference(scored[i][0], scored[i][1], parents, 10), 10)
    with pytest.raises(_lib.OskError) as e:                # the shipped library refuses the knob
        _lib.tune("nest_sq8_all_settle", 1)
    assert e.value.code == _lib.OSK_ERR_UNSUPPORTED


@pytest.mark.parametrize("dim,sim", [(768, SIM.COSINE), (96, SIM.EUCLIDEAN)], ids=["768-COSINE", "96-EUCLIDEAN"])
def test_the_settle_re_scores_exactly_the_rows_of_the_three_conditions(dim, sim):
    n, k = 4097, 10
    rows = synth(n, dim, 100 + dim)
    q = synth(9, dim, 7 + dim)[3]
    o2d, parents, max_doc = families(n, 11)
    scored = all_scores(("sq8lane", dim, sim, 3), rows, q, sim, o2d)
    with _lib.testing(), leaf1(rows, sim, o2d, parents, max_doc) as v:
        s0, c0 = v.settled(), v.ds.counter("nested_sq8_calls")
        s, d, c, vis = device_call(v.ds, q, k)
        assert v.ds.counter("nested_sq8_calls") - c0 == 1
        settled = v.settled() - s0
        ub, lbp = records(v.ds, n, len(parents))
        assert np.all(ub != 0)
        pid = np.searchsorted(parents, o2d, side="left")
        have = np.sort(lbp[lbp != 0])[::-1]
        T = have[k - 1] if len(have) >= k else np.uint32(0)
        want = (ub != 0) & (ub >= T) & (ub >= lbp[pid])
        assert settled == int(want.sum()), (settled, int(want.sum()))
        assert k <= settled < n // 4
        wd, ws = nested_reference(scored[0], scored[1], parents, k)
        assert np.all(want[np.searchsorted(o2d, wd)])       # every winner's record satisfies the conditions
        assert_result((s[0, 0], d[0, 0], c[0, 0]), (wd, ws), k)
        # the records bracket the exact scores, and a family's LBp is below its best score
        exact = np.full(n, np.nan, np.float32)
        exact[np.searchsorted(o2d, scored[0])] = scored[1]
        assert np.all(BR.sortable(exact) <= ub)
        best = np.zeros(len(parents), np.uint32)
        np.maximum.at(best, pid, BR.sortable(exact))
        assert np.all(lbp <= best)
