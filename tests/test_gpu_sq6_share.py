"""GPU tests of the shared 6-bit pass (osk_sq6.hip sq6_scan_shared).

Views over one segment set with equal tile tables form a share group: each posts its single query, and the
group's streaming passes score every posted query whose tile is not done against one read of the tile.
Sharing changes which launch scans a tile for a query, never the result, so every result here is compared
bit for bit (per-shard keys = score bits and docs, and counts) with the same query with `sq6_share` 0, and
on the shards without a sparse field with the oracle.  The testing build splits a call at its shared pass
(osk_testing_sq6_post / osk_testing_sq6_resume) so that who scans what is deterministic, and
`sq6_share_limit` bounds the workgroups that serve other views.

Shapes: 60k rows of 512, 768, 1024, 1280 and 1536 dims (C = 2, 3, 4, 5, 6: every instantiation) in three ragged
segments over three shards, one with a sparse field, 40 tiles; all four similarities; k 1, 10 and 12.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from opensearch_amd import _lib, lucene as LU
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIMS = [LU.VectorSimilarityFunction(s) for s in range(4)]
COS = LU.VectorSimilarityFunction.COSINE
DOT = LU.VectorSimilarityFunction.DOT_PRODUCT
SIZES = [30_005, 1_237, 28_763]      # ragged: partial 8-row blocks, a small segment
TILES = 40
N_VIEWS = 5
P = C.c_void_p


def corpus(n, dim, sim, seed):
    dist = {0: 1, 1: 3, 2: 3, 3: 2}[int(sim)]
    return O.synth(0, n, dim, seed, dist)


@pytest.fixture(scope="module", autouse=True)
def T():
    """The whole module runs on the testing build (the split entries and sq6_share_limit live there)."""
    with _lib.testing() as t:
        t.osk_testing_sq6_post.restype = C.c_int32
        t.osk_testing_sq6_post.argtypes = [P, P, C.c_int32, P, P, P, P]
        t.osk_testing_sq6_resume.restype = C.c_int32
        t.osk_testing_sq6_resume.argtypes = [P]
        _lib.tune("sq6_probe_pct", 100)     # keep the tier whatever the calibration says (uniform EUCLIDEAN rows)
        _lib.tune("tiles_target", TILES)
        _lib.tune("sq6_share_min_tiles", 1)  # (by default only views of more than one round of workgroups share)
        try:
            yield t
        finally:
            _lib.tune("tiles_target", 0)
            _lib.tune("sq6_probe_pct", 10)
            _lib.tune("sq6_share", 1)
            _lib.tune("sq6_share_limit", -1)
            _lib.tune("sq6_share_idle", 0)
            _lib.tune("sq6_share_min_tiles", 0)
            for w in list(_worlds.values()):
                w.close()
            _worlds.clear()


class World:
    """Readers, N_VIEWS views over them (one share group), a stream per view, calibrated and attached."""

    def __init__(self, T, dim, sim, queries=None):
        self.T, self.dim, self.sim = T, dim, sim
        self.rows = [corpus(n, dim, sim, 300 + i) for i, n in enumerate(SIZES)]
        rng = np.random.default_rng(dim)
        self.docs = np.sort(rng.choice(2_000, SIZES[1], replace=False)).astype(np.int32)
        self.readers = [LU.GpuFlatVectorsReader("v", self.rows[0], sim),
                        LU.GpuFlatVectorsReader("v", self.rows[1], sim, ord_to_doc=self.docs, max_doc=2_000),
                        LU.GpuFlatVectorsReader("v", self.rows[2], sim)]
        self.views = [self.new_view() for _ in range(N_VIEWS)]
        self.streams = [torch.cuda.Stream() for _ in range(N_VIEWS)]
        self.queries = corpus(8, dim, sim, 400) if queries is None else queries
        self.dq = torch.from_numpy(self.queries).cuda()
        torch.cuda.synchronize()
        self.refs = {}
        # calibration: four probe calls, their read-back, a call that folds it; then every view's first call
        # joins the group
        for i in range(4):
            self.search(0, 0, 10)
        torch.cuda.synchronize()
        for v in range(N_VIEWS):
            self.search(v, 0, 10)
            self.search(v, 1, 10)
        assert self.views[0].counter("sq6_calls") == 6
        self.n_tiles = self.views[0].counter("scan_tiles")
        assert self.n_tiles >= 32

    def new_view(self):
        return LU.DeviceShardSet([[LU.LeafReaderContext(0, 0, r)] for r in self.readers], [2, 0, 1])

    def buffers(self, k):
        keys = torch.zeros((1, 3, k), dtype=torch.int64, device="cuda")
        counts = torch.zeros((1, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        return keys, counts

    @staticmethod
    def result(keys, counts):
        torch.cuda.synchronize()
        c = counts.cpu().numpy()[0]
        kk = keys.cpu().numpy()[0].view(np.uint64)
        return [kk[s, :c[s]].copy() for s in range(3)], c.copy()

    def search(self, v, qi, k, ds=None, stream=None, wait=True):
        keys, counts = self.buffers(k)
        view = ds if ds is not None else self.views[v]
        st = stream if stream is not None else self.streams[v]
        _lib.check(self.T.osk_view_search_device(view.handle, self.dq[qi].data_ptr(), 1, k, None, keys.data_ptr(),
                                                 counts.data_ptr(), None, st.cuda_stream))
        return self.result(keys, counts) if wait else (keys, counts)

    def post(self, v, qi, k):
        keys, counts = self.buffers(k)
        _lib.check(self.T.osk_testing_sq6_post(self.views[v].handle, self.dq[qi].data_ptr(), k, keys.data_ptr(),
                                               counts.data_ptr(), None, self.streams[v].cuda_stream))
        return keys, counts

    def resume(self, v):
        _lib.check(self.T.osk_testing_sq6_resume(self.views[v].handle))

    def reference(self, qi, k):
        """The same query with sq6_share 0: today's launches (computed once, shared by the tests)."""
        if (qi, k) not in self.refs:
            _lib.tune("sq6_share", 0)
            try:
                self.refs[(qi, k)] = self.search(0, qi, k)
            finally:
                _lib.tune("sq6_share", 1)
        return self.refs[(qi, k)]

    def tiles(self, v):
        return tuple(self.views[v].counter(n) for n in ("sq6_tiles_own", "sq6_tiles_by_others", "sq6_tiles_helped"))

    def close(self):
        torch.cuda.synchronize()
        for v in self.views:
            v.close()
        for r in self.readers:
            r.close()


_worlds = {}


def world(T, dim, sim):
    if (dim, int(sim)) not in _worlds:
        _worlds[(dim, int(sim))] = World(T, dim, sim)
    return _worlds[(dim, int(sim))]


def same(got, want):
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    for a, b in zip(got[0], want[0]):
        assert np.array_equal(a, b), (a, b)


def delta(after, before):
    return tuple(a - b for a, b in zip(after, before))


SHAPES = [(768, s) for s in SIMS] + [(512, COS), (1024, COS), (1280, DOT), (1536, DOT)]
IDS = [f"{d}-{s.name}" for d, s in SHAPES]


def check_oracle(w, qi, k, got):
    """Shards 0 and 2 hold one dense segment each: the oracle's exact search of that segment."""
    for shard in (0, 2):
        os_, od, _ = O.exact_search(w.rows[shard], w.queries[qi], k, int(w.sim), O.ORDER_DEVICE)
        s, d = LU.decode_keys(got[0][shard])
        assert np.array_equal(d, od) and np.array_equal(s.view(np.uint32), os_.view(np.uint32))


@pytest.mark.parametrize("dim,sim", SHAPES, ids=IDS)
def test_all_helped(T, dim, sim):
    """B, C and D post; A's pass scans every tile for all four; their own passes find every tile done."""
    w = world(T, dim, sim)
    n, k = w.n_tiles, 10
    before = [w.tiles(v) for v in range(4)]
    held = [w.post(v, v, k) for v in (1, 2, 3)]
    a = w.search(0, 0, k)
    for v in (1, 2, 3):
        w.resume(v)
    got = [a] + [w.result(*h) for h in held]
    after = [w.tiles(v) for v in range(4)]
    assert delta(after[0], before[0]) == (n, 0, 3 * n)
    for v in (1, 2, 3):
        assert delta(after[v], before[v]) == (0, n, 0)
    for v in range(4):
        same(got[v], w.reference(v, k))
    check_oracle(w, 1, k, got[1])


@pytest.mark.parametrize("limit", ["half", 1])
@pytest.mark.parametrize("dim,sim", [(768, COS), (512, COS), (1280, DOT), (1536, DOT)],
                         ids=["768-COSINE", "512-COSINE", "1280-DOT", "1536-DOT"])
def test_split(T, dim, sim, limit):
    """sq6_share_limit X: A serves the others in its first X workgroups only; each finishes the rest itself."""
    w = world(T, dim, sim)
    n, k = w.n_tiles, 10
    x = n // 2 if limit == "half" else 1
    _lib.tune("sq6_share_limit", x)
    try:
        before = [w.tiles(v) for v in range(4)]
        held = [w.post(v, v + 1, k) for v in (1, 2, 3)]
        a = w.search(0, 0, k)
        for v in (1, 2, 3):
            w.resume(v)
        got = [a] + [w.result(*h) for h in held]
        after = [w.tiles(v) for v in range(4)]
    finally:
        _lib.tune("sq6_share_limit", -1)
    assert delta(after[0], before[0]) == (n, 0, 3 * x)
    for v in (1, 2, 3):
        assert delta(after[v], before[v]) == (n - x, x, 0)
    same(got[0], w.reference(0, k))
    for v in (1, 2, 3):
        same(got[v], w.reference(v + 1, k))


@pytest.mark.parametrize("dim,sim", [(768, COS), (768, SIMS[0]), (1536, DOT)], ids=["768-COSINE", "768-EUCLIDEAN", "1536-DOT"])
def test_different_k_and_a_fifth_query(T, dim, sim):
    """k 1, 10 and 12 in one pass; a pass serves at most four queries, so the fifth posted is left to its own."""
    w = world(T, dim, sim)
    n = w.n_tiles
    ks = {1: 1, 2: 10, 3: 12, 4: 10}
    before = [w.tiles(v) for v in range(5)]
    held = {v: w.post(v, v, ks[v]) for v in (1, 2, 3, 4)}
    a = w.search(0, 5, 10)
    for v in (4, 1, 2, 3):
        w.resume(v)
    after = [w.tiles(v) for v in range(5)]
    assert delta(after[0], before[0]) == (n, 0, 3 * n)
    for v in (1, 2, 3):
        assert delta(after[v], before[v]) == (0, n, 0)
    assert delta(after[4], before[4]) == (n, 0, 0)
    same(a, w.reference(5, 10))
    for v in (1, 2, 3, 4):
        got = w.result(*held[v])
        same(got, w.reference(v, ks[v]))
        if v == 3:
            check_oracle(w, v, ks[v], got)


@pytest.mark.parametrize("idle", [0, 1])
def test_a_pass_with_nothing_of_its_own(T, idle):
    """Five queries posted, so B's pass leaves the fifth (E) undone and does A's for it.  A's own pass then has
    nothing of its own: by default its workgroups exit and E scans for itself; with sq6_share_idle 1 they
    scan E's tiles."""
    w = world(T, 768, COS)
    n, k = w.n_tiles, 10
    _lib.tune("sq6_share_idle", idle)
    try:
        before = [w.tiles(v) for v in range(5)]
        held = {v: w.post(v, v, k) for v in (0, 2, 3, 4)}
        b = w.search(1, 1, k)
        mid = [w.tiles(v) for v in range(5)]
        for v in (0, 4, 2, 3):
            w.resume(v)
        after = [w.tiles(v) for v in range(5)]
    finally:
        _lib.tune("sq6_share_idle", 0)
    assert delta(mid[1], before[1]) == (n, 0, 3 * n)
    assert delta(after[0], before[0]) == ((0, n, n) if idle else (0, n, 0))
    assert delta(after[4], before[4]) == ((0, n, 0) if idle else (n, 0, 0))
    for v in (2, 3):
        assert delta(after[v], before[v]) == (0, n, 0)
    same(b, w.reference(1, k))
    for v in (0, 2, 3, 4):
        same(w.result(*held[v]), w.reference(v, k))


def test_a_helped_query_that_overflows_its_lists(T):
    """A zero query ties every row, so every row passes its 6-bit test and every list overflows cap6: that
    query's lists take the settle's exact re-scan, the queries scanned beside it none."""
    sim = DOT
    key = ("overflow", int(sim))
    if key not in _worlds:
        q = corpus(8, 768, sim, 400)
        q[2] = 0.0
        _worlds[key] = World(T, 768, sim, q)
    w = _worlds[key]
    n, k = w.n_tiles, 10

    def exact(v):
        return w.views[v].counter("sq8_exact_tiles")
    # what the other queries re-scan on their own: the 1 237-row shard is one tile, whose four lists cannot
    # form a floor for k = 10 (fewer lists than k), so its rows all pass and its lists overflow in every call
    e0 = exact(0)
    w.refs.pop((0, k), None)
    w.reference(0, k)
    alone = exact(0) - e0
    assert alone == 4
    exact0 = [exact(v) for v in range(3)]
    before = [w.tiles(v) for v in range(3)]
    held = [w.post(v, {1: 2, 2: 3}[v], k) for v in (1, 2)]
    a = w.search(0, 0, k)
    for v in (1, 2):
        w.resume(v)
    got = [a] + [w.result(*h) for h in held]
    after = [w.tiles(v) for v in range(3)]
    exact1 = [exact(v) for v in range(3)]
    assert delta(after[0], before[0]) == (n, 0, 2 * n) and delta(after[1], before[1]) == (0, n, 0)
    assert exact1[1] - exact0[1] == 4 * n        # every wave list of the zero query
    assert exact1[0] - exact0[0] == alone and exact1[2] - exact0[2] == alone
    same(got[0], w.reference(0, k))
    same(got[1], w.reference(2, k))
    same(got[2], w.reference(3, k))


def test_views_that_must_not_share(T):
    w = world(T, 768, COS)
    k = 10
    # another tile table over the same segments: a group of its own, alone in it
    _lib.tune("tiles_target", TILES + 8)
    try:
        other = w.new_view()
    finally:
        _lib.tune("tiles_target", TILES)
    st = torch.cuda.Stream()
    try:
        assert other.counter("scan_tiles") != w.n_tiles
        before = [w.tiles(v) for v in range(2)]
        held = w.post(1, 1, k)
        got = w.search(0, 0, k, ds=other, stream=st)
        assert tuple(other.counter(c) for c in ("sq6_tiles_own", "sq6_tiles_by_others", "sq6_tiles_helped")) == (0, 0, 0)
        assert other.counter("sq6_calls") == 1
        same(got, w.reference(0, k))
        # a filtered call and a batch of two on a view of the group, a query posted beside them
        accept = [np.ones(len(w.rows[0]), bool), None, None]
        accept[0][::3] = False
        _lib.tune("sq6_share", 0)
        try:
            want_f = w.views[0].search(w.queries[:1], k, 0, k, accept=accept)
            want_b = w.views[0].search(w.queries[:2], k, 0, k)
        finally:
            _lib.tune("sq6_share", 1)
        got_f = w.views[0].search(w.queries[:1], k, 0, k, accept=accept)
        got_b = w.views[0].search(w.queries[:2], k, 0, k)
        for a, b in zip(got_f + got_b, want_f + want_b):
            assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
        assert [delta(w.tiles(v), before[v]) for v in range(2)] == [(0, 0, 0), (0, 0, 0)]
        w.resume(1)
        same(w.result(*held), w.reference(1, k))
        assert delta(w.tiles(1), before[1]) == (w.n_tiles, 0, 0)
    finally:
        torch.cuda.synchronize()
        other.close()


def test_views_over_a_probing_segment_do_not_share(T):
    """Two views over fresh segments: their calibration probes take the private path."""
    sim = COS
    rows = corpus(40_000, 768, sim, 500)
    q = torch.from_numpy(corpus(4, 768, sim, 501)).cuda()
    reader = LU.GpuFlatVectorsReader("v", rows, sim)
    views = [LU.DeviceShardSet([[LU.LeafReaderContext(0, 0, reader)]]) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    keys = torch.zeros((4, 1, 10), dtype=torch.int64, device="cuda")
    counts = torch.zeros((4, 1), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    try:
        for i in range(4):   # (no synchronisation: no read-back is folded, every call is a probe or beside one)
            _lib.check(T.osk_view_search_device(views[i % 2].handle, q[i].data_ptr(), 1, 10, None, keys[i].data_ptr(),
                                                counts[i].data_ptr(), None, streams[i % 2].cuda_stream))
        torch.cuda.synchronize()
        for v in views:
            assert tuple(v.counter(c) for c in ("sq6_tiles_own", "sq6_tiles_by_others", "sq6_tiles_helped")) == (0, 0, 0)
            assert v.counter("sq6_calls") == 2
        kk = keys.cpu().numpy().view(np.uint64)
        for i in range(4):
            os_, od, _ = O.exact_search(rows, q[i].cpu().numpy(), 10, int(sim), O.ORDER_DEVICE)
            s, d = LU.decode_keys(kk[i, 0])
            assert np.array_equal(d, od) and np.array_equal(s.view(np.uint32), os_.view(np.uint32))
    finally:
        for v in views:
            v.close()
        reader.close()


@pytest.mark.parametrize("dim,sim", [(768, COS), (768, SIMS[3]), (512, COS)], ids=["768-COSINE", "768-MIP", "512-COSINE"])
def test_free_running(T, dim, sim):
    """4 streams × 4 views × 40 calls issued round-robin with nothing waiting, as the benchmark issues them: who
    scans which tile is up to the timing; every result is exact and every tile of every call is accounted for."""
    w = world(T, dim, sim)
    n, k, calls = w.n_tiles, 10, 40
    refs = [w.reference(qi, k) for qi in range(8)]
    before = [w.tiles(v) for v in range(4)]
    out = [[w.buffers(k) for _ in range(calls)] for _ in range(4)]
    for c in range(calls):
        for v in range(4):
            keys, counts = out[v][c]
            _lib.check(T.osk_view_search_device(w.views[v].handle, w.dq[(c + v) % 8].data_ptr(), 1, k, None,
                                                keys.data_ptr(), counts.data_ptr(), None, w.streams[v].cuda_stream))
    torch.cuda.synchronize()
    for v in range(4):
        own, others, helped = delta(w.tiles(v), before[v])
        print(f"view {v}: own {own} by others {others} helped {helped} of {calls * n} tiles")
        assert own + others == calls * n
        for c in range(calls):
            same(w.result(*out[v][c]), refs[(c + v) % 8])
    total = [sum(delta(w.tiles(v), before[v])[i] for v in range(4)) for i in range(3)]
    assert total[1] == total[2]   # every (query, tile) pair scanned for another view was found done by its owner


def test_view_lifetime(T):
    """A view of the group created, searched once and released 20 times while another keeps searching."""
    w = world(T, 768, COS)
    k = 10
    refs0 = w.views[0].counter("seg_refs")
    st = torch.cuda.Stream()
    kept = []
    for i in range(20):
        kept.append(w.search(0, i % 8, k, wait=False))
        v = w.new_view()
        got = w.search(0, (i + 1) % 8, k, ds=v, stream=st, wait=False)
        kept.append(w.search(1, (i + 2) % 8, k, wait=False))
        v.close()
        same(w.result(*got), w.reference((i + 1) % 8, k))
    for i in range(20):
        same(w.result(*kept[2 * i]), w.reference(i % 8, k))
        same(w.result(*kept[2 * i + 1]), w.reference((i + 2) % 8, k))
    assert w.views[0].counter("seg_refs") == refs0


def test_small_views_do_not_share_by_default(T):
    """The default gate: a view whose tiles fit one round of resident workgroups (40 tiles here) keeps the
    private path, and sq6_share_min_tiles above its tile count does the same."""
    w = world(T, 768, COS)
    before = [w.tiles(v) for v in range(4)]
    for gate in (0, w.n_tiles + 1):
        _lib.tune("sq6_share_min_tiles", gate)
        try:
            outs = [w.search(v, v, 10, wait=False) for v in range(4) for _ in range(2)]
            with pytest.raises(_lib.OskError):
                w.post(1, 1, 10)
            torch.cuda.synchronize()
        finally:
            _lib.tune("sq6_share_min_tiles", 1)
        for i, o in enumerate(outs):
            same(w.result(*o), w.reference(i // 2, 10))
    assert [delta(w.tiles(v), before[v]) for v in range(4)] == [(0, 0, 0)] * 4
    _lib.tune("sq6_share_min_tiles", w.n_tiles)     # exactly its tile count: shares
    try:
        held = w.post(1, 1, 10)
        w.resume(1)
    finally:
        _lib.tune("sq6_share_min_tiles", 1)
    same(w.result(*held), w.reference(1, 10))
    assert delta(w.tiles(1), before[1]) == (w.n_tiles, 0, 0)


def test_share_off_is_the_private_path(T):
    w = world(T, 768, COS)
    before = [w.tiles(v) for v in range(4)]
    _lib.tune("sq6_share", 0)
    try:
        outs = [w.search(v, v, 10, wait=False) for v in range(4) for _ in range(3)]
        with pytest.raises(_lib.OskError):
            w.post(1, 1, 10)        # nothing to split: the call does not share
        torch.cuda.synchronize()
    finally:
        _lib.tune("sq6_share", 1)
    assert [delta(w.tiles(v), before[v]) for v in range(4)] == [(0, 0, 0)] * 4
    for i, o in enumerate(outs):
        same(w.result(*o), w.reference(i // 3, 10))
