"""The 6-bit tier's certificate, looked at directly (osk_sq6.hip).

sq6_scan and sq6_scan_shared drop every row whose 6-bit upper bound lies below a per-(query, shard) floor, the
k-th best of 64 bucket maxima of lower bounds, and a dropped row is never seen again.  The result suites
(test_gpu_sq6.py, test_gpu_sq6_share.py, test_gpu_full_size.py) notice a bound that is too tight, a floor that is
too high, a wrong nibble weight or a non-zero padding code only if the wronged row sits at its shard's k-th
boundary.  Here the pass's own buffers are read back (testing build, osk_view_debug_copy "sq6cand", "sq6cnt",
"sq6floor", "sq6_tiles") and held to the float64 reference (oracle/bounds_reference.py: rows at 31 levels, the
query at 119) and to the oracle's score in each of its five orders.  A record's value is the bound side the
test read (osk_sq6.hip cand6_value): the dot's upper side, EUCLIDEAN the d² lower side, COSINE the dot's upper
side over √|x|².  Single queries, k = 10 unless said, sq6_probe_pct 100 (the tier stays whatever the edge
queries re-bound).

(A) Full-record views (bounds_inputs.Sq6FullInputs; dims 470 … 1536: every C from 2 to 6, in each a dim that is
no multiple of 4 or 16, 470 on sq6_supported's boundary; all four similarities; the edge set at the certified
scales with constant and zero rows; a shard on the far side of the query).  No shard has k non-empty wave lists,
so none gets a floor and every row is recorded:
  1 membership: each list holds exactly the rows of its sq6_wave share, each once;
  2 soundness, no tolerance: the score image of the value ≥ the oracle's score in every order;
  3 containment: the value's image is on the outer side of the real 6-bit interval's (to BI.REL);
  4 tightness: it exceeds the full interval's image by no more than twice the declared slack;
  5 buckets: the bucket a planted row decides is ≤ its score in every order, ≤ the real interval's lower image
    (and the full interval's, for COSINE with |x|² at the end of its fp32 range that lowers the score) and ≥
    the full interval's lower image less the declared slacks; the far shard's take the lo < 0 branches;
  6 sq6_scan, sq6_scan_shared for its own view and sq6_scan_shared run by another view's pass record the same
    bits;
  7 a tile of 1,500 rows overflows its four lists: full counts, 256 distinct rows with sound values, exact
    re-scans, the oracle's result.
(B) Floored views (bounds_inputs.Sq6FlooredInputs; 16,384 dist 3 rows in 16 tiles = 64 lists, flat and ragged
over three shards; dims 512, 768, 1024, 1536; k 1, 10, 12): the final floor T = the k-th best bucket is at
least the floor cell and at most the shard's k-th best score in every order; every dropped row scores below that
k-th best and has a real upper image below T; every bucket is at most its own list's best lower image; the
stored candidates satisfy 2–4; and the test does not pass on nothing (≥ 20 % of the rows dropped in every search;
≥ 5 % of the rows within 2 % of T in every search with k 10 or 12 and over each view's searches together — at
k = 1 alone as few as 0.4 % are: T is then the best row's own lower bound, test_not_passing_on_nothing).

Tightness measured on one MI355X (profiles/bounds/sq6_tightness.json; OSK_SQ6_TIGHTNESS_OUT=<file> writes it),
largest excess / allowed excess over (A), (A7) and (B): COSINE 0.52, DOT_PRODUCT 0.56, EUCLIDEAN 0.55,
MAXIMUM_INNER_PRODUCT 0.60.  The limit is 1, the declared slack, not these figures.
"""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bounds_inputs as BI
from opensearch_amd import _lib, lucene as LU
from oracle import bounds_reference as BR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIMS = [LU.VectorSimilarityFunction(s) for s in range(4)]
P = C.c_void_p
K = BI.SQ6_K
CAP = BI.SQ6_CAP
CAND = np.dtype([("row", np.uint32), ("val", np.float32)])
TILE = np.dtype([("seg", np.int32), ("shard", np.int32), ("rb", np.int64), ("re", np.int64)])
KNOBS = {"sq6_probe_pct": 10, "tiles_target": 0, "tile_min_rows": 1024, "sq6_share": 1, "sq6_share_min_tiles": 0}
TIGHTNESS = {}        # largest excess / allowed excess seen in this run, per similarity


@pytest.fixture(scope="module", autouse=True)
def T():
    """The whole module runs on the testing build; every knob is put back after."""
    with _lib.testing() as t:
        t.osk_testing_sq6_post.restype = C.c_int32
        t.osk_testing_sq6_post.argtypes = [P, P, C.c_int32, P, P, P, P]
        t.osk_testing_sq6_resume.restype = C.c_int32
        t.osk_testing_sq6_resume.argtypes = [P]
        _lib.tune("sq6_probe_pct", 100)
        _lib.tune("sq6_share_min_tiles", 1)
        try:
            yield t
        finally:
            for k, v in KNOBS.items():
                _lib.tune(k, v)


class View:
    """Readers over `segs`, shard by shard, and views over them with the tile table of (tiles_target,
    tile_min_rows)."""

    def __init__(self, segs, seg_shard, sim, tiles_target, tile_min_rows, docs=None, max_doc=None):
        self.readers, self.leaves = [], [[] for _ in range(max(seg_shard) + 1)]
        base = [0] * len(self.leaves)
        for i, (rows, sh) in enumerate(zip(segs, seg_shard)):
            kw = {} if docs is None or docs[i] is None else dict(ord_to_doc=docs[i], max_doc=max_doc[i])
            r = LU.GpuFlatVectorsReader("v", rows, sim, **kw)
            self.readers.append(r)
            self.leaves[sh].append(LU.LeafReaderContext(len(self.leaves[sh]), base[sh], r))
            base[sh] += max_doc[i] if kw else len(rows)
        self.n_shards = len(self.leaves)
        self.tune = (tiles_target, tile_min_rows)
        self.views = []

    def new(self):
        _lib.tune("tiles_target", self.tune[0])
        _lib.tune("tile_min_rows", self.tune[1])
        try:
            self.views.append(LU.DeviceShardSet(self.leaves))
        finally:
            _lib.tune("tiles_target", KNOBS["tiles_target"])
            _lib.tune("tile_min_rows", KNOBS["tile_min_rows"])
        return self.views[-1]

    def close(self):
        torch.cuda.synchronize()
        for v in self.views:
            v.close()
        for r in self.readers:
            r.close()


def tile_table(ds):
    t = BI.debug_copy(ds, "sq6_tiles", ds.counter("scan_tiles"), TILE)
    return [(int(a), int(b), int(c), int(d)) for a, b, c, d in t.tolist()]


def records(ds, n_shards):
    """The last 6-bit search's (counts [lists], candidates [lists, 256], buckets [shards, 64], cells [shards])."""
    n_lists = 4 * ds.counter("scan_tiles")
    cnt = BI.debug_copy(ds, "sq6cnt", n_lists, np.int32)
    cand = BI.debug_copy(ds, "sq6cand", n_lists * CAP, CAND).reshape(n_lists, CAP)
    fl = BI.debug_copy(ds, "sq6floor", n_shards * (BI.FLOOR_BUCKETS + 1) * BI.FLOOR_STRIDE, np.uint32)
    fl = fl.reshape(n_shards, BI.FLOOR_BUCKETS + 1, BI.FLOOR_STRIDE)[:, :, 0]
    return SimpleNamespace(cnt=cnt, cand=cand, buckets=fl[:, :BI.FLOOR_BUCKETS].copy(), cell=fl[:, BI.FLOOR_BUCKETS].copy())


def dense(c, rec):
    """A search's records by view row: (value f32 [n], times listed [n], whether the row's list overflowed [n])."""
    n = int(c.seg_vrow[-1])
    val, seen, over = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, bool)
    for l, (_, vrows) in enumerate(c.lists):
        stored = min(int(rec.cnt[l]), CAP)
        over[vrows] = rec.cnt[l] > CAP
        vr = c.seg_vrow[c.tiles[l >> 2][0]] + rec.cand["row"][l, :stored].astype(np.int64)
        assert np.all((vr >= 0) & (vr < n)), f"list {l}: a row outside the view"
        np.add.at(seen, vr, 1)
        val[vr] = rec.cand["val"][l, :stored]
    return val, seen, over


def first(mask):
    q, r = np.argwhere(mask)[0]
    return f"{int(mask.sum())} records, first: query {int(q)} row {int(r)}"


# ---- checks 2–4 on dense arrays [nq, n]: VAL the recorded values, have where a record exists ----------------

def value_image(sim, val, qn):
    """The float64 score image of a recorded value (COSINE: already over √|x|², so only the real |q|² enters)."""
    v = np.asarray(val, np.float64)
    with np.errstate(all="ignore"):
        if int(sim) == BR.COSINE:
            s = (1.0 + v / np.sqrt(qn)) / 2.0
            return np.where(s >= 0, s, np.where(np.isnan(s), s, 0.0))
        return BR.score64(int(sim), v)


def check_sound(sim, val, have, S, qn):
    """2: Java's own float transform of the value, operation by operation, against the oracle's float scores."""
    img = BI.score32(int(sim), val, qn)
    for oi in range(len(S)):
        bad = have & ~np.isnan(S[oi]) & ~(img >= S[oi])
        if bad.any():
            q, r = np.argwhere(bad)[0]
            raise AssertionError(f"score above the value's image in order {oi}: {first(bad)}: score {S[oi][q, r]!r} "
                                 f"image {img[q, r]!r} value {val[q, r]!r}")


def outer_images(sim, ref, lo, hi):
    """The score image of the side the 6-bit test reads: the upper image."""
    return BR.score_image(int(sim), lo, hi, ref["Q"].x2[:, None], ref["R"].x2[None, :])[1]


def check_contained(sim, val, have, ref):
    """3: value image ≥ the real interval's upper image, to BI.REL relative."""
    img = value_image(sim, val, ref["Q"].x2[:, None])
    want = outer_images(sim, ref, ref["rlo"], ref["rhi"])
    low = have & ~np.isnan(want) & ~(img >= want * (1.0 - BI.REL))
    assert not low.any(), f"value inside the real 6-bit interval: {first(low)}"


def tightness(sim, dim, val, have, ref):
    """4: (value image − full interval's upper image) / allowed, the allowed excess being twice the declared
    slack through the transform — sq8_bounds' 2^-20 terms (BI.declared_slack), for COSINE also cand6_value's
    2^-22 and the 1-ulp v_sqrt (2^-23) on the quotient and its 2^-126 floor — plus BI.REL of the image."""
    with np.errstate(all="ignore"):
        sl = 2.0 * BI.declared_slack(sim, ref, dim)
        qn = ref["Q"].x2[:, None]
        at = outer_images(sim, ref, ref["flo"], ref["fhi"])
        if int(sim) == BR.EUCLIDEAN:
            allowed = outer_images(sim, ref, np.maximum(ref["flo"] - sl, 0.0), ref["fhi"])
        elif int(sim) == BR.COSINE:
            v = (ref["fhi"] + sl) / np.sqrt(ref["R"].x2[None, :])
            v = v + np.abs(v) * 2.0 * (2.0 ** -22 + 2.0 ** -23) + 2.0 * 2.0 ** -126
            allowed = value_image(sim, v, qn)
        else:
            allowed = outer_images(sim, ref, ref["flo"], ref["fhi"] + sl)
        allow = (allowed - at) + BI.REL * at
        ok = have & np.isfinite(at) & np.isfinite(allow) & np.isfinite(val)
        excess = np.where(ok, value_image(sim, val, qn) - at, 0.0)
        ratio = np.where(excess > 0, excess / allow, 0.0)
    key = LU.VectorSimilarityFunction(int(sim)).name
    TIGHTNESS[key] = max(TIGHTNESS.get(key, 0.0), float(ratio.max()))
    out = os.environ.get("OSK_SQ6_TIGHTNESS_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"largest observed excess / allowed excess of a 6-bit record, per similarity": TIGHTNESS}, f,
                      indent=1, sort_keys=True)
    return ratio


def check_tight(sim, dim, val, have, ref):
    ratio = tightness(sim, dim, val, have, ref)
    print(f"6-bit tightness {LU.VectorSimilarityFunction(int(sim)).name} dim {dim}: {float(ratio.max()):.4f}")
    assert not (ratio > 1.0).any(), f"value wider than the declared slack allows ({ratio.max():.3f}): {first(ratio > 1.0)}"


# ---- (A) full-record views -----------------------------------------------------------------------------------

def device_search(T, ds, dq_row, k, n_shards, stream, post=False):
    keys = torch.zeros((1, n_shards, k), dtype=torch.int64, device="cuda")
    counts = torch.zeros((1, n_shards), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if post:
        _lib.check(T.osk_testing_sq6_post(ds.handle, dq_row.data_ptr(), k, keys.data_ptr(), counts.data_ptr(), None,
                                          stream.cuda_stream))
    else:
        _lib.check(T.osk_view_search_device(ds.handle, dq_row.data_ptr(), 1, k, None, keys.data_ptr(),
                                            counts.data_ptr(), None, stream.cuda_stream))
        torch.cuda.synchronize()
    return keys, counts


def share_counters(ds):
    return np.array([ds.counter(n) for n in ("sq6_calls", "sq6_tiles_own", "sq6_tiles_by_others")])


FULL = [pytest.param((s, d), id=f"{s.name}-{d}") for s in SIMS for d in BI.SQ6_DIMS]


@pytest.fixture(scope="module", params=FULL)
def full(request, T):
    """The inputs, oracle scores [5, nq, n], reference and the device's records of every query of one (sim, dim),
    recorded three ways: `scan` (sq6_scan), `own` (sq6_scan_shared for its own view), `others` (sq6_scan_shared
    run by another view's pass)."""
    sim, dim = request.param
    c = BI.Sq6FullInputs(sim, dim)
    ref = BI.sq6_reference(sim, c.rows, c.queries, dim)
    S = np.stack([BI.oracle_scores_batch(c.rows, c.queries, int(sim), o) for o in BI.ORDERS])
    w = View(c.segs, c.seg_shard, sim, len(c.segs), c.TILE_MIN_ROWS)
    nq, ns = len(c.queries), w.n_shards
    try:
        v0, v1 = w.new(), w.new()
        st0, st1 = torch.cuda.Stream(), torch.cuda.Stream()
        dq = torch.from_numpy(c.queries).cuda()
        n_tiles = v0.counter("scan_tiles")
        # the segments' first four single queries calibrate the tier; the fifth folds the last read-back
        _lib.tune("sq6_share", 0)
        before = share_counters(v0)
        for _ in range(5):
            device_search(T, v0, dq[0], K, ns, st0)
        calibrated = share_counters(v0) - before
        tiles = tile_table(v0)
        before = share_counters(v0)
        scan = []
        for qi in range(nq):
            device_search(T, v0, dq[qi], K, ns, st0)
            scan.append(records(v0, ns))
        d_scan = share_counters(v0) - before
        # both views join the share group with their next call
        _lib.tune("sq6_share", 1)
        device_search(T, v0, dq[0], K, ns, st0)
        device_search(T, v1, dq[0], K, ns, st1)
        before = share_counters(v0)
        own = []
        for qi in range(nq):
            device_search(T, v0, dq[qi], K, ns, st0)
            own.append(records(v0, ns))
        d_own = share_counters(v0) - before
        before = share_counters(v0)
        others = []
        for qi in range(nq):
            device_search(T, v0, dq[qi], K, ns, st0, post=True)
            device_search(T, v1, dq[(qi + 1) % nq], K, ns, st1)
            _lib.check(T.osk_testing_sq6_resume(v0.handle))
            torch.cuda.synchronize()
            others.append(records(v0, ns))
        d_others = share_counters(v0) - before
    finally:
        _lib.tune("sq6_share", 1)
        w.close()
    dn = [dense(c, r) for r in scan]
    return SimpleNamespace(sim=sim, dim=dim, c=c, ref=ref, S=S, n_tiles=n_tiles, tiles=tiles, calibrated=calibrated,
                           scan=scan, own=own, others=others, d_scan=d_scan, d_own=d_own, d_others=d_others,
                           val=np.stack([d[0] for d in dn]), seen=np.stack([d[1] for d in dn]))


def test_full_record_mode(full):
    """The dim keeps its tier (sq6_calls rises with every call), the view has the tile table the inputs assume,
    no shard gets a floor, and every row of the view is recorded: Σ sq6cnt = rows, no count above 256."""
    c, nq = full.c, len(full.c.queries)
    assert full.calibrated[0] == 5 and full.d_scan[0] == nq and tuple(full.d_scan[1:]) == (0, 0)
    assert full.tiles == c.tiles
    for qi, r in enumerate(full.scan):
        assert int(r.cnt.sum()) == len(c.rows) and r.cnt.max() <= CAP, qi
        assert not r.cell.any(), (qi, "a floor in a shard of fewer than k lists")


def test_membership(full):
    """1: each list holds exactly the rows of its sq6_wave share (recomputed from the tile table), each once."""
    c = full.c
    for qi, r in enumerate(full.scan):
        for l, (_, vrows) in enumerate(c.lists):
            assert r.cnt[l] == len(vrows), (qi, l)
            got = np.sort(c.seg_vrow[c.tiles[l >> 2][0]] + r.cand["row"][l, :len(vrows)].astype(np.int64))
            assert np.array_equal(got, vrows), (qi, l)
    assert np.all(full.seen == 1)


def test_soundness(full):
    """2: no tolerance.  A COSINE zero row's record is +inf (it is kept: its score is NaN in every order and the
    settle decides it)."""
    have = full.seen == 1
    check_sound(full.sim, full.val, have, full.S, full.ref["Q"].x2[:, None])
    if int(full.sim) == BR.COSINE:
        zero = full.ref["R"].x2 == 0
        assert zero.sum() == len(BI.CERTIFIED_SCALES) and np.all(np.isposinf(full.val[:, zero])) and have[:, zero].all()
        assert np.all(np.isfinite(full.val[:, ~zero]))
    else:
        assert np.all(np.isfinite(full.val))


def test_containment(full):
    """3: fails on about half the rows if a nibble weight, a lane's half-chunk or a padding code is wrong, on
    every row if a bound term is dropped."""
    check_contained(full.sim, full.val, full.seen == 1, full.ref)


def test_tightness(full):
    """4: the rule of test_gpu_bounds.py test_records_are_tight, for the one side the 6-bit test reads."""
    check_tight(full.sim, full.dim, full.val, full.seen == 1, full.ref)


def test_buckets(full):
    """5: query 0's buckets.  Each non-empty list's planted row tops every other lower bound its list can publish
    (asserted from the reference first), so the list's bucket is that row's floor_lb_score."""
    c, ref, sim = full.c, full.ref, int(full.sim)
    least = BI.bucket_low_limit(sim, ref, full.dim, 0)
    margins = c.plant_margin(ref, least)
    assert all(lo > others * (1.0 + BI.REL) for _, lo, others in margins)
    real_lb = BR.floor_image(sim, ref["rlo"][0], ref["rhi"][0], ref["Q"].x2[0], ref["R"].x2)
    most = BI.bucket_high_limit(sim, ref, full.dim, 0)
    r = full.scan[0]
    expected = np.zeros_like(r.buckets, dtype=bool)
    negative = 0
    for l, vrow in c.plants.items():
        shard = c.lists[l][0]
        expected[shard, l & (BI.FLOOR_BUCKETS - 1)] = True
        bits = r.buckets[shard, l & (BI.FLOOR_BUCKETS - 1)]
        b = float(BR.from_sortable(np.array([bits], np.uint32))[0])
        for oi in range(len(full.S)):
            assert bits <= BR.sortable(full.S[oi][0, vrow:vrow + 1])[0], (l, oi, b, full.S[oi][0, vrow])
        assert b <= real_lb[vrow], (l, b, real_lb[vrow])
        assert b <= most[vrow], (l, b, most[vrow])      # (the full interval's, COSINE with the norm at its worst)
        assert b >= least[vrow], (l, b, least[vrow])
        negative += ref["rhi"][0][vrow] < 0
    assert not r.buckets[~expected].any(), "a bucket no list of the shard maps to"
    assert sim == BR.EUCLIDEAN or negative == 6       # the far shard's lists: lo < 0 decides


def same_records(a, b, what):
    assert np.array_equal(a.cnt, b.cnt), what
    assert np.array_equal(a.buckets, b.buckets) and np.array_equal(a.cell, b.cell), what
    for l in range(len(a.cnt)):
        n = min(int(a.cnt[l]), CAP)
        assert np.array_equal(a.cand[l, :n].view(np.uint64), b.cand[l, :n].view(np.uint64)), (what, l)


def test_the_three_producers_agree(full):
    """6: the dots are exact integers and everything after them is shared code, so any difference is a bug."""
    nq = len(full.c.queries)
    assert tuple(full.d_own) == (nq, nq * full.n_tiles, 0)
    assert tuple(full.d_others) == (nq, 0, nq * full.n_tiles)
    for qi in range(nq):
        same_records(full.scan[qi], full.own[qi], (qi, "sq6_scan_shared for its own view"))
        same_records(full.scan[qi], full.others[qi], (qi, "sq6_scan_shared in another view's pass"))


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("dim", BI.SQ6_DIMS)
@pytest.mark.parametrize("sim", SIMS, ids=lambda s: s.name)
def test_overflow(T, sim, dim):
    """7: one tile of 1,500 rows and no floor: every list passes 375 rows into 256 slots."""
    n = 1500
    rows = O.synth(0, n, dim, 9100 + dim, BI.DIST[int(sim)])
    queries = O.synth(0, 2, dim, 9101 + dim, BI.DIST[int(sim)])
    c = SimpleNamespace(seg_vrow=np.array([0, n]), tiles=[(0, 0, 0, n)])
    c.lists = BI.sq6_wave_lists(c.tiles, c.seg_vrow)
    ref = BI.sq6_reference(sim, rows, queries, dim)
    S = np.stack([BI.oracle_scores_batch(rows, queries, int(sim), o) for o in BI.ORDERS])
    w = View([rows], [0], sim, 1, 2048)
    try:
        ds = w.new()
        assert tile_table(ds) == c.tiles
        val, seen = np.zeros((2, n), np.float32), np.zeros((2, n), np.int32)
        for qi in range(2):
            calls, exact = ds.counter("sq6_calls"), ds.counter("sq8_exact_tiles")
            s, d, _, cnt, _, _ = ds.search(queries[qi:qi + 1], K, 0, K)
            assert ds.counter("sq6_calls") == calls + 1 and ds.counter("sq8_exact_tiles") > exact
            r = records(ds, 1)
            assert [int(x) for x in r.cnt] == [len(v) for _, v in c.lists] and r.cnt.min() > CAP
            val[qi], seen[qi], _ = dense(c, r)
            for l, (_, vrows) in enumerate(c.lists):
                assert np.isin(r.cand["row"][l], vrows).all(), (qi, l)
            os_, od, _ = O.exact_search(rows, queries[qi], K, int(sim), O.ORDER_DEVICE)
            assert cnt[0] == K and np.array_equal(d[0], od) and np.array_equal(bits(s[0]), bits(os_))
    finally:
        w.close()
    assert seen.max() == 1 and np.all(seen.sum(axis=1) == 4 * CAP)
    have = seen == 1
    check_sound(sim, val, have, S, ref["Q"].x2[:, None])
    check_contained(sim, val, have, ref)
    check_tight(sim, dim, val, have, ref)


# ---- (B) floored views ---------------------------------------------------------------------------------------

FLOORED = [pytest.param((s, d, rg), id=f"{s.name}-{d}-{'ragged' if rg else 'flat'}") for s in SIMS
           for d in BI.SQ6_FLOOR_DIMS for rg in (False, True)]
KS = (1, 10, 12)


@pytest.fixture(scope="module", params=FLOORED)
def floored(request, T):
    """One floored view: inputs, oracle scores, reference, and per (k, query) the records of its search."""
    sim, dim, ragged = request.param
    c = BI.Sq6FlooredInputs(sim, dim, ragged)
    ref = BI.sq6_reference(sim, c.rows, c.queries, dim)
    S = np.stack([BI.oracle_scores_batch(c.rows, c.queries, int(sim), o) for o in BI.ORDERS])
    segs = [c.rows[c.seg_vrow[i]:c.seg_vrow[i + 1]] for i in range(len(c.seg_rows))]
    w = View(segs, c.seg_shard, sim, c.TILES, c.TILE_MIN_ROWS, c.docs, c.max_doc)
    rec = {}
    try:
        ds = w.new()
        tiles = tile_table(ds)
        calls = ds.counter("sq6_calls")
        for k in KS:
            for qi in range(len(c.queries)):
                ds.search(c.queries[qi:qi + 1], k, 0, k)
                rec[(k, qi)] = records(ds, w.n_shards)
        calls = ds.counter("sq6_calls") - calls
    finally:
        w.close()
    out = SimpleNamespace(sim=sim, dim=dim, c=c, ref=ref, S=S, tiles=tiles, calls=calls, rec=rec, n_shards=w.n_shards)
    out.dense = {key: dense(c, r) for key, r in rec.items()}
    # the final floor of every (search, shard): the k-th largest of the buckets as the pass left them
    out.floor = {(k, qi): np.sort(r.buckets, axis=1)[:, ::-1][:, k - 1] for (k, qi), r in rec.items()}
    return out


def test_floored_view_is_what_the_inputs_assume(floored):
    assert floored.tiles == floored.c.tiles and floored.calls == len(floored.rec)
    assert 4 * len(floored.tiles) == BI.FLOOR_BUCKETS * (floored.c.N // 16384)


def test_floor_is_below_the_kth_best_score(floored):
    """B1: cell ≤ T ≤ sortable(the shard's k-th best score) in every order, no tolerance."""
    c = floored.c
    for (k, qi), r in floored.rec.items():
        T_ = floored.floor[(k, qi)]
        assert np.all(T_ > 0) and np.all(r.cell <= T_), (k, qi)
        for sh in range(floored.n_shards):
            rows = c.shard_of_row == sh
            for oi in range(len(floored.S)):
                kth = np.sort(BR.sortable(floored.S[oi][qi, rows]))[::-1][k - 1]
                assert T_[sh] <= kth, (k, qi, sh, oi, BR.from_sortable(T_[sh:sh + 1])[0], BR.from_sortable(np.array([kth]))[0])


def test_buckets_belong_to_their_lists(floored):
    """The floor protocol: a list's bucket is list & 63 of its shard's 64 (the 64-list views map one to one).
    Every bucket some list maps to was seeded by pilot rows (> 0) and none exceeds the best lower image of its
    own lists' rows (6-bit of any row, int8 of the four pilot rows): a bucket raised by another list's row
    would; a bucket no list maps to stays 0."""
    c, ref, sim = floored.c, floored.ref, int(floored.sim)
    for (k, qi), r in floored.rec.items():
        lb6 = BR.floor_image(sim, ref["rlo"][qi], ref["rhi"][qi], ref["Q"].x2[qi], ref["R"].x2)
        lb8 = BR.floor_image(sim, ref["p_rlo"][qi], ref["p_rhi"][qi], ref["Q"].x2[qi], ref["R"].x2)
        most = np.zeros(r.buckets.shape)
        for l, (sh, vrows) in enumerate(c.lists):
            b = l & (BI.FLOOR_BUCKETS - 1)
            most[sh, b] = max(most[sh, b], lb6[vrows].max(), lb8[vrows[:4]].max())
        got = BR.from_sortable(r.buckets).astype(np.float64)
        assert np.all((most > 0) == (r.buckets > 0)), (k, qi)
        bad = (most > 0) & ~(got <= most)
        assert not bad.any(), (k, qi, np.argwhere(bad)[0], got[bad][0], most[bad][0])


def test_dropped_rows_cannot_enter_the_top_k(floored):
    """B2: a row absent from its list (whose list did not overflow) scores below the shard's k-th best in every
    order, and its real-interval upper image lies below T.  A wave tests against a floor no higher than T and
    sq8_quick is lenient on top, so a row dropped although its real upper side reaches T means the device's
    bound is below the real one."""
    c, ref, sim = floored.c, floored.ref, int(floored.sim)
    for (k, qi), r in floored.rec.items():
        _, seen, over = floored.dense[(k, qi)]
        assert seen.max() <= 1
        dropped = (seen == 0) & ~over
        Tf = BR.from_sortable(floored.floor[(k, qi)]).astype(np.float64)[c.shard_of_row]
        ub = BR.score_image(sim, ref["rlo"][qi], ref["rhi"][qi], ref["Q"].x2[qi], ref["R"].x2)[1]
        bad = dropped & ~(ub < Tf)
        assert not bad.any(), (k, qi, int(bad.sum()), int(np.argwhere(bad)[0][0]))
        for sh in range(floored.n_shards):
            rows = c.shard_of_row == sh
            for oi in range(len(floored.S)):
                sc = floored.S[oi][qi]
                kth = np.sort(sc[rows])[::-1][k - 1]
                assert np.all(sc[rows & dropped] < kth), (k, qi, sh, oi)


def test_stored_candidates(floored):
    """B3: every stored candidate satisfies A2–A4."""
    for k in KS:
        val = np.stack([floored.dense[(k, qi)][0] for qi in range(len(floored.c.queries))])
        have = np.stack([floored.dense[(k, qi)][1] for qi in range(len(floored.c.queries))]) == 1
        assert have.any(axis=1).all()
        check_sound(floored.sim, val, have, floored.S, floored.ref["Q"].x2[:, None])
        check_contained(floored.sim, val, have, floored.ref)
        check_tight(floored.sim, floored.dim, val, have, floored.ref)


def test_not_passing_on_nothing(floored):
    """B4: every search drops ≥ 20 % of the view's rows, and ≥ 5 % of the rows have a reference upper image
    within 2 % of T — in every search with k 10 and 12, and over the view's searches together.  (k = 1 alone
    cannot: its T is the best row's own lower bound, which up to 98 % of these rows lie below, and in 12 of its
    64 searches fewer than 5 % (as few as 0.4 %) are within 2 % of it, fewer still with more rows;
    test_bounds_reference_cpu.py.)"""
    c, ref, sim = floored.c, floored.ref, int(floored.sim)
    band_all = []
    for (k, qi), r in floored.rec.items():
        _, seen, over = floored.dense[(k, qi)]
        dropped = float(((seen == 0) & ~over).mean())
        Tf = BR.from_sortable(floored.floor[(k, qi)]).astype(np.float64)
        _, band = c.shares(ref, qi, Tf)
        print(f"{LU.VectorSimilarityFunction(sim).name} dim {floored.dim} k {k} query {qi}: dropped {dropped:.3f}, "
              f"within 2 % of T {band:.3f}, overflowed lists {int((r.cnt > CAP).sum())}")
        band_all.append(band)
        assert dropped >= 0.20, (k, qi, dropped)
        assert band >= 0.05 or k == 1, (k, qi, band)
    assert np.mean(band_all) >= 0.05
