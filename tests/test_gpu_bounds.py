"""The int8 prefilter's certified score intervals, looked at directly (DESIGN.md §1 "Bars", §3b, §3e).

Every float32 path that is not the fp32 scan itself is exact only because, for every (row, query), the
device's interval [LB, UB] contains the score the fp32 scan gives.  The other suites compare final top-k
lists, where an interval that is too tight on one side shows only if the affected row sits at the k-th
boundary.  Here the intervals themselves are read back (testing build, osk_view_debug_copy): the select
path's writer `sel_bounds` stores (LB, UB) for every row of the view ("sel_lb" / "sel_ub"), and the wave
lists of the k ≤ 12 kernels carry (ub, row) keys and lb ("sq8cand" / "sq8lb").

(a) soundness, no tolerance: LB ≤ sortable(score) ≤ UB for the oracle's score in each of its five orders;
(b) the record contains the score image of the real interval (oracle/bounds_reference.py), which fails on
    every row when a bound term is dropped or rounded the wrong way;
(c) the record exceeds the score image of the full interval by no more than twice the slack the source
    declares (a sound but needlessly wide interval costs only speed and shows nowhere else);
(d) the wave lists of sq8_scan, sq8_mfma and sq6_rebound carry the same numbers as writer 0's records,
    the wide kernel's entries (bounded through the group-scaled copy) satisfy (a);
(e) the k = 13 and k = 10 results on the same inputs equal the oracle's.

The int8 paths certify vectors whose largest |component| lies in [2^-32, 2^32] (osk_device.h sq8_in_range:
outside it the bound's float products underflow or overflow).  The first run of these tests found that, without
that gate, rows scaled by 2^60 or 2^63 lost their record (|x|² = inf made lo / hi NaN) and dropped out of
k = 13 results (EUCLIDEAN, dim 17: the row equal to the query, score 1), and rows and queries scaled by 2^-70
had intervals that missed the score (s_x·s_b underflows to 0; COSINE, dim 768).  So:
  * the certified view holds the edge set at scales 1, 2^-24 and 2^20 and is asked every query, the issue's
    scales 2^-70 … 2^63 included; an out-of-range query's record is exactly [0, +inf] for every accepted row;
  * the extreme view also holds the edge set at 2^-70 … 2^63: it has no records (the exact paths serve it),
    and (e) holds it to the oracle, which is where the lost rows showed.
"""
import contextlib
import functools
import json
import os

import numpy as np
import pytest

import bounds_inputs as BI
from opensearch_amd import _lib, lucene as LU
from oracle import bounds_reference as BR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIMS = [LU.VectorSimilarityFunction(s) for s in range(4)]
N_BASE = 2300                     # + 21 (42) edge rows in segments of 1000, 700 (sparse) and the rest
CUT = [0, 1000, 1700]
TILE_MIN_ROWS = 256               # several tiles per segment (the default 1024 gives one each)


def sel_bounds_cfg(u8):
    """osk_select.hip sel_bounds_cfg: the writer's lane-config instantiation of a row of u8 16-byte units."""
    return 0 if u8 <= 4 else 1 if u8 <= 8 else 2 if u8 <= 16 else 3 if u8 <= 32 else 4 if u8 <= 48 else \
        5 if u8 <= 64 else 6 if u8 <= 128 else 7


RAGGED = [1, 3, 17, 100, 1000, 4096]
DIMS = sorted(set(RAGGED) | {48, 200, 384, 768, 2048})
assert {sel_bounds_cfg((d + 15) // 16) for d in DIMS} == set(range(8))

# writer varies fastest: the host-side oracle / reference of a (sim, dim) is computed once and kept
CASES = [pytest.param(s, d, w, id=f"{s.name}-{d}-w{w}") for s in SIMS for d in DIMS for w in range(4)]


class Case:
    """One view: three segments of one shard (the middle one sparse), doc bases, a Bernoulli(0.3) accept
    bitset per leaf.  View row i is row i of `rows`."""

    def __init__(self, sim, dim, extreme=False):
        seed = 7000 + 16 * dim + int(sim)
        self.sim, self.dim = sim, dim
        self.rows = BI.make_rows(N_BASE, dim, sim, seed, BI.SCALES if extreme else BI.CERTIFIED_SCALES)
        self.queries = BI.make_queries(dim, sim, seed, BI.ALL_SCALES)
        self.q_ok = BI.in_range(self.queries)          # queries the int8 paths certify
        assert BI.in_range(self.rows).all() != extreme
        n = len(self.rows)
        rng = np.random.default_rng(seed)
        self.cut = CUT + [n]
        self.max_doc = [1000, 1500, n - 1700]
        self.docs = [None, np.sort(rng.choice(1500, 700, replace=False)).astype(np.int32), None]
        self.bases = [0, 1000, 2500]
        self.accept = [rng.random(m) < 0.3 for m in self.max_doc]
        self.accepted = np.concatenate([
            a[d if d is not None else np.arange(self.cut[i + 1] - self.cut[i])]
            for i, (a, d) in enumerate(zip(self.accept, self.docs))])

    def seg_rows(self, i):
        return self.rows[self.cut[i]:self.cut[i + 1]]

    def open(self):
        readers, leaves = [], []
        for i in range(3):
            kw = {} if self.docs[i] is None else dict(ord_to_doc=self.docs[i], max_doc=self.max_doc[i])
            r = LU.GpuFlatVectorsReader("v", self.seg_rows(i), self.sim, **kw)
            readers.append(r)
            leaves.append(LU.LeafReaderContext(i, self.bases[i], r))
        return LU.DeviceShardSet([leaves], [0]), readers


@functools.lru_cache(maxsize=2)
def case(sim, dim, extreme=False):
    return Case(sim, dim, extreme)


@functools.lru_cache(maxsize=1)
def oracle_all(sim, dim):
    """The oracle's score of every (order, query, row): float32 [5, nq, n], NaN = never a hit."""
    c = case(sim, dim)
    out = np.stack([BI.oracle_scores_batch(c.rows, c.queries, sim, order) for order in BI.ORDERS])
    return out


@functools.lru_cache(maxsize=1)
def reference(sim, dim):
    c = case(sim, dim)
    R, Q = BR.Quantised(c.rows), BR.Quantised(c.queries)
    rlo, rhi, cc, r = BR.real_interval(int(sim), R, Q)
    flo, fhi, _, _ = BR.full_interval(int(sim), R, Q, dim)
    return dict(R=R, Q=Q, rlo=rlo, rhi=rhi, flo=flo, fhi=fhi, c=cc, r=r)


TUNE_DEFAULTS = {"sel_writer": 2, "tile_min_rows": 1024, "sq6": 1, "sq8_mfma_min": 2, "sq8_mfma_queries": 32,
                 "sq8_wide_min": 64, "sq8_wide_force": 0, "sq8_scan_deep": 0, "sq8_mfma_ring": -1,
                 "sq6_probe_pct": 10}


@contextlib.contextmanager
def tuned(**kv):
    """Knobs of the library in use (the two builds share no state), put back to their defaults after."""
    try:
        for k, v in kv.items():
            _lib.tune(k, v)
        yield
    finally:
        for k in kv:
            _lib.tune(k, TUNE_DEFAULTS[k])


@contextlib.contextmanager
def bounds_view(c):
    with _lib.testing(), tuned(tile_min_rows=TILE_MIN_ROWS):
        ds, readers = c.open()
        try:
            yield ds
        finally:
            ds.close()
            for r in readers:
                r.close()


def device_records(ds, c, writer, filtered, queries=None):
    """(LB, UB) sortable u32 [nq, n] of `sel_bounds`: one k = 13 search per query (the buffers hold the last
    query's records)."""
    qs = range(len(c.queries)) if queries is None else queries
    n = len(c.rows)
    LB, UB = np.empty((len(qs), n), np.uint32), np.empty((len(qs), n), np.uint32)
    with tuned(sel_writer=writer):
        before = ds.counter("select_calls")
        for j, qi in enumerate(qs):
            ds.search(c.queries[qi:qi + 1], 13, 0, 13, accept=c.accept if filtered else None)
            LB[j], UB[j] = BI.select_records(ds, n)
        assert ds.counter("select_calls") - before == len(qs)
    return LB, UB


def first(mask):
    q, r = np.argwhere(mask)[0]
    return f"{int(mask.sum())} records, first: query {int(q)} row {int(r)}"


def check_sound(LB, UB, S, acc, what):
    """(a): S float32 [5, nq, n] oracle scores, acc bool [n]."""
    empty = (LB == 0) & (UB == 0)
    assert not ((LB == 0) ^ (UB == 0)).any(), what + ": half a record"
    assert empty[:, ~acc].all(), what + ": a record for a row the filter / ord→doc refuses"
    lost = empty & ~np.isnan(S[0]) & acc[None, :]
    assert not lost.any(), f"{what}: no record for a row the scan scores: {first(lost)}"
    for oi in range(len(S)):
        sb = BR.sortable(S[oi])
        bad = ~np.isnan(S[oi]) & ~empty & acc[None, :] & ~((LB <= sb) & (sb <= UB))
        if bad.any():
            q, r = np.argwhere(bad)[0]
            raise AssertionError(
                f"{what}: score outside [LB, UB] in order {oi}: {first(bad)}: score {S[oi][q, r]!r} "
                f"LB {BR.from_sortable(LB[q, r:r + 1])[0]!r} UB {BR.from_sortable(UB[q, r:r + 1])[0]!r}")


@pytest.mark.parametrize("sim,dim,writer", CASES)
def test_soundness_of_every_record(sim, dim, writer):
    """(a) No tolerance.  A row whose ORDER_DEVICE score is NaN (COSINE with a zero vector; an overflow to
    inf − inf) may have the empty record (0, 0), no other accepted row may; a refused row has it."""
    c, S = case(sim, dim), oracle_all(sim, dim)
    with bounds_view(c) as ds:
        for filtered in (True, False):
            LB, UB = device_records(ds, c, writer, filtered)
            acc = c.accepted if filtered else np.ones(len(c.rows), bool)
            check_sound(LB, UB, S, acc, "filtered" if filtered else "unfiltered")
            # a query outside the certified range: [0, +inf] for every accepted row
            zero, inf = BR.sortable(np.float32([0.0, np.inf]))
            assert np.all(LB[~c.q_ok][:, acc] == zero) and np.all(UB[~c.q_ok][:, acc] == inf)
            assert not np.all(UB[c.q_ok][:, acc] == inf)


def images(sim, ref, lo, hi):
    return BR.score_image(int(sim), lo, hi, ref["Q"].x2[:, None], ref["R"].x2[None, :])


@pytest.mark.parametrize("sim,dim,writer", CASES)
def test_records_contain_the_real_interval(sim, dim, writer):
    """(b) UB ≥ score64(c + r), LB ≤ score64(c − r) (sides swapped for EUCLIDEAN), to 2^-22 relative (the
    float roundings of Java's transform).  The data does not have to reach the edge."""
    c, ref = case(sim, dim), reference(sim, dim)
    with bounds_view(c) as ds:
        LB, UB = device_records(ds, c, writer, False)
    lb_img, ub_img = images(sim, ref, ref["rlo"], ref["rhi"])
    lbf, ubf = BR.from_sortable(LB).astype(np.float64), BR.from_sortable(UB).astype(np.float64)
    have = ~((LB == 0) & (UB == 0)) & ~np.isnan(lb_img) & ~np.isnan(ub_img)
    low = have & ~(ubf >= ub_img * (1.0 - BI.REL))
    assert not low.any(), f"UB below the real interval's image: {first(low)}"
    high = have & ~(lbf <= lb_img * (1.0 + BI.REL))
    assert not high.any(), f"LB above the real interval's image: {first(high)}"


declared_slack = BI.declared_slack   # (shared with test_gpu_sq6_bounds.py)


TIGHTNESS = {}


@pytest.mark.parametrize("sim,dim,writer", CASES)
def test_records_are_tight(sim, dim, writer):
    """(c) A record may exceed the score image of the reference's full interval by twice the declared slack
    mapped through the transform, plus 2·2^-17·max(1, |cos|) for the fp32 COSINE writers (1–3), plus the
    2^-22 relative of the transform's own float roundings (a float record cannot sit closer to a real bound).
    Queries outside the certified range have the record [0, +inf] by design and are not judged, nor are
    records whose full interval is open.  Measured on one MI355X (profiles/bounds/tightness.json): EUCLIDEAN and
    DOT_PRODUCT 1/(1 + 2^-22) (where the allowed lower end clamps to score 0 and LB is 0), MAXIMUM_INNER_PRODUCT
    0.80, COSINE 0.63 (writer 0) and 0.51 (writers 1–3)."""
    c, ref = case(sim, dim), reference(sim, dim)
    with bounds_view(c) as ds:
        LB, UB = device_records(ds, c, writer, False)
    with np.errstate(all="ignore"):
        sl = 2.0 * declared_slack(sim, ref, dim)
        lb_f, ub_f = images(sim, ref, ref["flo"], ref["fhi"])
        lo_a = np.maximum(ref["flo"] - sl, 0.0) if int(sim) == BR.EUCLIDEAN else ref["flo"] - sl
        lb_a, ub_a = images(sim, ref, lo_a, ref["fhi"] + sl)
        extra = 0.0
        if int(sim) == BR.COSINE and writer > 0:
            den = np.sqrt(ref["Q"].x2[:, None] * ref["R"].x2[None, :])
            extra = 2.0 * 2.0 ** -17 * np.maximum(1.0, np.maximum(np.abs(ref["flo"]), np.abs(ref["fhi"])) / den)
        up_allow = (ub_a - ub_f) + BI.REL * ub_f + extra
        dn_allow = (lb_f - lb_a) + BI.REL * lb_f + extra
        lbf, ubf = BR.from_sortable(LB).astype(np.float64), BR.from_sortable(UB).astype(np.float64)
        have = ~((LB == 0) & (UB == 0)) & np.isfinite(ub_f) & np.isfinite(lb_f) & np.isfinite(ub_a) & \
            np.isfinite(lb_a) & np.isfinite(up_allow) & np.isfinite(dn_allow) & c.q_ok[:, None]
        up, dn = np.where(have, ubf - ub_f, 0.0), np.where(have, lb_f - lbf, 0.0)
        ru = np.where(up > 0, up / up_allow, 0.0)
        rd = np.where(dn > 0, dn / dn_allow, 0.0)
    ratio = float(max(ru.max(), rd.max()))
    key = f"{sim.name}/writer{writer}"
    TIGHTNESS[key] = max(TIGHTNESS.get(key, 0.0), ratio)
    print(f"tightness {key} dim {dim}: largest excess / allowed = {ratio:.4f}")
    out = os.environ.get("OSK_BOUNDS_TIGHTNESS_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"largest observed excess / allowed excess, per similarity and sel_writer": TIGHTNESS}, f,
                      indent=1, sort_keys=True)
    wide = (ru > 1.0) | (rd > 1.0)
    assert not wide.any(), f"record wider than the declared slack allows (ratio {ratio:.3f}): {first(wide)}"


# ---- (d) the wave lists of the k ≤ 12 kernels ---------------------------------------------------------

LIST_KERNELS = {
    # name: (tunes, batch, dims, filtered too, the counter that proves the path)
    "sq8_scan": (dict(sq8_mfma_min=0, sq6=0), 1, [17, 100, 768, 4096], True, "sq8_calls"),
    "sq8_scan_deep": (dict(sq8_mfma_min=0, sq6=0, sq8_scan_deep=1), 1, [100, 768], False, "sq8_calls"),
    "sq8_mfma_b2": (dict(sq8_mfma_min=2, sq8_wide_min=0), 2, [100, 768], False, "sq8_calls"),
    "sq8_mfma_b32": (dict(sq8_mfma_min=2, sq8_wide_min=0), 32, [100, 768], False, "sq8_calls"),
    "sq8_mfma_b32_q16": (dict(sq8_mfma_min=2, sq8_wide_min=0, sq8_mfma_queries=16), 32, [100], False, "sq8_calls"),
    "sq8_mfma_b32_reg": (dict(sq8_mfma_min=2, sq8_wide_min=0, sq8_mfma_ring=0), 32, [100], False, "sq8_calls"),
    # (sq6_probe_pct 100: the calibration keeps the tier whatever the edge queries re-bound)
    "sq6_rebound": (dict(sq8_mfma_min=0, sq6=1, sq6_probe_pct=100), 1, [768, 1000], False, "sq6_calls"),
    "sq8_wide": (dict(sq8_mfma_min=2, sq8_wide_min=2, sq8_wide_force=1), 32, [100, 200], False, "sq8_wide_calls"),
}
LIST_CASES = [pytest.param(k, s, d, id=f"{k}-{s.name}-{d}") for k, v in LIST_KERNELS.items() for s in SIMS
              for d in v[2]]
N_LIST_QUERIES = 64               # the two synth queries, the certified edge queries (42) and 20 at 2^-70 / 2^-64


def list_entries(keys, lbs):
    """The real entries of one query's lists: (view row, ub bits, lb bits).  Key 0 is an empty slot; a key
    whose score field is all ones is a list's overflow mark (sq6_rebound ~0, the wide kernel 0xFFFFFFFF·2^32)."""
    real = (keys != 0) & ((keys >> np.uint64(32)) != np.uint64(0xFFFFFFFF))
    k = keys[real]
    return (0xFFFFFFFF - (k & np.uint64(0xFFFFFFFF))).astype(np.int64), (k >> np.uint64(32)).astype(np.uint32), lbs[real]


@pytest.mark.parametrize("kernel,sim,dim", LIST_CASES)
def test_wave_lists_carry_the_records(kernel, sim, dim):
    """(d) After a k = 10 search of the same view and query, every listed (ub, lb) equals writer 0's record
    of that row bit for bit: sq8_scan, sq8_mfma and sq6_rebound all evaluate sq8_bounds on the same exact
    integer dot and bound terms and apply the Java transform, as writer 0 does.  The wide kernel bounds
    through the group-scaled copy (one scale per 16 rows, other terms), so its entries are held to (a)."""
    tunes, batch, _, filt_too, counter = LIST_KERNELS[kernel]
    c = case(sim, dim)
    nq = N_LIST_QUERIES
    S = oracle_all(sim, dim) if kernel == "sq8_wide" else None
    n = len(c.rows)
    with bounds_view(c) as ds:
        for filtered in ((False, True) if filt_too else (False,)):
            acc = c.accept if filtered else None
            LB, UB = device_records(ds, c, 0, filtered, range(nq))
            listed = 0
            with tuned(**tunes):
                for q0 in range(0, nq, batch):
                    before = ds.counter(counter)
                    ds.search(c.queries[q0:q0 + batch], 10, 0, 10, accept=acc)
                    assert ds.counter(counter) == before + 1, f"{kernel} did not take this search"
                    keys, lbs = BI.wave_lists(ds, batch)
                    for b in range(batch):
                        if not c.q_ok[q0 + b]:
                            continue   # (the settle re-scans every list of such a query and reads none)
                        rows, ub, lb = list_entries(keys[b], lbs[b])
                        assert np.all((rows >= 0) & (rows < n)) and len(np.unique(rows)) == len(rows)
                        listed += len(rows)
                        if kernel == "sq8_wide":
                            for oi in range(len(S)):
                                sc = S[oi][q0 + b, rows]
                                sb = BR.sortable(sc)
                                assert np.all(np.isnan(sc) | ((lb <= sb) & (sb <= ub))), (q0 + b, oi)
                        else:
                            assert np.array_equal(ub, UB[q0 + b, rows]), (q0 + b, "ub")
                            assert np.array_equal(lb, LB[q0 + b, rows]), (q0 + b, "lb")
            assert listed >= int(c.q_ok[:nq].sum())   # (the lists were really read)


# ---- (e) end to end on the same inputs -----------------------------------------------------------------

SCAN_KERNELS = {   # test_gpu_prefilter.py's scan_kernel fixture values
    "mfma32": {}, "mfma16": dict(sq8_mfma_queries=16), "mfma32reg": dict(sq8_mfma_ring=0),
    "valu": dict(sq8_mfma_min=0), "valudeep": dict(sq8_mfma_min=0, sq8_scan_deep=1),
    "wide": dict(sq8_wide_min=2, sq8_wide_force=1),
}


E2E_BATCH = 38


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=1)
def expected(sim, dim, extreme):
    """(k, filtered) → per query the shard's (scores, docs): [L] exactSearch per leaf, merged."""
    c = case(sim, dim, extreme)
    out = {}
    for k in (13, 10):
        for filtered in (False, True):
            want = []
            for qi in range(len(c.queries)):
                leaf = []
                for i in range(3):
                    ab = O.bits_from_bool(c.accept[i]) if filtered else None
                    sc, dc, _ = O.exact_search(c.seg_rows(i), c.queries[qi], k, int(sim), ord_to_doc=c.docs[i],
                                               accept_bits=ab)
                    leaf.append((sc, dc + c.bases[i]))
                ms, md, _, _, _ = O.topdocs_merge(leaf, 0, k)
                want.append((ms, md))
            out[(k, filtered)] = want
    return out


@pytest.mark.parametrize("scan_kernel", list(SCAN_KERNELS))
@pytest.mark.parametrize("extreme", [False, True], ids=["certified", "extreme"])
@pytest.mark.parametrize("dim", [17, 100, 768])
@pytest.mark.parametrize("sim", SIMS, ids=lambda s: s.name)
def test_end_to_end_equals_oracle(sim, dim, extreme, scan_kernel):
    """(e) k = 13 (select path) and k = 10 (prefilter; batched and one by one) on the shipped library: docs,
    score bits and counts equal [L] exactSearch per leaf merged per shard; each leaf's own search also gives
    the oracle's visited count, with and without the accept bitset."""
    c = case(sim, dim, extreme)
    with tuned(tile_min_rows=TILE_MIN_ROWS, **SCAN_KERNELS[scan_kernel]):
        ds, readers = c.open()
        try:
            for k in (13, 10):
                for filtered in (False, True):
                    acc = c.accept if filtered else None
                    want = expected(sim, dim, extreme)[(k, filtered)]
                    # (batches below mfma_min_batch = 96: larger ones take the bf16×3 path, which is not this
                    # certificate's)
                    parts = [ds.search(c.queries[i:i + E2E_BATCH], k, 0, k, accept=acc)
                             for i in range(0, len(c.queries), E2E_BATCH)]
                    runs = [tuple(np.concatenate([p[j] for p in parts]) for j in range(6))]
                    if k == 10:   # single queries take sq8_scan / the 6-bit tier
                        one = [ds.search(c.queries[i:i + 1], k, 0, k, accept=acc) for i in range(0, len(c.queries), 7)]
                        runs.append(one)
                    s, d, _, cnt, tot, _ = runs[0]
                    for qi, (ms, md) in enumerate(want):
                        assert cnt[qi] == len(md) and tot[qi] == len(md), (k, filtered, qi)
                        assert np.array_equal(d[qi, :cnt[qi]], md), (k, filtered, qi)
                        assert np.array_equal(bits(s[qi, :cnt[qi]]), bits(ms)), (k, filtered, qi)
                    if k == 10:
                        for j, qi in enumerate(range(0, len(c.queries), 7)):
                            s1, d1, _, c1, _, _ = runs[1][j]
                            assert c1[0] == cnt[qi] and np.array_equal(d1[0], d[qi]) and \
                                np.array_equal(bits(s1[0]), bits(s[qi])), (filtered, qi)
            # the int8 prefilter served the certified view's k = 10 searches and none of the extreme view's
            assert (ds.counter("sq8_calls") > 0) == (not extreme)
            for k in (13, 10):
                for i, r in enumerate(readers):
                    for ab in (None, O.bits_from_bool(c.accept[i])):
                        s, d, cnt, vis = r.search_batch(c.queries[:9], k, ab)
                        for qi in range(9):
                            sc, dc, ov = O.exact_search(c.seg_rows(i), c.queries[qi], k, int(sim),
                                                        ord_to_doc=c.docs[i], accept_bits=ab)
                            assert cnt[qi] == len(dc) and vis[qi] == ov, (k, i, qi)
                            assert np.array_equal(d[qi, :cnt[qi]], dc) and np.array_equal(bits(s[qi, :cnt[qi]]), bits(sc))
        finally:
            ds.close()
            for r in readers:
                r.close()
