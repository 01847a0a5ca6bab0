"""Inputs and helpers shared by test_bounds_reference_cpu.py and test_gpu_bounds.py.

The corpus of a case is `O.synth` rows in the similarity's usual distribution followed by an edge set at
scale 1 and at five power-of-two scales; the queries are two `O.synth` queries followed by the edge set, its
negation and a query orthogonal to a large-norm row, at the same six scales.
"""
import ctypes as C

import numpy as np

from oracle import oracle as O

ORDERS = [O.ORDER_DEVICE, O.ORDER_SCALAR, O.ORDER_PANAMA512, O.ORDER_SCALAR_NOFMA, O.ORDER_PANAMA512_NOFMA]
DIST = {0: 1, 1: 3, 2: 3, 3: 2}                      # each similarity's usual O.synth distribution
# |x|² subnormal, near FLT_MIN, (2^60) near FLT_MAX, (2^63) past it with finite components
SCALES = [1.0, 2.0 ** -70, 2.0 ** -64, 2.0 ** -60, 2.0 ** 60, 2.0 ** 63]
# The int8 paths certify vectors whose largest |component| lies in [2^-32, 2^32] (osk_device.h sq8_in_range);
# a view holding any other row is served by the exact paths and has no records.  These scales keep the whole
# edge set inside that range, near its ends.
CERTIFIED_SCALES = [1.0, 2.0 ** -24, 2.0 ** 20]
ALL_SCALES = CERTIFIED_SCALES + SCALES[1:]


def in_range(vecs: np.ndarray) -> np.ndarray:
    m = np.abs(np.asarray(vecs, np.float32)).max(axis=-1)
    return (m == 0) | ((m >= np.float32(2.0 ** -32)) & (m <= np.float32(2.0 ** 32)))
REL = 2.0 ** -22                                     # Java's transforms round to float at most twice


def edge_rows(dim: int, seed: int) -> np.ndarray:
    """Scale-1 edge rows (float32, every entry exact in float32 where the property needs it)."""
    rng = np.random.default_rng(seed)
    zero = np.zeros(dim, np.float32)
    one = zero.copy()
    one[dim // 2] = 0.75                                              # one non-zero component
    const = np.full(dim, 0.5, np.float32)                             # constant row
    pm = np.where(rng.random(dim) < 0.5, -1.0, 1.0).astype(np.float32)   # ±max only: δ = 0
    # quantisation midpoints: max = 127·2^-7 so s = 2^-7 exactly, the rest s·(q + ½): |δ| is maximal
    mid = ((rng.integers(-127, 127, dim) + 0.5) * 2.0 ** -7).astype(np.float32)
    mid[0] = 127 * 2.0 ** -7
    # one huge component, every other code 0 (x/s = 0.49)
    huge = np.full(dim, 0.49 / 127.0, np.float32) * np.where(rng.random(dim) < 0.5, -1.0, 1.0).astype(np.float32)
    huge[dim - 1] = 1.0
    big = (rng.standard_normal(dim) * 64.0).astype(np.float32)        # large norm; `cancel_query` is ⟂ to it
    return np.stack([zero, one, const, pm, mid, huge, big])


def cancel_query(big: np.ndarray, seed: int) -> np.ndarray:
    """A large-norm query whose dot product with `big` cancels to (almost) nothing."""
    rng = np.random.default_rng(seed)
    a = big.astype(np.float64)
    c = rng.standard_normal(len(a)) * 64.0
    if a @ a > 0:
        c = c - (c @ a) / (a @ a) * a
    return c.astype(np.float32)


def scaled(vecs: np.ndarray, scales) -> np.ndarray:
    return np.concatenate([(vecs.astype(np.float64) * s).astype(np.float32) for s in scales])


def make_rows(n_base: int, dim: int, sim: int, seed: int, scales=SCALES) -> np.ndarray:
    return np.concatenate([O.synth(0, n_base, dim, seed, DIST[int(sim)]), scaled(edge_rows(dim, seed + 1), scales)])


def make_queries(dim: int, sim: int, seed: int, scales=SCALES) -> np.ndarray:
    e = edge_rows(dim, seed + 1)                                      # the rows' own edge set
    qs = np.concatenate([e, -e[1:], cancel_query(e[-1], seed + 2)[None, :]])
    return np.concatenate([O.synth(0, 2, dim, seed + 3, DIST[int(sim)]), scaled(qs, scales)])


def oracle_scores(rows, query, sim, order, ord_to_doc=None, accept_bits=None):
    """Every accepted row's oracle score by ordinal (float32 [n]); NaN where the row was not collected
    (a NaN score is never a hit) and `collected` tells the two apart from a row the filter refused."""
    n = len(rows)
    sc, dc, _ = O.exact_search(rows, query, n, int(sim), order, ord_to_doc=ord_to_doc, accept_bits=accept_bits)
    out = np.full(n, np.nan, np.float32)
    ords = dc if ord_to_doc is None else np.searchsorted(ord_to_doc, dc)
    out[ords] = sc
    got = np.zeros(n, bool)
    got[ords] = True
    return out, got


def oracle_scores_batch(rows, queries, sim, order, nthreads=8):
    """`oracle_scores` of every query at once: float32 [nq, n] (the same exact search, over row slices on
    `nthreads` threads, O.knn_batch)."""
    n = len(rows)
    sc, dc, cc = O.knn_batch(rows, queries, n, int(sim), order, nthreads)
    out = np.full((len(queries), n), np.nan, np.float32)
    for q in range(len(queries)):
        out[q, dc[q, :cc[q]]] = sc[q, :cc[q]]
    return out


def view_handle(ds) -> int:
    return ds.handle


def debug_copy(ds, name: str, count: int, dtype) -> np.ndarray:
    """`count` items of the view's workspace buffer `name` after its last search (testing build only)."""
    from opensearch_amd import _lib
    out = np.zeros(count, dtype)
    _lib.check(_lib.lib().osk_view_debug_copy(C.c_void_p(view_handle(ds)), name.encode(), out.ctypes.data, out.nbytes))
    return out


def select_records(ds, n_view_rows: int):
    """(LB, UB) sortable u32 per view row of the last query searched on the select path."""
    return debug_copy(ds, "sel_lb", n_view_rows, np.uint32), debug_copy(ds, "sel_ub", n_view_rows, np.uint32)


def wave_lists(ds, nq: int):
    """The prefilter's wave lists of the last search: (keys u64 [nq, lists·16], lb u32 [nq, lists·16])."""
    n_lists = int(debug_copy(ds, "sq8_lists", 1, np.int64)[0])
    n = nq * n_lists * 16
    return debug_copy(ds, "sq8cand", n, np.uint64).reshape(nq, -1), debug_copy(ds, "sq8lb", n, np.uint32).reshape(nq, -1)



# ---------------------------------------------------------------------------------------------------------
# The 6-bit tier's certificate (osk_sq6.hip): inputs and host restatements shared by
# test_bounds_reference_cpu.py and test_gpu_sq6_bounds.py
# ---------------------------------------------------------------------------------------------------------
# every C = ⌈dim/256⌉ from 2 to 6, in each one dim that is no multiple of 4 or 16; 470 has exactly 0.8 × its int8 row bytes, the most a tier may have
SQ6_DIMS = [470, 512, 717, 768, 1001, 1024, 1201, 1280, 1430, 1536]
SQ6_FLOOR_DIMS = [512, 768, 1024, 1536]
SQ6_CAP, FLOOR_BUCKETS, FLOOR_STRIDE = 256, 64, 16       # osk_internal.h kSq6Cap, kFloorBuckets, kFloorStride
SQ6_K = 10


def sq6_supported(dim: int) -> bool:
    """osk_sq6.hip sq6_supported: 6-bit rows (padded to 256 dims) ≤ 0.8 × the int8 rows, 2 ≤ C ≤ 6."""
    c = (dim + 255) // 256
    return 2 <= c <= 6 and 192 * c * 10 <= 16 * ((dim + 15) // 16) * 8


def wave_share(row_begin: int, row_end: int, wave: int):
    """osk_sq6.hip sq6_wave: the rows [wb, we) of a tile that wave `wave` (< 4) scans, 8-row blocks."""
    per = (row_end - row_begin + 31) // 32 * 8
    wb = row_begin + wave * per
    return wb, max(wb, min(wb + per, row_end))


def tile_table(seg_rows, seg_shard, target: int, min_rows: int):
    """osk_view_create's tile split with tune tiles_target = `target` and tile_min_rows = `min_rows` (≥ 32):
    [(seg, shard, row_begin, row_end)], shard by shard.  The GPU tests hold the view's own table to it."""
    total = sum(seg_rows)
    cap = [max(1, -(-n // min_rows)) for n in seg_rows]
    share = [n * float(target) / float(total) for n in seg_rows]
    nt = [min(c, max(1, int(s))) if n else 0 for n, c, s in zip(seg_rows, cap, share)]
    for _, i in sorted((-(s - int(s)), i) for i, (s, n) in enumerate(zip(share, seg_rows)) if n):
        if sum(nt) < target and nt[i] < cap[i]:
            nt[i] += 1
    tiles = []
    for sh in sorted(set(seg_shard)):
        for i, n in enumerate(seg_rows):
            if seg_shard[i] != sh or n == 0:
                continue
            cut = [n if t >= nt[i] else (n * t // nt[i]) & ~15 for t in range(nt[i] + 1)]
            tiles += [(i, sh, cut[t], cut[t + 1]) for t in range(nt[i]) if cut[t + 1] > cut[t]]
    return tiles


def sq6_wave_lists(tiles, seg_vrow):
    """Per list l (wave l & 3 of tile l >> 2): (shard, the view rows of its share)."""
    out = []
    for seg, shard, rb, re in tiles:
        for w in range(4):
            wb, we = wave_share(rb, re, w)
            out.append((shard, np.arange(seg_vrow[seg] + wb, seg_vrow[seg] + we)))
    return out


def score32(sim: int, raw, qn=None):
    """Java's float transforms of a raw float32 value, operation by operation (osk_common.h score_f32).  COSINE
    takes the dot already divided by √|x|² (the 6-bit record's form) and the real |q|²."""
    raw = np.asarray(raw, np.float32)
    one, two = np.float32(1.0), np.float32(2.0)
    with np.errstate(all="ignore"):
        if sim == 0:
            return one / (one + raw)
        if sim == 3:
            return np.where(raw < 0, one / (one - raw), raw + one)
        if sim == 2:
            raw = (raw.astype(np.float64) / np.sqrt(np.float64(qn))).astype(np.float32)
        v = (one + raw) / two
        return np.where(v >= 0, v, np.where(np.isnan(v), v, np.float32(0.0)))


class _X2:
    def __init__(self, x2):
        self.x2 = x2


def sq6_reference(sim: int, rows, queries, dim: int, chunk: int = 2048):
    """The reference's intervals of every (query, row), float64 [nq, n]: the 6-bit tier's (rows at 31 levels,
    the query at 119) real (rlo, rhi) and full (flo, fhi) intervals with centre c and radius r, the int8
    intervals the pilot's bounds rest on (p_rlo, p_rhi, p_flo, p_fhi), and the real dot (d² for EUCLIDEAN) `real`.
    Rows go through in chunks (a 16k × 1536 view would hold gigabytes of float64 otherwise)."""
    from oracle import bounds_reference as BR
    sim = int(sim)
    Q6, Q8 = BR.Quantised(queries, BR.SQ6_QUERY_LEVELS), BR.Quantised(queries)
    keys = ("rlo", "rhi", "flo", "fhi", "c", "r", "p_rlo", "p_rhi", "p_flo", "p_fhi", "real")
    parts = {k: [] for k in keys}
    x2 = []
    for i in range(0, len(rows), chunk):
        R6, R8 = BR.Quantised(rows[i:i + chunk], BR.SQ6_ROW_LEVELS), BR.Quantised(rows[i:i + chunk])
        rlo, rhi, c, r = BR.real_interval(sim, R6, Q6)
        flo, fhi, _, _ = BR.full_interval(sim, R6, Q6, dim)
        p_rlo, p_rhi, _, _ = BR.real_interval(sim, R8, Q8)
        p_flo, p_fhi, _, _ = BR.full_interval(sim, R8, Q8, dim)
        with np.errstate(all="ignore"):
            real = Q6.x @ R6.x.T
            if sim == BR.EUCLIDEAN:
                real = R6.x2[None, :] + Q6.x2[:, None] - 2.0 * real
        for k, v in zip(keys, (rlo, rhi, flo, fhi, c, r, p_rlo, p_rhi, p_flo, p_fhi, real)):
            parts[k].append(v)
        x2.append(R6.x2)
    ref = {k: np.concatenate(v, axis=1) for k, v in parts.items()}
    ref["R"], ref["Q"] = _X2(np.concatenate(x2)), _X2(Q6.x2)     # (the shape test_gpu_bounds' helpers read)
    return ref


class Sq6FullInputs:
    """(A) A view whose shards never get a floor (fewer than k = 10 non-empty wave lists each: one tile per
    segment with tune tiles_target > 0 and tile_min_rows 2048), so every row passes the 6-bit test and is
    recorded.  Shard 0: `O.synth` rows in segments of 1000 and 37; shard 1: 200 more and the edge set at the
    certified scales (constant and zero rows among them); shard 2: rows on the far side of query 0 (every dot
    negative) in segments of 333 and 13.  Every list holds a planted row at a position the pilot does not
    sample (not among the first 4 of the wave's share) whose lower bound for query 0 tops its list."""
    SEGS = [(0, 1000), (0, 37), (1, 221), (2, 333), (2, 13)]      # (shard, rows)
    TILE_MIN_ROWS = 2048

    def __init__(self, sim, dim: int):
        sim = int(sim)
        seed = 9000 + 16 * dim + sim
        self.sim, self.dim = sim, dim
        self.queries = make_queries(dim, sim, seed, CERTIFIED_SCALES)
        rng = np.random.default_rng(seed)
        qp = self.queries[0].astype(np.float64)
        qn = float(np.linalg.norm(qp))
        qhat = qp / qn

        def noise():
            v = rng.standard_normal(dim)
            return v / np.linalg.norm(v)

        synth = O.synth(0, 1237 + 346, dim, seed + 5, DIST[sim])
        norm = float(np.linalg.norm(synth[0].astype(np.float64)))
        far = np.stack([-(0.8 * qhat + 0.6 * noise()) * np.linalg.norm(synth[1237 + i].astype(np.float64))
                        for i in range(346)]).astype(np.float32)
        segs = [synth[:1000].copy(), synth[1000:1037].copy(),
                np.concatenate([synth[1037:1237], scaled(edge_rows(dim, seed + 1), CERTIFIED_SCALES)]),
                far[:333], far[333:]]
        assert [len(s) for s in segs] == [n for _, n in self.SEGS]
        self.seg_shard = [s for s, _ in self.SEGS]
        self.seg_vrow = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
        self.tiles = [(i, sh, 0, n) for i, (sh, n) in enumerate(self.SEGS)]
        self.lists = sq6_wave_lists(self.tiles, self.seg_vrow)
        self.plants = {}                                              # list → view row of its planted row
        for l, (shard, vrows) in enumerate(self.lists):
            if len(vrows) == 0:
                continue
            assert len(vrows) >= 5, "a list too short to hold a row the pilot does not sample"
            seg = self.tiles[l >> 2][0]
            vrow = int(vrows[4 + (5 * l) % (len(vrows) - 4)])
            if shard == 2:
                p = -(0.25 * qhat + 0.97 * noise()) * norm
            elif sim == 0:
                p = qp + noise() * 0.02 * qn
            else:
                # (beside the edge set's large-norm row a dot product tops its list at 8 × the usual norm)
                p = (0.98 * qhat + 0.2 * noise()) * norm * (8.0 if shard == 1 and sim in (1, 3) else 1.0)
            segs[seg][vrow - self.seg_vrow[seg]] = p.astype(np.float32)
            self.plants[l] = vrow
        self.segs = segs
        self.rows = np.concatenate(segs)
        assert in_range(self.rows).all() and in_range(self.queries).all()

    def plant_margin(self, ref, low_limit):
        """The planted rows' lower bounds for query 0 against everything else their lists can publish: for
        each planted list (the least the planted row's bucket may be: `low_limit` [n], the greatest any other
        row's 6-bit lower bound or any pilot row's int8 lower bound may be).  The device's lower side is the
        full interval's (the real one widened by gam·(|x|² + |b|²), which buries the edge rows at 2^20) less
        its 2^-20 slack, so its image does not exceed the full interval's lower image."""
        from oracle import bounds_reference as BR
        lb6 = BR.floor_image(self.sim, ref["flo"][0], ref["fhi"][0], ref["Q"].x2[0], ref["R"].x2)
        lb8 = BR.floor_image(self.sim, ref["p_flo"][0], ref["p_fhi"][0], ref["Q"].x2[0], ref["R"].x2)
        out = []
        for l, vrow in self.plants.items():
            vrows = self.lists[l][1]
            others = np.concatenate([lb6[vrows[vrows != vrow]], lb8[vrows[:4]]])
            out.append((l, float(low_limit[vrow]), float(np.nanmax(others))))
        return out


class Sq6FlooredInputs:
    """(B) 16,384 `O.synth` dist 3 rows in 16 tiles of 1,024 rows (64 wave lists, one per floor bucket; tune
    tiles_target): one segment, or ragged segments over three shards, one with a sparse ord→doc map.  The
    ragged 1536-dim view holds twice the rows in twice the tiles: with 16, 24 and 24 wave lists in its shards
    the pilot's floor alone dropped only 14–19 % of 16,384 rows (test_bounds_reference_cpu.py asks for 20 %)."""
    TILE_MIN_ROWS, N_QUERIES = 1024, 2

    def __init__(self, sim, dim: int, ragged: bool):
        sim = int(sim)
        seed = 9500 + 16 * dim + sim + (8 if ragged else 0)
        self.sim, self.dim, self.ragged = sim, dim, ragged
        self.N = 32768 if ragged and dim == 1536 else 16384
        self.TILES = self.N // 1024
        self.rows = O.synth(0, self.N, dim, seed, 3)
        self.queries = O.synth(0, self.N_QUERIES, dim, seed + 1, 3)
        self.seg_rows = [self.N] if not ragged else [6149, 1237, 5003, 3995] if self.N == 16384 else \
            [12293, 2477, 10003, 7995]
        assert sum(self.seg_rows) == self.N
        self.seg_shard = [0, 1, 1, 2] if ragged else [0]
        rng = np.random.default_rng(seed)
        self.docs = [None] * len(self.seg_rows)
        self.max_doc = list(self.seg_rows)
        if ragged:
            self.max_doc[1] = self.seg_rows[1] + 763
            self.docs[1] = np.sort(rng.choice(self.max_doc[1], self.seg_rows[1], replace=False)).astype(np.int32)
        self.seg_vrow = np.concatenate([[0], np.cumsum(self.seg_rows)]).astype(np.int64)
        self.tiles = tile_table(self.seg_rows, self.seg_shard, self.TILES, self.TILE_MIN_ROWS)
        assert len(self.tiles) == self.TILES
        self.lists = sq6_wave_lists(self.tiles, self.seg_vrow)
        self.shard_of_row = np.concatenate([np.full(n, s) for n, s in zip(self.seg_rows, self.seg_shard)])

    def reference_floors(self, ref, qi: int, k: int):
        """Per shard the floor the pilot alone gives and the highest the pass can reach, from the reference:
        the k-th largest of the 64 bucket maxima of the pilot rows' int8 lower images, and of those and every
        row's 6-bit lower image (scores, float64; 0: no floor)."""
        from oracle import bounds_reference as BR
        qn, xn = ref["Q"].x2[qi], ref["R"].x2
        lb6 = BR.floor_image(self.sim, ref["rlo"][qi], ref["rhi"][qi], qn, xn)
        lb8 = BR.floor_image(self.sim, ref["p_rlo"][qi], ref["p_rhi"][qi], qn, xn)
        n_shards = max(self.seg_shard) + 1
        pilot, final = np.zeros((n_shards, FLOOR_BUCKETS)), np.zeros((n_shards, FLOOR_BUCKETS))
        for l, (shard, vrows) in enumerate(self.lists):
            if len(vrows):
                b = l & (FLOOR_BUCKETS - 1)
                pilot[shard, b] = max(pilot[shard, b], lb8[vrows[:4]].max())
                final[shard, b] = max(final[shard, b], pilot[shard, b], lb6[vrows].max())
        kth = lambda a: np.sort(a, axis=1)[:, ::-1][:, k - 1]
        return kth(pilot), kth(final)

    def shares(self, ref, qi: int, floors, band: float = 0.02):
        """(the share of the view's rows whose 6-bit upper image lies below their shard's floor, the share
        within `band` relative of it)."""
        from oracle import bounds_reference as BR
        ub6 = BR.score_image(self.sim, ref["rlo"][qi], ref["rhi"][qi], ref["Q"].x2[qi], ref["R"].x2)[1]
        t = np.asarray(floors)[self.shard_of_row]
        return float((ub6 < t).mean()), float((np.abs(ub6 / t - 1.0) <= band).mean())


def declared_slack(sim, ref, dim):
    """The raw-domain slack the source declares for the bound's own float arithmetic (osk_device.h
    sq8_bounds): 2^-20·(|approx| + e) per side, e the whole radius; EUCLIDEAN 2^-20·(|x|² + |b|² + 2(|approx|
    + e)) on d² before the (1 ± g2) factor."""
    from oracle import bounds_reference as BR
    R, Q = ref["R"], ref["Q"]
    base = R.x2[None, :] + Q.x2[:, None]
    if int(sim) == BR.EUCLIDEAN:
        return 2.0 ** -20 * (base + 2.0 * (np.abs(ref["c"]) + ref["r"])) * (1.0 + BR.g2(dim))
    return 2.0 ** -20 * (np.abs(ref["c"]) + ref["r"] + BR.gam(dim) * base)


def bucket_low_limit(sim, ref, dim: int, qi: int):
    """The least a floor bucket raised by a row's 6-bit lower bound may be (osk_sq6.hip floor_lb_score), per
    row [n]: the score image of the full interval's low side (high side for EUCLIDEAN) moved out by twice
    sq8_bounds' declared slack, COSINE with |x|² widened by g2 on the side that lowers the score and its
    cosine moved out by two factors of 2^-18 (v_rsq and the explicit one), then lowered by (1 − 2^-18) for
    each remaining declared factor (three in all) and by REL for the float roundings of the transform."""
    from oracle import bounds_reference as BR
    sim = int(sim)
    sl = 2.0 * declared_slack(sim, ref, dim)[qi]
    qn, xn = ref["Q"].x2[qi], ref["R"].x2
    e = 2.0 ** -18
    with np.errstate(all="ignore"):
        if sim == BR.EUCLIDEAN:
            img = BR.score64(sim, ref["fhi"][qi] + sl) * (1.0 - e) ** 3
        elif sim == BR.COSINE:
            lo = ref["flo"][qi] - sl
            c = lo / np.sqrt(qn * np.where(lo >= 0, xn * (1.0 + BR.g2(dim)), xn * (1.0 - BR.g2(dim))))
            c = c - np.abs(c) * 2.0 * e
            img = np.where(np.isnan(c), 0.0, np.maximum((1.0 + c) / 2.0, 0.0)) * (1.0 - e)
        else:
            img = BR.score64(sim, ref["flo"][qi] - sl) * (1.0 - e) ** 3
    return img * (1.0 - REL)


def bucket_high_limit(sim, ref, dim: int, qi: int):
    """The most a floor bucket raised by a row's 6-bit lower bound may be, per row [n]: the lowest score the
    design's model leaves the row — the image of the full interval's low side (high side for EUCLIDEAN), COSINE
    with the row's fp32 |x|² anywhere in |x|²·(1 ± g2), taken on the side that lowers the score (a larger norm
    under a positive dot, a smaller one under a negative dot): what floor_lb_score's g2 is there for."""
    from oracle import bounds_reference as BR
    sim = int(sim)
    qn, xn = ref["Q"].x2[qi], ref["R"].x2
    if sim != BR.COSINE:
        return BR.floor_image(sim, ref["flo"][qi], ref["fhi"][qi], qn, xn)
    lo = ref["flo"][qi]
    with np.errstate(all="ignore"):
        c = lo / np.sqrt(qn * np.where(lo >= 0, xn * (1.0 + BR.g2(dim)), xn * (1.0 - BR.g2(dim))))
        return np.where(np.isnan(c), np.inf, np.maximum((1.0 + c) / 2.0, 0.0))
