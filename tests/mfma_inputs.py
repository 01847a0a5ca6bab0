"""Inputs and host restatements shared by test_mfma_reference_cpu.py and test_gpu_mfma_cert.py: the views on
which the bf16×3 batched path (osk_mfma.hip) is held to oracle/mfma_reference.py.

Besides `O.synth` data in each similarity's usual distribution the rows and queries hold bounds_inputs' edge
set at its certified scales, and
  * vectors whose float32 mantissas end 0 1111 1111 0 11 1111 after seven free bits: hi rounds down, lo = the
    eight ones rounds down again, so |lo| is as large as it gets (the dropped lo·lo term is maximal) and the
    residue v − hi − lo sits just below half an ulp of lo — with the rows' signs aligned to the queries', so
    the dropped terms all add up on one side;
  * vectors mixing components near 2^20 and near 2^-20;
  * vectors of one sign throughout (the accumulation error of a positive sum is one-sided);
  * queries whose norm is 1e-4 and 1e4 times the rows';
  * non-negative vectors with the largest component at 2^32 and at 2^-32, rows and queries alike: |q|²·|x|²
    leaves float's range from either end although each norm and every dot product stays in it.
"""
import functools

import numpy as np

import bounds_inputs as BI
from oracle import mfma_reference as MR
from oracle import oracle as O

DIMS = [3, 17, 100, 128, 129, 768, 1000, 4096]
K = 12
KC = MR.KC
N_QUERIES_VISIBLE, N_QUERIES_TILED = 272, 40
UNDECIDABLE = 2e-6


def lolo_vectors(dim: int, seed: int, n: int) -> np.ndarray:
    """Positive float32 [n, dim]: sign 0, exponent 126 … 128, mantissa [7 free bits] 0 1111 1111 0 11 1111."""
    rng = np.random.default_rng(seed)
    top = rng.integers(0, 128, (n, dim)).astype(np.uint32)
    exp = rng.integers(126, 129, (n, dim)).astype(np.uint32)
    bits = (exp << 23) | (top << 16) | np.uint32(0xFF << 7) | np.uint32(0x3F)
    return np.ascontiguousarray(bits, np.uint32).view(np.float32)


def mixed_vectors(dim: int, seed: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, dim)) * np.where(rng.random((n, dim)) < 0.5, 2.0 ** 20, 2.0 ** -20)).astype(np.float32)


def one_sign_vectors(dim: int, seed: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (np.abs(rng.standard_normal((n, dim))) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None]).astype(np.float32)


def pow_vectors(dim: int, seed: int, n: int, e: int) -> np.ndarray:
    """Non-negative vectors whose largest component is exactly 2^e."""
    rng = np.random.default_rng(seed)
    v = np.abs(rng.standard_normal((n, dim))) + 0.05
    v /= v.max(axis=1, keepdims=True)
    return (v * 2.0 ** e).astype(np.float32)


def special_rows(dim: int, seed: int, tame: bool = False) -> np.ndarray:
    """Edge rows at the certified scales, lo·lo rows (three aligned with `special_queries`' signs, one against
    them), mixed-magnitude and one-sign rows.  `tame`: without the rows of large norm (the edge set's last row,
    its 2^20 scale, the mixed-magnitude rows) — the certificate's bound grows with the largest norm of a shard,
    and beside such a row every certificate of DOT_PRODUCT, MAXIMUM_INNER_PRODUCT and EUCLIDEAN fails."""
    sign = np.where(np.random.default_rng(seed + 11).random(dim) < 0.5, -1.0, 1.0).astype(np.float32)
    lolo = lolo_vectors(dim, seed + 12, 4) * sign
    lolo[3] = -lolo[3]
    if tame:
        return np.concatenate([BI.scaled(BI.edge_rows(dim, seed + 1)[:-1], [1.0, 2.0 ** -24]), lolo,
                               one_sign_vectors(dim, seed + 14, 4)])
    return np.concatenate([BI.scaled(BI.edge_rows(dim, seed + 1), BI.CERTIFIED_SCALES), lolo,
                           mixed_vectors(dim, seed + 13, 4), one_sign_vectors(dim, seed + 14, 4)])


def special_queries(dim: int, sim: int, seed: int, row_norm: float) -> np.ndarray:
    """bounds_inputs' queries at the certified scales (edge set, its negation, a cancelling query), lo·lo,
    mixed-magnitude and one-sign queries, and `O.synth` queries at 1e-4 and 1e4 times `row_norm`."""
    sign = np.where(np.random.default_rng(seed + 11).random(dim) < 0.5, -1.0, 1.0).astype(np.float32)
    s = O.synth(0, 4, dim, seed + 25, BI.DIST[int(sim)]).astype(np.float64)
    s *= (row_norm * np.array([1e-4, 1e-4, 1e4, 1e4]) / np.linalg.norm(s, axis=1))[:, None]
    return np.concatenate([BI.make_queries(dim, sim, seed, BI.CERTIFIED_SCALES), lolo_vectors(dim, seed + 22, 4) * sign,
                           mixed_vectors(dim, seed + 23, 4), one_sign_vectors(dim, seed + 24, 4), s.astype(np.float32)])


class View:
    """Segments (rows, ord→doc or None, max_doc, shard) and what the tests derive from them.  View row i is
    row i of `rows` (the segments in order); a segment's doc base is the docs of its shard's earlier segments."""

    def __init__(self, sim, dim, segs, queries, seed, certified=True):
        self.sim, self.dim, self.queries = sim, dim, np.ascontiguousarray(queries, np.float32)
        self.seg_rows = [np.ascontiguousarray(s[0], np.float32) for s in segs]
        self.seg_docs = [s[1] for s in segs]
        self.seg_max_doc = [s[2] for s in segs]
        self.seg_shard = [s[3] for s in segs]
        self.n_shards = max(self.seg_shard) + 1
        self.rows = np.concatenate(self.seg_rows)
        self.seg_vrow = np.concatenate([[0], np.cumsum([len(r) for r in self.seg_rows])]).astype(np.int64)
        self.seg_base, used = [], {}
        for sh, md in zip(self.seg_shard, self.seg_max_doc):
            self.seg_base.append(used.get(sh, 0))
            used[sh] = used.get(sh, 0) + md
        rng = np.random.default_rng(seed + 31)
        self.accept = [rng.random(md) < 0.3 for md in self.seg_max_doc]
        n = len(self.rows)
        self.shard_of_row = np.concatenate([np.full(len(r), sh) for r, sh in zip(self.seg_rows, self.seg_shard)])
        local = [d if d is not None else np.arange(len(r)) for r, d in zip(self.seg_rows, self.seg_docs)]
        self.doc_of_row = np.concatenate([np.asarray(l, np.int64) + b for l, b in zip(local, self.seg_base)])
        self.accepted = np.concatenate([a[l] for a, l in zip(self.accept, local)])
        assert len(self.doc_of_row) == n
        assert not certified or (BI.in_range(self.rows).all() and BI.in_range(self.queries).all())

    def open(self, LU):
        readers, shard_leaves = [], [[] for _ in range(self.n_shards)]
        for i, rows in enumerate(self.seg_rows):
            kw = {} if self.seg_docs[i] is None else dict(ord_to_doc=self.seg_docs[i], max_doc=self.seg_max_doc[i])
            r = LU.GpuFlatVectorsReader("v", rows, self.sim, **kw)
            readers.append(r)
            shard_leaves[self.seg_shard[i]].append(LU.LeafReaderContext(i, self.seg_base[i], r))
        return LU.DeviceShardSet(shard_leaves), readers

    @functools.cached_property
    def scores(self):
        """The oracle's ORDER_DEVICE score of every (query, view row), float32 [nq, n]; NaN: never a hit."""
        return BI.oracle_scores_batch(self.rows, self.queries, int(self.sim), O.ORDER_DEVICE)

    @functools.cached_property
    def qnorm(self):
        return MR.device_norm2(self.queries)

    @functools.cached_property
    def xnorm(self):
        return MR.device_norm2(self.rows)

    @functools.cached_property
    def shard_maxnorm2(self):
        return np.array([self.xnorm[self.shard_of_row == s].max() for s in range(self.n_shards)], np.float32)

    def reference_keys(self, filtered: bool):
        """The candidate lists the reference's approximate scores give: (scores f32, view rows i64, counts),
        [nq, shards, 16] / [nq, shards]; rows −1 past the count."""
        with np.errstate(all="ignore"):
            d = MR.approx_dot(self.rows, self.queries).astype(np.float32)
        a = MR.approx_score(int(self.sim), d, self.qnorm[:, None], self.xnorm[None, :])
        nq = len(self.queries)
        sc = np.zeros((nq, self.n_shards, KC), np.float32)
        vr = np.full((nq, self.n_shards, KC), -1, np.int64)
        cnt = np.zeros((nq, self.n_shards), np.int32)
        for s in range(self.n_shards):
            rows = np.flatnonzero((self.shard_of_row == s) & (self.accepted if filtered else True))
            for q in range(nq):
                order = rows[np.lexsort((rows, -a[q, rows].astype(np.float64)))][:KC]
                cnt[q, s] = len(order)
                sc[q, s, :len(order)], vr[q, s, :len(order)] = a[q, order], order
        return sc, vr, cnt

    def bound(self, sa, c, maxnorm2=None, qnorm=None):
        """U of approximate scores sa [nq, shards, …]; +inf where sa is NaN or ±inf."""
        maxnorm2 = self.shard_maxnorm2 if maxnorm2 is None else maxnorm2
        qnorm = self.qnorm if qnorm is None else qnorm
        sa = np.asarray(sa, np.float64)
        extra = (1,) * (sa.ndim - 2)
        xmax = np.broadcast_to(np.sqrt(maxnorm2.astype(np.float64)).reshape((1, -1) + extra), sa.shape)
        qabs = np.broadcast_to(np.sqrt(np.maximum(qnorm, np.float32(0.0)).astype(np.float64)).reshape((-1, 1) + extra), sa.shape)
        u = MR.U(int(self.sim), sa, c, xmax, qabs)
        return np.where(np.isfinite(sa), u, np.inf)

    def restated_flags(self, sc, vr, cnt, c, maxnorm2=None, qnorm=None):
        """`rescore`'s certificate from candidate lists (scores, view rows, counts): per (query, shard) with 16
        candidates, fail = not (k exact hits among them and the k-th exact score > U(16th approximate score)).
        Returns (fail bool [nq, shards], undecidable bool [nq, shards], e_kth f32 [nq, shards]); a pair is
        undecidable when |e_kth − U| ≤ 2e-6·|U| (device and numpy sqrt may differ in the last bit)."""
        S = self.scores
        nq = len(self.queries)
        full = cnt == KC
        e = np.where(vr >= 0, S[np.arange(nq)[:, None, None], np.maximum(vr, 0)], np.nan)     # [nq, S, 16]
        hits = (~np.isnan(e)).sum(axis=2)
        e_sorted = -np.sort(-np.where(np.isnan(e), -np.inf, e).astype(np.float64), axis=2)
        e_kth = e_sorted[:, :, K - 1]
        u = self.bound(sc[:, :, KC - 1], c, maxnorm2, qnorm)
        with np.errstate(all="ignore"):
            ok = (hits >= K) & (e_kth > u)
            undecidable = full & (hits >= K) & (np.abs(e_kth - u) <= UNDECIDABLE * np.abs(u))
        return full & ~ok, undecidable, e_kth.astype(np.float32)

    def expected(self, filtered: bool, queries=None):
        """[L] exactSearch per leaf merged per shard and across shards, per query: (scores, docs, shards)."""
        out = []
        for qi in range(len(self.queries)) if queries is None else queries:
            shard_hits = []
            for s in range(self.n_shards):
                per_leaf = []
                for i, rows in enumerate(self.seg_rows):
                    if self.seg_shard[i] != s:
                        continue
                    ab = O.bits_from_bool(self.accept[i]) if filtered else None
                    sc, dc, _ = O.exact_search(rows, self.queries[qi], K, int(self.sim), ord_to_doc=self.seg_docs[i],
                                               accept_bits=ab)
                    per_leaf.append((sc, dc + self.seg_base[i]))
                ms, md, _, _, _ = O.topdocs_merge(per_leaf, 0, K, [0] * len(per_leaf))
                shard_hits.append((ms, md))
            es, ed, esh, _, _ = O.topdocs_merge(shard_hits, 0, K, list(range(self.n_shards)))
            out.append((es, ed, esh))
        return out


def _seed(sim, dim):
    return 11000 + 16 * dim + int(sim)


@functools.lru_cache(maxsize=2)
def visible_view(sim, dim) -> View:
    """40 shards of one segment each with 1, 2, … 16 rows in rotation (308 rows) and 272 queries (two query
    blocks, the second mostly padding): every row of a shard is one of its 16 candidates, so "akeys" holds the
    approximate score of every (query, row)."""
    seed = _seed(sim, dim)
    sizes = [1 + i % 16 for i in range(40)]
    n = sum(sizes)
    special = np.concatenate([special_rows(dim, seed), pow_vectors(dim, seed + 15, 24, 32),
                              pow_vectors(dim, seed + 16, 24, -32)])
    synth = O.synth(0, n - len(special), dim, seed, BI.DIST[int(sim)])
    rows = np.concatenate([synth, special])
    row_norm = float(np.median(np.linalg.norm(synth.astype(np.float64), axis=1)))
    qs = np.concatenate([special_queries(dim, sim, seed, row_norm), pow_vectors(dim, seed + 26, 12, 32),
                         pow_vectors(dim, seed + 27, 12, -32)])
    qs = np.concatenate([qs, O.synth(0, N_QUERIES_VISIBLE - len(qs), dim, seed + 5, BI.DIST[int(sim)])])
    cut = np.concatenate([[0], np.cumsum(sizes)])
    segs = [(rows[cut[i]:cut[i + 1]], None, sizes[i], i) for i in range(40)]
    return View(sim, dim, segs, qs, seed)


TILED_SEGS = [1000, 129, 2300]
DUP_ROWS = (TILED_SEGS[0] + TILED_SEGS[1] + 256, 8)      # view rows of the near-duplicate run (tile 2 of segment 2)
TIE_ROWS = 24                                             # rows of a near-tie cluster
Q_DUP, Q_TIE0, Q_TIE1 = 0, 1, 2                           # queries of the tiled view built for a purpose
N_SYNTH_QUERIES_TILED = 12                                # queries 3 … 14: plain `O.synth`


@functools.lru_cache(maxsize=2)
def tiled_view(sim, dim) -> View:
    """2 shards over 3 segments — 1000 rows with a sparse ord→doc map and 129 rows; 2300 rows — and 40 queries.
    Query 0 equals a run of 8 near-duplicate rows inside one 128-row tile, its best matches under every
    similarity (more survivors than the tile's 4 slots per query); queries 1 and 2 each have a near-tie cluster in one shard: 24 copies of the row at rank
    8, scaled by 1 + j·2^-23, so their dot products with the query lie a few ulp apart across ranks 8 … 31 and
    the approximate order among them is arbitrary.

    The certificate's bound grows with the shard's largest norm and with |q|, and under a tiny query every
    DOT_PRODUCT / MAXIMUM_INNER_PRODUCT score sits within the bound's own 1e-6·|U| of it, so beside the rows of
    large norm and under the queries of small norm no flag could be restated: this view leaves both out (`tame`
    rows, queries of at least 1e-2 of the rows' norm).  Those rows and queries therefore meet the quick tests and
    the survivor slots nowhere: they are in the visible view only, whose every tile overflows to the full path."""
    seed = _seed(sim, dim) + 7
    rng = np.random.default_rng(seed)
    n = sum(TILED_SEGS)
    special = special_rows(dim, seed, tame=True)
    rows = np.concatenate([O.synth(0, n - len(special), dim, seed, BI.DIST[int(sim)]), special])
    rows = rows[rng.permutation(n)]
    row_norm = float(np.median(np.linalg.norm(rows[:200].astype(np.float64), axis=1)))
    n_fill = N_QUERIES_TILED - 3 - N_SYNTH_QUERIES_TILED
    sq = special_queries(dim, sim, seed, row_norm)
    # (under a zero or tiny query every DOT_PRODUCT score is 0.5 and every MAXIMUM_INNER_PRODUCT score 1 to within
    # the bound's own 1e-6·|U| term, too close to the bound to restate the flag; the visible view asks those)
    sq = sq[np.linalg.norm(sq.astype(np.float64), axis=1) >= 1e-2 * row_norm]
    qs = np.concatenate([O.synth(0, 3 + N_SYNTH_QUERIES_TILED, dim, seed + 5, BI.DIST[int(sim)]),
                         sq[rng.permutation(len(sq))[:n_fill]]])
    # the near-duplicate run: the query and 7 copies with one component moved by an ulp; the query has twice the
    # largest norm among the rows, so that under every similarity the run is its best match
    d0, nd = DUP_ROWS
    q0 = qs[Q_DUP].astype(np.float64)
    qs[Q_DUP] = (q0 / np.linalg.norm(q0) * 2.0 * np.linalg.norm(rows.astype(np.float64), axis=1).max()).astype(np.float32)
    rows[d0:d0 + nd] = qs[Q_DUP]
    for j in range(1, nd):
        rows[d0 + j, j % dim] = np.nextafter(rows[d0 + j, j % dim], np.float32(np.inf))
    # near-tie clusters: one in shard 0 (view rows 0 … 1128) for query 1, one in shard 1 for query 2
    cut = np.concatenate([[0], np.cumsum(TILED_SEGS)])
    for q, lo, hi in ((Q_TIE0, 0, cut[2]), (Q_TIE1, cut[2], n)):
        sc, dc, _ = O.exact_search(rows[lo:hi], qs[q], 9, int(sim))
        base = rows[lo + dc[8]].astype(np.float64)
        free = np.setdiff1d(np.arange(lo, hi), np.concatenate([lo + dc, np.arange(d0, d0 + nd)]))
        at = rng.choice(free, TIE_ROWS, replace=False)
        rows[at] = np.stack([base * (1.0 + j * 2.0 ** -23) for j in range(TIE_ROWS)]).astype(np.float32)
    docs0 = np.sort(rng.choice(1700, TILED_SEGS[0], replace=False)).astype(np.int32)
    segs = [(rows[cut[0]:cut[1]], docs0, 1700, 0), (rows[cut[1]:cut[2]], None, TILED_SEGS[1], 0),
            (rows[cut[2]:cut[3]], None, TILED_SEGS[2], 1)]
    return View(sim, dim, segs, qs, seed)


@functools.lru_cache(maxsize=2)
def extreme_view(sim, dim) -> View:
    """Rows the int8 paths refuse (the edge set at 2^-70 … 2^63 among `O.synth` rows) in two shards, asked
    bounds_inputs' queries at every scale: the batched path serves such a view at any batch ≥ mfma_min_batch."""
    seed = _seed(sim, dim) + 13
    rows = BI.make_rows(900, dim, sim, seed, BI.SCALES)
    rows = rows[np.random.default_rng(seed).permutation(len(rows))]
    qs = BI.make_queries(dim, sim, seed, BI.ALL_SCALES)
    return View(sim, dim, [(rows[:600], None, 600, 0), (rows[600:], None, len(rows) - 600, 1)], qs, seed,
                certified=False)


@functools.lru_cache(maxsize=2)
def pow_view(sim, dim, e) -> View:
    """One shard of 700 non-negative rows whose largest component is 2^e, and 20 such queries (e = ±32: the
    product of the norms' squares leaves float's range).  The rows nearest each query are not among the first."""
    seed = _seed(sim, dim) + 19 + (1 if e > 0 else 0)
    rows = pow_vectors(dim, seed, 700, e)
    qs = pow_vectors(dim, seed + 1, 20, e)
    near = rows[300:310].astype(np.float64) * 0.75 + qs[:10].astype(np.float64) * 0.25
    qs[:10] = (near / near.max(axis=1, keepdims=True) * 2.0 ** e).astype(np.float32)
    return View(sim, dim, [(rows, None, 700, 0)], qs, seed)


PILOT_ROWS, PILOT_LATE = 512, 300                        # 4 tiles in one unit (mfma_units 1); the 16th best row


@functools.lru_cache(maxsize=2)
def pilot_view(sim, dim) -> View:
    """One shard of 512 unit-norm rows, searched as one unit of 4 tiles, and 16 unit-norm queries within 1e-3 of
    one direction: rows 0 … 14 (the pilot tile) are every query's 15 best (cosine 0.90, 0.89, … 0.76), row 300
    (tile 2) its 16th (0.7), the rest of tile 0 lies near cosine 0.3 and the rest of tiles 1 … 3 near −0.3.  With
    equal norms every similarity orders rows by cosine.  Tile 0 overflows its slots (15 survivors) and takes the
    full path; tile 2 has one survivor per query — row 300, which a pilot threshold taken one place too high
    (the 15th score instead of the 16th) drops."""
    seed = _seed(sim, dim) + 29
    rng = np.random.default_rng(seed)
    qhat = rng.standard_normal(dim)
    qhat /= np.linalg.norm(qhat)

    def perp():
        v = rng.standard_normal(dim)
        v -= (v @ qhat) * qhat
        return v / np.linalg.norm(v)

    cos = np.where(np.arange(PILOT_ROWS) < 128, 0.3, -0.3) + rng.uniform(-0.05, 0.05, PILOT_ROWS)
    cos[:15] = 0.90 - 0.01 * np.arange(15)
    cos[PILOT_LATE] = 0.7
    rows = np.stack([c * qhat + np.sqrt(1.0 - c * c) * perp() for c in cos]).astype(np.float32)
    qs = np.stack([qhat + 1e-3 * perp() for _ in range(16)])
    qs = (qs / np.linalg.norm(qs, axis=1, keepdims=True)).astype(np.float32)
    return View(sim, dim, [(rows, None, PILOT_ROWS, 0)], qs, seed)
