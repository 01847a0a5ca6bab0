"""An independent restatement of Lucene's byte-vector scoring and exact search, in plain numpy.

TEST INFRASTRUCTURE ONLY, like the rest of oracle/: imported by tests/, never by opensearch_amd/.

liboracle's `orc_score_i8` / `orc_exact_search_i8` are the bar of every byte GPU test; this module restates
the same operations without sharing a line with them, so a mistake in one is caught by the other
(tests/test_byte_reference_cpu.py).  Every sum is an int64 numpy reduction, asserted to fit Java's int; the
float steps are the ones `VectorSimilarityFunction.compare(byte[], byte[])` performs (lucene-core 10.3.0,
restated in osk_common.h):

    EUCLIDEAN              1f / (1f + (float) d²)             d² = Σ(q−x)², from the differences
    DOT_PRODUCT            0.5f + (float) dot / (float)(dim · 2^15)
    COSINE                 (1f + (float)((double) dot / sqrt((double) |q|² · (double) |x|²))) / 2f
    MAXIMUM_INNER_PRODUCT  scaleMaxInnerProductScore((float) dot): dot < 0 ? 1/(1 + −1·dot) : dot + 1
"""
from __future__ import annotations

import numpy as np

EUCLIDEAN, DOT_PRODUCT, COSINE, MAXIMUM_INNER_PRODUCT = 0, 1, 2, 3
INT32_MAX = 2**31 - 1
_CHUNK = 1024

_F1, _F2, _FH = np.float32(1.0), np.float32(2.0), np.float32(0.5)


def _int32(a: np.ndarray) -> np.ndarray:
    """An int64 sum that Java holds in an int: it must fit."""
    assert a.dtype == np.int64
    assert a.size == 0 or (int(a.min()) >= -2**31 and int(a.max()) <= INT32_MAX), "sum leaves the int32 range"
    return a


def scores(rows: np.ndarray, q: np.ndarray, sim: int) -> np.ndarray:
    """float32 score of every row of int8 `rows` [n, dim] against the int8 query `q` [dim] (NaN: COSINE with a
    zero vector on either side)."""
    rows, q = np.asarray(rows), np.asarray(q)
    assert rows.dtype == np.int8 and q.dtype == np.int8 and rows.ndim == 2 and q.shape == (rows.shape[1],)
    sim = int(sim)
    n, dim = rows.shape
    out = np.empty(n, np.float32)
    q32 = q.astype(np.int32)
    n1 = _int32(np.sum(q32 * q32, dtype=np.int64, keepdims=True))[0]
    for r0 in range(0, n, _CHUNK):
        x32 = rows[r0:r0 + _CHUNK].astype(np.int32)
        o = out[r0:r0 + _CHUNK]
        if sim == EUCLIDEAN:
            diff = x32 - q32                                     # |diff| ≤ 255: its square fits an int32
            d2 = _int32(np.sum(diff * diff, axis=1, dtype=np.int64))
            o[:] = _F1 / (_F1 + d2.astype(np.float32))
            continue
        dot = _int32(np.sum(x32 * q32, axis=1, dtype=np.int64))
        if sim == DOT_PRODUCT:
            o[:] = _FH + dot.astype(np.float32) / np.float32(dim * (1 << 15))
        elif sim == COSINE:
            n2 = _int32(np.sum(x32 * x32, axis=1, dtype=np.int64))
            with np.errstate(divide="ignore", invalid="ignore"):
                c = (dot.astype(np.float64) / np.sqrt(np.float64(n1) * n2.astype(np.float64))).astype(np.float32)
            o[:] = (_F1 + c) / _F2
        elif sim == MAXIMUM_INNER_PRODUCT:
            f = dot.astype(np.float32)
            with np.errstate(divide="ignore"):
                o[:] = np.where(f < 0, _F1 / (_F1 + np.float32(-1.0) * f), f + _F1)
        else:
            raise ValueError(f"unknown similarity {sim}")
    return out


def top_k_of(sc: np.ndarray, k: int, ord_to_doc=None, accept=None):
    """[L] exactSearch over rows already scored: the accepted rows (accept: bool over the leaf's docs) by score
    descending, then doc ascending, cut to k; a NaN score is visited but never a hit.
    → (scores f32, docs i32, visited)."""
    sc = np.asarray(sc, np.float32)
    docs = np.arange(len(sc), dtype=np.int64) if ord_to_doc is None else np.asarray(ord_to_doc, np.int64)
    assert len(docs) == len(sc)
    if accept is not None:
        ok = np.asarray(accept, dtype=bool)[docs]
        sc, docs = sc[ok], docs[ok]
    visited = len(sc)
    hit = ~np.isnan(sc)
    sc, docs = sc[hit], docs[hit]
    order = np.lexsort((docs, -sc.astype(np.float64)))[:k]
    return sc[order].copy(), docs[order].astype(np.int32), visited


def top_k(rows, q, k: int, sim: int, ord_to_doc=None, accept=None):
    return top_k_of(scores(rows, q, sim), k, ord_to_doc, accept)


# ------------------------------------------------------------------------------------------------
# the edge set of the byte tests
# ------------------------------------------------------------------------------------------------
def edge_rows(dim: int) -> np.ndarray:
    """E: all −128, all 127, alternating −128/127, all 0 (NaN under COSINE), a duplicate of row 0, all 1."""
    e = np.zeros((6, dim), np.int8)
    e[0] = -128
    e[1] = 127
    e[2, 0::2] = -128
    e[2, 1::2] = 127
    e[4] = e[0]
    e[5] = 1
    return e


def edge_positions(n: int) -> list[int]:
    """Where E goes in a corpus of n ≥ 18 rows: rows 0–5, six rows from the middle on (7 apart, so in other row
    groups and waves), and the last six in reverse."""
    assert n >= 18
    mid = [min(n // 2 + 7 * i, n - 7) for i in range(6)]
    return list(range(6)) + mid + [n - 1 - i for i in range(6)]


def inject_edges(rows: np.ndarray) -> np.ndarray:
    """`rows` with E written in place at edge_positions (short corpora: as many rows of E as fit, from row 0)."""
    n, dim = rows.shape
    e = edge_rows(dim)
    if n < 18:
        rows[: min(n, 6)] = e[: min(n, 6)]
        return rows
    for j, p in enumerate(edge_positions(n)):
        rows[p] = e[j % 6]
    return rows


def edge_queries(queries: np.ndarray) -> np.ndarray:
    """`queries` with all −128 at 0, all 127 at 1 and, when there are that many, all 0 at 4 and alternating
    127/−128 at 8 (the single-query tail of a 9-query batch), in place."""
    nq = len(queries)
    if nq > 0:
        queries[0] = -128
    if nq > 1:
        queries[1] = 127
    if nq > 4:
        queries[4] = 0
    if nq > 8:
        queries[8, 0::2] = 127
        queries[8, 1::2] = -128
    return queries
