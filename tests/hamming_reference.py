"""Hamming k-NN over packed bits, restated in numpy: the reference of test_hamming_reference_cpu.py (which holds it
to the oracle) and of test_gpu_hamming.py (which holds the device to it).

A vector is `dim` bytes = 8·dim bits; d(q, x) = popcount(q XOR x); score = 1 / (1 + d) in float32; hits by score
descending, then doc ascending; visited = the accepted vectors scored.  Nothing here calls the library under test.
"""
import numpy as np

INT32_MAX = 2**31 - 1


def u8(a) -> np.ndarray:
    """int8 or uint8 packed bits as uint8 (the same bit patterns)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype == np.int8 else a.astype(np.uint8, casting="safe")


def distances(rows, q) -> np.ndarray:
    """int64 [n]: popcount(rows[i] XOR q)."""
    rows, q = u8(rows), u8(q)
    assert rows.ndim == 2 and q.shape == (rows.shape[1],)
    return np.unpackbits(rows ^ q[None, :], axis=1).sum(1).astype(np.int64)


def scores_of(d) -> np.ndarray:
    """float32 1 / (1 + d), in float32 operations (d ≤ 32768 converts exactly)."""
    return (np.float32(1.0) / (np.float32(1.0) + np.asarray(d).astype(np.float32))).astype(np.float32)


def top_k(rows, q, k, ord_to_doc=None, accept=None, d=None):
    """One leaf → (scores float32, docs int32, visited, distances int64 of the hits).  accept: bool[max_doc]
    or None; ord_to_doc: ascending docs or None (doc == ord).  `d`: distances(rows, q) if already known."""
    n = len(rows)
    d = distances(rows, q) if d is None else d
    doc = np.arange(n, dtype=np.int64) if ord_to_doc is None else np.asarray(ord_to_doc, np.int64)
    keep = np.ones(n, bool) if accept is None else np.asarray(accept, bool)[doc]
    dk, dock = d[keep], doc[keep]
    order = np.lexsort((dock, dk))[:k]                  # distance ascending = score descending, then doc ascending
    return scores_of(dk[order]), dock[order].astype(np.int32), int(keep.sum()), dk[order]


# ------------------------------------------------------------------------------------------------
# the edge set
# ------------------------------------------------------------------------------------------------
def edge_rows(dim: int) -> np.ndarray:
    """all 0x00, all 0xFF, alternating 0xAA / 0x55, and a duplicate of row 0 (so every placement of the set
    holds two equal rows, and the three placements six)."""
    e = np.zeros((4, dim), np.uint8)
    e[1] = 0xFF
    e[2, 0::2] = 0xAA
    e[2, 1::2] = 0x55
    e[3] = e[0]
    return e


def inject_edges(rows) -> np.ndarray:
    """A copy of `rows` (uint8) with the edge set at rows 0–3, from the middle on and at the end (≥ 16 rows)."""
    rows = u8(rows).copy()
    n, dim = rows.shape
    assert n >= 16
    e = edge_rows(dim)
    for at in (0, n // 2, n - 4):
        rows[at:at + 4] = e
    return rows


def edge_queries(queries, rows) -> np.ndarray:
    """A copy of `queries` (uint8, ≥ 4) whose first four are: all 0x00, all 0xFF, a copy of corpus row 7
    (distance 0, score exactly 1.0) and its complement (distance 8·dim)."""
    q = u8(queries).copy()
    assert len(q) >= 4
    q[0] = 0x00
    q[1] = 0xFF
    q[2] = u8(rows)[7]
    q[3] = ~u8(rows)[7]
    return q


def expand_bits(a) -> np.ndarray:
    """Packed bytes [.., dim] → 0/1 int8 [.., 8·dim]: Hamming distance = byte-EUCLIDEAN d² over these."""
    return np.unpackbits(u8(a), axis=-1).astype(np.int8)
