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

