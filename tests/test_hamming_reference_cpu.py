"""tests/hamming_reference.py held to the oracle, without touching it: the Hamming distance of two packed-bit
vectors is the byte-EUCLIDEAN d² of the same bits expanded to 0/1 int8 vectors, and the Hamming score
1 / (1 + d) is that similarity's 1 / (1 + d²).  So `O.exact_search(expand(rows), expand(q), k, EUCLIDEAN)` must
return the reference's docs, score bits and visited — ties, filters and sparse docs included.  Plus answers
computed by hand and a cross-check of every distance with int.bit_count.
"""
import numpy as np
import pytest

import hamming_reference as HR
from opensearch_amd import _lib
from oracle import oracle as O

EUCLIDEAN = 0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def corpus(n, dim, seed, nq=6):
    rows = HR.inject_edges(O.synth(0, n, dim, seed, _lib.DIST_INT8))
    queries = HR.edge_queries(O.synth(0, nq, dim, seed + 1, _lib.DIST_INT8), rows)
    return rows, queries


def test_hand_computed():
    rows = np.array([[0x00, 0x00], [0xFF, 0xFF], [0x0F, 0xF0], [0x01, 0x00], [0x00, 0x00], [0x80, 0x01]], np.uint8)
    q = np.array([0x00, 0x00], np.uint8)
    assert HR.distances(rows, q).tolist() == [0, 16, 8, 1, 0, 2]
    s, d, vis, dist = HR.top_k(rows, q, 4)
    assert d.tolist() == [0, 4, 3, 5] and dist.tolist() == [0, 0, 1, 2] and vis == 6
    assert bits(s).tolist() == bits([1.0, 1.0, 0.5, np.float32(1.0) / np.float32(3.0)]).tolist()
    # int8 input is the same bits
    assert HR.distances(rows.view(np.int8), np.array([-1, -1], np.int8)).tolist() == [16, 0, 8, 15, 16, 14]
    # accept and sparse docs: docs 10, 20, … ; accept drops doc 10 and 50; a stray accepted doc changes nothing
    o2d = np.array([10, 20, 30, 40, 50, 60], np.int32)
    acc = np.zeros(64, bool)
    acc[[20, 30, 40, 60, 61]] = True
    s, d, vis, dist = HR.top_k(rows, q, 10, o2d, acc)
    assert d.tolist() == [40, 60, 30, 20] and dist.tolist() == [1, 2, 8, 16] and vis == 4
    # nothing accepted
    s, d, vis, _ = HR.top_k(rows, q, 3, o2d, np.zeros(64, bool))
    assert len(s) == 0 and len(d) == 0 and vis == 0
    # extremes: distance 0 scores exactly 1.0; 8·dim bits apart scores 1 / (1 + 8·dim), never 0 or NaN
    assert HR.scores_of([0])[0] == np.float32(1.0)
    top = HR.scores_of([8 * 4096])[0]
    assert top == np.float32(1.0) / np.float32(32769.0) and top > 0


@pytest.mark.parametrize("dim", [1, 12, 100])
def test_distances_equal_bit_count(dim):
    rows, queries = corpus(500, dim, 4100 + dim)
    for q in queries:
        want = [sum((int(a) ^ int(b)).bit_count() for a, b in zip(r, q)) for r in rows]
        assert HR.distances(rows, q).tolist() == want
    d = HR.distances(rows, queries[2])
    assert d[7] == 0 and HR.distances(rows, queries[3])[7] == 8 * dim


@pytest.mark.parametrize("dim", [1, 12, 100])
@pytest.mark.parametrize("mode", ["dense", "filtered", "sparse", "sparse-filtered"])
def test_reference_equals_oracle_on_expanded_bits(dim, mode):
    n = 3000
    rows, queries = corpus(n, dim, 4200 + dim)
    rng = np.random.default_rng(dim)
    sparse, filtered = mode.startswith("sparse"), mode.endswith("filtered")
    max_doc = 8000 if sparse else n
    o2d = np.sort(rng.choice(max_doc, n, replace=False)).astype(np.int32) if sparse else None
    accept = rng.random(max_doc) < 0.5 if filtered else None
    ab = None if accept is None else O.bits_from_bool(accept)
    xrows = HR.expand_bits(rows)
    for qi, q in enumerate(queries):
        d = HR.distances(rows, q)
        for k in (1, 50, 1000):
            s, docs, vis, dist = HR.top_k(rows, q, k, o2d, accept, d)
            os_, od, ov = O.exact_search(xrows, HR.expand_bits(q), k, EUCLIDEAN, O.ORDER_DEVICE, ord_to_doc=o2d,
                                         accept_bits=ab)
            assert ov == vis, (dim, mode, qi, k)
            assert np.array_equal(od, docs), (dim, mode, qi, k)
            assert np.array_equal(bits(os_), bits(s)), (dim, mode, qi, k)
            if k == 50 and dim == 1:   # nine distinct scores over 3000 rows: the cut falls inside a tie
                dist51 = HR.top_k(rows, q, 51, o2d, accept, d)[3]
                assert dist51[49] == dist51[50], (mode, qi)
