"""The oracle's byte path (liboracle: orc_score_i8 / orc_exact_search_i8) against an independent numpy
restatement (oracle/byte_reference.py).  The oracle is the bar of every byte GPU test; this keeps a mistake shared
by the oracle and the kernels (both are C with the same shape) from passing unseen.

Required, at every dim of the GPU byte matrix and on all four similarities, dense and sparse + filtered: docs
equal, score bits equal, visited equal — over the whole leaf (k = rows) and at k = 10.  The corpus carries the
edge set E (all −128, all 127, alternating −128/127, all 0, a duplicate of row 0, all 1) and the queries all −128,
all 127, all 0 and alternating, so the sums reach the ends of their ranges: |Σab| = dim·2^14, d² = dim·255².
"""
import numpy as np
import pytest

from oracle import byte_reference as BR
from oracle import oracle as O

SIMS = [BR.EUCLIDEAN, BR.DOT_PRODUCT, BR.COSINE, BR.MAXIMUM_INNER_PRODUCT]
SIM_IDS = ["EUCLIDEAN", "DOT_PRODUCT", "COSINE", "MAXIMUM_INNER_PRODUCT"]
DIMS = [1, 3, 100, 250, 300, 1000, 1100, 3000, 4096]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def corpus(dim):
    n = 400 + dim % 13
    rows = BR.inject_edges(O.synth(0, n, dim, 900 + dim, 4))
    queries = BR.edge_queries(O.synth(0, 9, dim, 901 + dim, 4))
    return rows, queries


def assert_same(rows, q, k, sim, o2d=None, accept=None):
    ab = None if accept is None else O.bits_from_bool(accept)
    os_, od, ov = O.exact_search(rows, q, k, sim, O.ORDER_DEVICE, ord_to_doc=o2d, accept_bits=ab)
    rs, rd, rv = BR.top_k(rows, q, k, sim, o2d, accept)
    assert ov == rv
    assert np.array_equal(od, rd), (od[:8], rd[:8])
    assert np.array_equal(bits(os_), bits(rs))
    assert len(rs) == 0 or rs.min() >= 0          # every byte score is ≥ 0: key 0 stays the empty slot
    return rs, rd, rv


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("sim", SIMS, ids=SIM_IDS)
def test_oracle_equals_numpy_reference(dim, sim):
    rows, queries = corpus(dim)
    n = len(rows)
    rng = np.random.default_rng(dim)
    max_doc = 3 * n
    o2d = np.sort(rng.choice(max_doc, n, replace=False)).astype(np.int32)
    accept = rng.random(max_doc) < 0.5
    accept[o2d[:6]] = True                        # E's first copy stays accepted
    for q in queries:
        zero_q = not q.any()
        for k in (n, 10):
            rs, rd, rv = assert_same(rows, q, k, sim)
            assert rv == n
            if sim == BR.COSINE:
                nan_rows = int((~rows.any(axis=1)).sum())
                assert nan_rows >= 3 and len(rd) == (0 if zero_q else min(k, n - nan_rows))
            else:
                assert len(rd) == min(k, n)
            rs, rd, rv = assert_same(rows, q, k, sim, o2d, accept)
            assert rv == int(accept[o2d].sum())


@pytest.mark.parametrize("sim", SIMS, ids=SIM_IDS)
def test_pair_scores_at_the_range_ends(sim):
    """orc_score_i8 on E × the edge queries at dim 4096 (the largest sums a field can produce), pair by pair, and
    the values themselves where they are round."""
    dim = 4096
    e = BR.edge_rows(dim)
    qs = np.stack([e[0], e[1], e[2], e[5]])
    for q in qs:
        ref = BR.scores(e, q, sim)
        for j in range(len(e)):
            got = np.float32(O.score(q, e[j], sim))
            assert bits([got])[0] == bits(ref[j:j + 1])[0] or (np.isnan(got) and np.isnan(ref[j])), (j, got, ref[j])
    lo, hi = e[0], e[1]
    if sim == BR.EUCLIDEAN:
        assert BR.scores(hi[None], lo, sim)[0] == np.float32(1.0) / (np.float32(1.0) + np.float32(dim * 255 * 255))
        assert BR.scores(lo[None], lo, sim)[0] == 1.0
    elif sim == BR.DOT_PRODUCT:
        assert BR.scores(lo[None], lo, sim)[0] == 1.0                      # 0.5 + 2^26 / 2^27
        assert BR.scores(hi[None], lo, sim)[0] == np.float32(0.5) - np.float32(128 * 127 / 32768)
    elif sim == BR.COSINE:
        assert BR.scores(lo[None], lo, sim)[0] == 1.0 and BR.scores(hi[None], lo, sim)[0] == 0.0
        assert np.isnan(BR.scores(e[3][None], lo, sim)[0])
    else:
        assert BR.scores(lo[None], lo, sim)[0] == np.float32(2**26 + 1)
        assert BR.scores(e[3][None], lo, sim)[0] == 1.0


def test_ties_take_the_lower_doc():
    rows = np.zeros((50, 4), np.int8)
    rows[:, 0] = np.arange(50) % 5                                         # 10 copies of 5 vectors
    q = np.array([4, 0, 0, 0], np.int8)
    for sim in (BR.EUCLIDEAN, BR.DOT_PRODUCT, BR.MAXIMUM_INNER_PRODUCT):
        rs, rd, _ = assert_same(rows, q, 12, sim)
        assert rd.tolist() == list(range(4, 50, 5)) + [3, 8]
    o2d = (np.arange(50) * 3 + 1).astype(np.int32)
    acc = np.ones(150, bool)
    acc[o2d[4]] = False
    rs, rd, rv = assert_same(rows, q, 3, BR.EUCLIDEAN, o2d, acc)
    assert rd.tolist() == [o2d[9], o2d[14], o2d[19]] and rv == 49
