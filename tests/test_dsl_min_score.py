"""`min_score` on the `knn` query: radial search in place of k (the OpenSearch k-NN plugin's request format),
built into [L] FloatVectorSimilarityQuery / ByteVectorSimilarityQuery.  A query with `k` parses, validates and
serialises exactly as before."""
import json
import struct

import numpy as np
import pytest

from opensearch_amd import dsl as Q
from opensearch_amd.lucene import (ByteVectorSimilarityQuery, FloatVectorSimilarityQuery, KnnFloatVectorQuery)


def test_parse_and_round_trip_min_score():
    body = {"knn": {"emb": {"vector": [0.5, 1.0, -2.0], "min_score": 0.75,
                            "filter": {"term": {"color": "red"}}, "boost": 2.0, "_name": "q1"}}}
    b = Q.parse_query(body)
    assert b.k is None and b.min_score == 0.75 and b.filter == {"term": {"color": "red"}}
    assert b.to_xcontent() == body
    assert Q.parse_query(json.dumps(b.to_xcontent())) == b
    assert Q.KnnQueryBuilder.read_from(b.write_to()) == b
    # an integer threshold is a number too
    assert Q.parse_query({"knn": {"emb": {"vector": [1], "min_score": 1}}}).min_score == 1.0
    plain = Q.KnnQueryBuilder("emb", [1.0, 2.0], min_score=0.25)
    assert plain.to_xcontent() == {"knn": {"emb": {"vector": [1.0, 2.0], "min_score": 0.25}}}
    assert Q.KnnQueryBuilder.read_from(plain.write_to()) == plain
    # float32 on the wire, like the vector: a threshold that float32 holds exactly survives bit for bit
    assert Q.KnnQueryBuilder.read_from(Q.KnnQueryBuilder("e", [1], min_score=0.1).write_to()).min_score == \
        float(np.float32(0.1))


def test_exactly_one_of_k_and_min_score():
    for inner in [{"vector": [1], "k": 3, "min_score": 0.5}, {"vector": [1]}]:
        with pytest.raises(Q.ParsingException):
            Q.parse_query({"knn": {"a": inner}})
    with pytest.raises(ValueError):
        Q.KnnQueryBuilder("a", [1], 3, min_score=0.5)
    with pytest.raises(ValueError):
        Q.KnnQueryBuilder("a", [1])


@pytest.mark.parametrize("bad", [0, 0.0, -0.5, float("nan"), float("inf"), "0.5", None, True, [0.5]])
def test_min_score_must_be_a_finite_positive_number(bad):
    with pytest.raises(Q.ParsingException):
        Q.parse_query({"knn": {"a": {"vector": [1], "min_score": bad}}})
    if bad is not None:
        with pytest.raises(ValueError):
            Q.KnnQueryBuilder("a", [1], min_score=bad)


def _legacy_write_to(field_name, vector, k, filt, boost, query_name) -> bytes:
    """The packing of a k query as it was before min_score existed."""
    name = field_name.encode()
    f = b"" if filt is None else json.dumps(filt, sort_keys=True).encode()
    qn = b"" if query_name is None else query_name.encode()
    vec = np.asarray(vector, np.float32)
    return (struct.pack(">I", len(name)) + name + struct.pack(">I", len(vec)) + vec.astype(">f4").tobytes()
            + struct.pack(">i", k) + struct.pack(">?", filt is not None)
            + struct.pack(">I", len(f)) + f + struct.pack(">f", boost)
            + struct.pack(">?", query_name is not None) + struct.pack(">I", len(qn)) + qn)


def test_k_query_bytes_and_behaviour_unchanged():
    cases = [("emb", [1.0, 2.5, -3.0], 10, None, 1.0, None),
             ("v", [0.25], 1, {"bool": {"must": [{"term": {"c": 1}}]}}, 1.5, "named"),
             ("emb", [7, 8], 10000, {"range": {"n": {"gte": 3}}}, 1.0, None)]
    for name, vec, k, filt, boost, qn in cases:
        b = Q.KnnQueryBuilder(name, vec, k, filt, boost, qn)
        assert b.write_to() == _legacy_write_to(name, vec, k, filt, boost, qn)
        back = Q.KnnQueryBuilder.read_from(b.write_to())
        assert back == b and back.min_score is None and back.k == k
        x = b.to_xcontent()
        assert "min_score" not in x["knn"][name] and x["knn"][name]["k"] == k
        assert Q.parse_query(x) == b
    # a min_score query's bytes differ from every k query's: its k slot is 0, never a valid k
    m = Q.KnnQueryBuilder("emb", [1.0], min_score=0.5).write_to()
    assert m != _legacy_write_to("emb", [1.0], 1, None, 1.0, None)
    assert m[:-4] == _legacy_write_to("emb", [1.0], 0, None, 1.0, None) and m[-4:] == struct.pack(">f", 0.5)
    for bad_k in (0, -1, 10001, 1.5, True):
        with pytest.raises(ValueError):
            Q.KnnQueryBuilder("a", [1], bad_k)


def test_do_to_query_builds_the_similarity_query():
    ctx = Q.QueryShardContext(
        {"emb": Q.parse_knn_vector_mapping("emb", {"type": "knn_vector", "dimension": 4, "space_type": "cosinesimil"}),
         "bytes": Q.parse_knn_vector_mapping("bytes", {"type": "knn_vector", "dimension": 4, "data_type": "byte"}),
         "color": "keyword"},
        doc_values=lambda leaf, f: np.array(["red", "blue", "red"]))
    q = Q.KnnQueryBuilder("emb", [1, 2, 3, 4], min_score=0.9, filter={"term": {"color": "red"}}).do_to_query(ctx)
    assert isinstance(q, FloatVectorSimilarityQuery) and q.result_similarity == pytest.approx(0.9)
    assert q.traversal_similarity <= q.result_similarity and q.target.dtype == np.float32

    class Leaf:
        max_doc = 3
        live_docs = np.array([True, True, False])
    assert q._accept(Leaf()).tolist() == [True, False, False]     # liveDocs ∩ filter
    qb = Q.KnnQueryBuilder("bytes", [1, 2, 3, 4], min_score=0.5).do_to_query(ctx)
    assert isinstance(qb, ByteVectorSimilarityQuery) and qb.target.dtype == np.int8 and qb.filter is None
    assert isinstance(Q.KnnQueryBuilder("emb", [1, 2, 3, 4], 5).do_to_query(ctx), KnnFloatVectorQuery)
    with pytest.raises(Q.QueryShardException, match="invalid dimension"):
        Q.KnnQueryBuilder("emb", [1, 2, 3], min_score=0.5).do_to_query(ctx)
    with pytest.raises(ValueError):
        FloatVectorSimilarityQuery("emb", [1, 2, 3, 4], 0.9, 0.5)    # traversal > result, as Lucene refuses
