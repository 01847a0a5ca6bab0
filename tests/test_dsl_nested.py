"""`nested` around a `knn` query (the OpenSearch k-NN plugin's nested-field search): the builder's XContent, and
`do_to_query` building [L] DiversifyingChildrenFloat/ByteKnnVectorQuery exactly when the shard context carries a
parent filter.  A plain `knn` query parses, builds and serialises as before."""
import json
import struct

import numpy as np
import pytest

from opensearch_amd import dsl as Q
from opensearch_amd.lucene import (DiversifyingChildrenByteKnnVectorQuery, DiversifyingChildrenFloatKnnVectorQuery,
                                   FloatVectorSimilarityQuery, KnnByteVectorQuery, KnnFloatVectorQuery)

KNN = {"knn": {"chunks.emb": {"vector": [1.0, 2.0, 3.0, 4.0], "k": 3, "filter": {"term": {"color": "red"}}}}}


def _ctx(**kw):
    return Q.QueryShardContext(
        {"chunks.emb": Q.parse_knn_vector_mapping("chunks.emb", {"type": "knn_vector", "dimension": 4,
                                                                 "space_type": "cosinesimil"}),
         "chunks.bytes": Q.parse_knn_vector_mapping("chunks.bytes", {"type": "knn_vector", "dimension": 4,
                                                                     "data_type": "byte"}),
         "color": "keyword"},
        doc_values=lambda leaf, f: np.array(["red", "blue", "red", "red"]), **kw)


def test_nested_xcontent_round_trip():
    body = {"nested": {"path": "chunks", "query": KNN, "score_mode": "max"}}
    b = Q.parse_nested_query(body)
    assert b.path == "chunks" and b.score_mode == "max" and b.query == Q.parse_query(KNN)
    assert b.to_xcontent() == body
    assert Q.parse_nested_query(json.dumps(b.to_xcontent())) == b
    # score_mode defaults to max and is always written
    short = Q.parse_nested_query({"nested": {"path": "chunks", "query": KNN}})
    assert short == b and short.to_xcontent() == body
    assert Q.NestedQueryBuilder("chunks", Q.parse_query(KNN)) == b


@pytest.mark.parametrize("body", [
    {"nested": {"path": "chunks", "query": KNN, "ignore_unmapped": True}},      # an unknown field
    {"nested": {"path": "chunks", "query": KNN, "inner_hits": {}}},
    {"nested": {"query": KNN}},                                                 # no path
    {"nested": {"path": "chunks"}},                                             # no query
    {"nested": {"path": "", "query": KNN}},
    {"nested": {"path": "chunks", "query": {"match_all": {}}}},                 # not a knn query
    {"nested": {"path": "chunks", "query": {"knn": {"a": {"vector": [1], "k": 3, "bogus": 1}}}}},
    {"nested": {"path": "chunks", "query": KNN, "score_mode": "median"}},
    {"nested": {"path": "chunks", "query": KNN, "score_mode": "avg"}},          # a real mode, not served
    {"nested": ["chunks"]},
    {"knn": KNN["knn"]},                                                        # not a nested query
    {"nested": {"path": "chunks", "query": KNN}, "boost": 2},
], ids=lambda b: json.dumps(b)[:60])
def test_nested_parse_errors(body):
    with pytest.raises(Q.ParsingException):
        Q.parse_nested_query(body)


def test_do_to_query_builds_the_diversifying_query_only_under_a_parent_filter():
    parents = np.array([False, False, False, True])
    seen = []

    def parent_docs(leaf, path):
        seen.append(path)
        return parents
    ctx = _ctx(parent_docs=parent_docs)

    class Leaf:
        max_doc = 4
        live_docs = np.array([True, True, False, True])

    q = Q.parse_nested_query({"nested": {"path": "chunks", "query": KNN}}).do_to_query(ctx)
    assert isinstance(q, DiversifyingChildrenFloatKnnVectorQuery) and q.k == 3 and q.target.dtype == np.float32
    assert q.parents_filter(Leaf()) is parents and seen == ["chunks"]
    assert q._accept(Leaf()).tolist() == [True, False, False, True]             # liveDocs ∩ child filter
    qb = Q.NestedQueryBuilder("chunks", Q.KnnQueryBuilder("chunks.bytes", [1, 2, 3, 4], 5)).do_to_query(ctx)
    assert isinstance(qb, DiversifyingChildrenByteKnnVectorQuery) and qb.target.dtype == np.int8 and qb.filter is None
    # the same knn builder outside `nested`: the plain query, whether or not the shard has nested docs
    for plain_ctx in (ctx, _ctx()):
        p = Q.parse_query(KNN).do_to_query(plain_ctx)
        assert type(p) is KnnFloatVectorQuery
        assert type(Q.KnnQueryBuilder("chunks.bytes", [1, 2, 3, 4], 5).do_to_query(plain_ctx)) is KnnByteVectorQuery
        m = Q.KnnQueryBuilder("chunks.emb", [1, 2, 3, 4], min_score=0.5).do_to_query(plain_ctx)
        assert type(m) is FloatVectorSimilarityQuery
    assert ctx.parent_filter is None                                            # the outer context is not changed
    # a shard without nested docs cannot run the nested query
    with pytest.raises(Q.QueryShardException, match="nested"):
        Q.parse_nested_query({"nested": {"path": "chunks", "query": KNN}}).do_to_query(_ctx())
    with pytest.raises(Q.QueryShardException, match="invalid dimension"):
        Q.NestedQueryBuilder("chunks", Q.KnnQueryBuilder("chunks.emb", [1, 2], 5)).do_to_query(ctx)


def test_min_score_under_nested_raises():
    ctx = _ctx(parent_docs=lambda leaf, path: np.array([False, True]))
    b = Q.parse_nested_query({"nested": {"path": "chunks",
                                         "query": {"knn": {"chunks.emb": {"vector": [1, 2, 3, 4], "min_score": 0.5}}}}})
    with pytest.raises(Q.QueryShardException, match="min_score"):
        b.do_to_query(ctx)


def test_context_defaults_leave_existing_callers_untouched():
    ctx = Q.QueryShardContext({"a": "keyword"})
    assert ctx.parent_docs is None and ctx.parent_filter is None and ctx.doc_values is None
    ctx2 = Q.QueryShardContext({"a": "keyword"}, lambda leaf, f: None)           # the positional form still works
    assert ctx2.doc_values is not None and ctx2.parent_filter is None


def _legacy_write_to(field_name, vector, k, filt, boost, query_name) -> bytes:
    """The packing of a k query as it has always been."""
    name = field_name.encode()
    f = b"" if filt is None else json.dumps(filt, sort_keys=True).encode()
    qn = b"" if query_name is None else query_name.encode()
    vec = np.asarray(vector, np.float32)
    return (struct.pack(">I", len(name)) + name + struct.pack(">I", len(vec)) + vec.astype(">f4").tobytes()
            + struct.pack(">i", k) + struct.pack(">?", filt is not None)
            + struct.pack(">I", len(f)) + f + struct.pack(">f", boost)
            + struct.pack(">?", query_name is not None) + struct.pack(">I", len(qn)) + qn)


def test_knn_parse_and_wire_bytes_unchanged():
    b = Q.parse_query(KNN)
    assert isinstance(b, Q.KnnQueryBuilder) and b.to_xcontent() == KNN
    inner = KNN["knn"]["chunks.emb"]
    assert b.write_to() == _legacy_write_to("chunks.emb", inner["vector"], 3, inner["filter"], 1.0, None)
    assert Q.KnnQueryBuilder.read_from(b.write_to()) == b
    nested = Q.NestedQueryBuilder("chunks", b)
    assert nested.query.write_to() == b.write_to()                              # wrapping changes nothing inside
    with pytest.raises(Q.ParsingException):
        Q.parse_query({"nested": {"path": "chunks", "query": KNN}})             # parse_query stays the knn parser
