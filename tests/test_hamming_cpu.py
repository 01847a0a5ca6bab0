"""Binary vectors (OSK_BYTE / OSK_HAMMING) without a device: the C-ABI's argument refusals, the Python constants
and the whole `data_type: binary` / `space_type: hamming` DSL contract (modelled on tests/test_dsl.py)."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

from opensearch_amd import _lib, dsl as Q, lucene as LU
from opensearch_amd._lib import lib, ptr

HEADER = Path(__file__).resolve().parent.parent / "include" / "osknn.h"


def stage(rows, enc, sim):
    """osk_seg_stage of `rows` on device 0 → (return code, last error); a staged segment is released."""
    h = C.c_void_p(None)
    n, dim = rows.shape
    rc = lib().osk_seg_stage(0, ptr(rows), n, dim, enc, sim, None, n, C.byref(h))
    msg = (lib().osk_last_error() or b"").decode()
    if rc == _lib.OSK_OK:
        _lib.check(lib().osk_seg_release(h))
    return rc, msg


# ------------------------------------------------------------------------------------------------
# C-ABI and constants
# ------------------------------------------------------------------------------------------------
def test_constant_matches_header_and_abi_version_stays():
    text = HEADER.read_text()
    m = re.search(r"^#define\s+OSK_HAMMING\s+(\d+)", text, re.M)
    assert m and int(m.group(1)) == _lib.OSK_HAMMING == 4
    assert int(re.search(r"^#define\s+OSK_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == 2 == lib().osk_abi_version()
    at = text.index("#define OSK_HAMMING")
    assert "not a Lucene ordinal" in text[max(0, at - 2500): at]     # (the header says so where it defines it)


def test_lucene_enum_keeps_four_members_and_binary_is_separate():
    assert [m.name for m in LU.VectorSimilarityFunction] == ["EUCLIDEAN", "DOT_PRODUCT", "COSINE",
                                                            "MAXIMUM_INNER_PRODUCT"]
    assert [int(m) for m in LU.VectorSimilarityFunction] == [0, 1, 2, 3]
    assert list(LU.BinarySimilarity) == [LU.BinarySimilarity.HAMMING] and int(LU.BinarySimilarity.HAMMING) == 4
    assert issubclass(LU.GpuBinaryVectorsReader, LU.GpuFlatVectorsReader)


def test_float32_with_hamming_is_invalid_before_the_device():
    rc, msg = stage(np.zeros((4, 8), np.float32), _lib.FLOAT32, _lib.OSK_HAMMING)
    assert rc == _lib.OSK_ERR_INVALID and "hamming" in msg.lower(), (rc, msg)


def test_similarity_five_stays_unknown():
    for enc, rows in ((_lib.BYTE, np.zeros((4, 8), np.int8)), (_lib.FLOAT32, np.zeros((4, 8), np.float32))):
        rc, msg = stage(rows, enc, 5)
        assert rc == _lib.OSK_ERR_INVALID and "unknown similarity" in msg, (rc, msg)
    rc, msg = stage(np.zeros((4, 8), np.int8), _lib.BYTE, -1)
    assert rc == _lib.OSK_ERR_INVALID and "unknown similarity" in msg


def test_byte_with_hamming_passes_the_argument_checks():
    """OSK_OK where there is a device, OSK_ERR_NO_DEVICE where there is none — never OSK_ERR_INVALID."""
    for dim in (1, 16, 4096):
        rc, msg = stage(np.zeros((4, dim), np.int8), _lib.BYTE, _lib.OSK_HAMMING)
        assert rc in (_lib.OSK_OK, _lib.OSK_ERR_NO_DEVICE), (dim, rc, msg)
    rc, msg = stage(np.zeros((4, 4097), np.int8), _lib.BYTE, _lib.OSK_HAMMING)
    assert rc == _lib.OSK_ERR_INVALID and "dim" in msg


def test_ham_stream_knob():
    for v in (0, 1):
        _lib.tune("ham_stream", v)
    with pytest.raises(_lib.OskError):
        _lib.tune("ham_stream", 2)
    _lib.tune("ham_stream", 1)


def test_packed_bytes_input():
    u = np.array([[0, 255, 128, 127]], np.uint8)
    p = LU.GpuBinaryVectorsReader.packed_bytes(u)
    assert p.dtype == np.int8 and p.tolist() == [[0, -1, -128, 127]]
    assert LU.GpuBinaryVectorsReader.packed_bytes(p) is p or np.array_equal(LU.GpuBinaryVectorsReader.packed_bytes(p), p)
    with pytest.raises(ValueError):
        LU.GpuBinaryVectorsReader.packed_bytes(np.zeros((1, 4), np.float32))


# ------------------------------------------------------------------------------------------------
# DSL
# ------------------------------------------------------------------------------------------------
BIN = {"type": "knn_vector", "dimension": 768, "data_type": "binary", "space_type": "hamming"}


def test_binary_mapping_parse_and_round_trip():
    ft = Q.parse_knn_vector_mapping("bits", BIN)
    assert (ft.dimension, ft.vector_length, ft.encoding, ft.similarity) == (768, 96, LU.VectorEncoding.BYTE,
                                                                            LU.BinarySimilarity.HAMMING)
    assert (ft.data_type, ft.space_type, ft.binary) == ("binary", "hamming", True)
    assert ft.to_xcontent() == BIN
    assert Q.parse_knn_vector_mapping("bits", json.loads(json.dumps(ft.to_xcontent()))) == ft
    # space_type omitted → hamming
    dflt = Q.parse_knn_vector_mapping("bits", {"type": "knn_vector", "dimension": 768, "data_type": "binary"})
    assert dflt == ft and dflt.to_xcontent() == BIN
    # with a method
    fm = Q.parse_knn_vector_mapping("bits", dict(BIN, method={"name": "flat", "engine": "gpu"}))
    assert fm.to_xcontent()["method"] == {"name": "flat", "engine": "gpu"}
    # the limits: 8 bits … 8·MAX_DIMENSION bits
    assert Q.parse_knn_vector_mapping("b", dict(BIN, dimension=8)).vector_length == 1
    assert Q.parse_knn_vector_mapping("b", dict(BIN, dimension=8 * Q.MAX_DIMENSION)).vector_length == Q.MAX_DIMENSION
    # float and byte fields are what they were
    f = Q.parse_knn_vector_mapping("f", {"type": "knn_vector", "dimension": 12})
    assert (f.vector_length, f.binary, f.space_type) == (12, False, "l2")
    b = Q.parse_knn_vector_mapping("f", {"type": "knn_vector", "dimension": 12, "data_type": "byte"})
    assert (b.vector_length, b.binary, b.similarity) == (12, False, LU.VectorSimilarityFunction.EUCLIDEAN)


@pytest.mark.parametrize("dimension", [0, 4, 7, 12, 100, -8, 8 * Q.MAX_DIMENSION + 8, 8.0, "768", True, None])
def test_binary_dimension_is_bits_in_multiples_of_eight(dimension):
    with pytest.raises(Q.MapperParsingException):
        Q.parse_knn_vector_mapping("bits", dict(BIN, dimension=dimension))


@pytest.mark.parametrize("node", [
    {"data_type": "binary", "space_type": "l2"}, {"data_type": "binary", "space_type": "innerproduct"},
    {"data_type": "binary", "space_type": "cosinesimil"}, {"data_type": "binary", "space_type": "dot_product"},
    {"data_type": "byte", "space_type": "hamming"}, {"data_type": "float", "space_type": "hamming"},
    {"space_type": "hamming"}])
def test_other_pairings_name_both_parameters(node):
    with pytest.raises(Q.MapperParsingException) as e:
        Q.parse_knn_vector_mapping("bits", dict({"type": "knn_vector", "dimension": 64}, **node))
    assert "space_type" in str(e.value) and "data_type" in str(e.value)


def test_binary_mapping_still_rejects_what_every_mapping_rejects():
    for bad in [dict(BIN, m=16), dict(BIN, method={"name": "hnsw"}), dict(BIN, space_type="l1"),
                {k: v for k, v in BIN.items() if k != "dimension"}, dict(BIN, type="dense_vector")]:
        with pytest.raises(Q.MapperParsingException):
            Q.parse_knn_vector_mapping("bits", bad)


def test_binary_document_vectors():
    ft = Q.parse_knn_vector_mapping("bits", dict(BIN, dimension=32))
    v = Q.parse_document_vector(ft, [-128, 127, 0, -1])
    assert v.dtype == np.int8 and v.tolist() == [-128, 127, 0, -1]
    for bad in ([1, 2, 3], [0] * 32, [1, 2, 3, 4, 5], [1.5, 0, 0, 0], [128, 0, 0, 0], [255, 0, 0, 0],
                [-129, 0, 0, 0], [float("nan"), 0, 0, 0], [[1, 2, 3, 4]]):
        with pytest.raises(Q.MapperParsingException):
            Q.parse_document_vector(ft, bad)


def context():
    return Q.QueryShardContext({"bits": Q.parse_knn_vector_mapping("bits", dict(BIN, dimension=32)), "color": "keyword"},
                               doc_values=lambda leaf, f: np.zeros(leaf.max_doc),
                               parent_docs=lambda leaf, path: np.zeros(leaf.max_doc, bool))


def test_binary_to_query_is_the_byte_knn_query():
    ctx = context()
    b = Q.parse_query({"knn": {"bits": {"vector": [1, -2, 3, -128], "k": 7, "filter": {"term": {"color": "x"}}}}})
    q = b.do_to_query(ctx)
    assert isinstance(q, LU.KnnByteVectorQuery) and q.k == 7 and q.filter is not None
    assert q.target.dtype == np.int8 and q.target.tolist() == [1, -2, 3, -128]
    assert Q.parse_query(json.dumps(b.to_xcontent())) == b and Q.KnnQueryBuilder.read_from(b.write_to()) == b
    # the query vector holds dimension / 8 integers in [-128, 127]
    with pytest.raises(Q.QueryShardException, match="invalid dimension: 32. Dimension should be: 4"):
        Q.KnnQueryBuilder("bits", [0] * 32, 5).do_to_query(ctx)
    with pytest.raises(Q.QueryShardException, match="invalid dimension"):
        Q.KnnQueryBuilder("bits", [1, 2, 3], 5).do_to_query(ctx)
    for bad in ([200, 0, 0, 0], [0.5, 0, 0, 0], [-129, 0, 0, 0]):
        with pytest.raises(Q.MapperParsingException):
            Q.KnnQueryBuilder("bits", bad, 5).do_to_query(ctx)


def test_binary_radial_and_nested_are_refused():
    ctx = context()
    with pytest.raises(Q.QueryShardException, match="radial.*not served for binary fields"):
        Q.KnnQueryBuilder("bits", [1, 2, 3, 4], min_score=0.5).do_to_query(ctx)
    nested = Q.parse_nested_query({"nested": {"path": "chunks", "query": {"knn": {"bits": {"vector": [1, 2, 3, 4],
                                                                                           "k": 3}}}}})
    with pytest.raises(Q.QueryShardException, match="nested.*not served for binary fields"):
        nested.do_to_query(ctx)
