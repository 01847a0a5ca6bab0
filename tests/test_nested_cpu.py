"""The nested k-NN entries of the C-ABI on a machine without a GPU — exported, bound by the ctypes table and by
OsKnn.java, argument errors refused before the device is touched, a valid call without a device failing loudly with
OSK_ERR_NO_DEVICE — and the numpy reference of tests/test_gpu_nested.py checked against a brute-force loop written
straight from [L] DiversifyingChildren*KnnVectorQuery.exactSearch."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from opensearch_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_gpu_nested as N   # noqa: E402  (the reference under test lives with the GPU tests)

OSKNN_JAVA = ROOT / "java" / "plugin" / "src" / "main" / "java" / "org" / "opensearch" / "knn" / "gpu" / "OsKnn.java"
NAMES = ["osk_seg_set_parents", "osk_seg_parents", "osk_seg_search_nested", "osk_view_search_nested",
         "osk_view_search_nested_device"]


def _err() -> str:
    return _lib.lib().osk_last_error().decode()


def test_symbols_exported_and_bound():
    L = C.CDLL(str(_lib.LIB_PATH))
    T = C.CDLL(str(_lib.TESTING_LIB_PATH))
    java = re.sub(r"//[^\n]*", "", OSKNN_JAVA.read_text())
    header = (ROOT / "include" / "osknn.h").read_text()
    for name in NAMES:
        assert hasattr(L, name) and hasattr(T, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(rf'h\(\s*"{name}"\s*,\s*FunctionDescriptor\.of\(', java), name
        assert re.search(rf"\b{name}\s*\(", header), name
    # the search entries mirror their k-NN twins argument for argument
    for nested, knn in (("osk_seg_search_nested", "osk_seg_search"), ("osk_view_search_nested", "osk_view_search"),
                        ("osk_view_search_nested_device", "osk_view_search_device")):
        assert _lib.SIGNATURES[nested] == _lib.SIGNATURES[knn]
    assert _lib.lib().osk_abi_version() == 2


def _bufs(nq=1, k=4, size=4):
    return dict(h=(C.c_uint8 * 4096)(), q=np.zeros((nq, 8), np.float32),
                scores=np.full(nq * max(k, size), -7, np.float32), docs=np.full(nq * max(k, size), -7, np.int32),
                shard=np.full(nq * size, -7, np.int32), count=np.full(nq, -7, np.int32),
                total=np.full(nq, -7, np.int64), mx=np.full(nq, -7, np.float32), visited=np.full(nq, -7, np.int64),
                keys=np.full(nq * k, 7, np.uint64))


def _seg_call(b, **over):
    a = dict(seg=C.addressof(b["h"]), q=b["q"].ctypes.data, nq=1, k=4, acc=None, scores=b["scores"].ctypes.data,
             docs=b["docs"].ctypes.data, count=b["count"].ctypes.data, visited=b["visited"].ctypes.data)
    a.update(over)
    return _lib.lib().osk_seg_search_nested(a["seg"], a["q"], a["nq"], a["k"], a["acc"], a["scores"], a["docs"],
                                            a["count"], a["visited"])


def _view_call(b, **over):
    a = dict(view=C.addressof(b["h"]), q=b["q"].ctypes.data, nq=1, k=4, from_=0, size=4, acc=None,
             scores=b["scores"].ctypes.data, docs=b["docs"].ctypes.data, shard=b["shard"].ctypes.data,
             count=b["count"].ctypes.data, total=b["total"].ctypes.data, mx=b["mx"].ctypes.data)
    a.update(over)
    return _lib.lib().osk_view_search_nested(a["view"], a["q"], a["nq"], a["k"], a["from_"], a["size"], a["acc"],
                                             a["scores"], a["docs"], a["shard"], a["count"], a["total"], a["mx"])


def _device_call(b, **over):
    a = dict(view=C.addressof(b["h"]), q=b["q"].ctypes.data, nq=1, k=4, acc=None, keys=b["keys"].ctypes.data,
             count=b["count"].ctypes.data)
    a.update(over)
    return _lib.lib().osk_view_search_nested_device(a["view"], a["q"], a["nq"], a["k"], a["acc"], a["keys"],
                                                    a["count"], None, None)


def _untouched(b):
    return np.all(b["docs"] == -7) and np.all(b["count"] == -7) and np.all(b["keys"] == 7)


_ids = lambda d: next(iter(d)) + "=" + str(next(iter(d.values())))   # noqa: E731
COMMON = [dict(q=None), dict(count=None), dict(nq=0), dict(nq=-3), dict(k=0), dict(k=-1)]


@pytest.mark.parametrize("bad", COMMON + [dict(seg=None), dict(scores=None), dict(docs=None)], ids=_ids)
def test_seg_entry_rejects_bad_arguments_before_the_device(bad):
    b = _bufs()
    assert _seg_call(b, **bad) == _lib.OSK_ERR_INVALID
    assert _err() != "" and _untouched(b)


@pytest.mark.parametrize("bad", COMMON + [dict(view=None), dict(scores=None), dict(docs=None), dict(shard=None),
                                          dict(total=None), dict(mx=None), dict(from_=-1), dict(size=0)], ids=_ids)
def test_view_entry_rejects_bad_arguments_before_the_device(bad):
    b = _bufs()
    assert _view_call(b, **bad) == _lib.OSK_ERR_INVALID
    assert _err() != "" and _untouched(b)


@pytest.mark.parametrize("bad", COMMON + [dict(view=None), dict(keys=None)], ids=_ids)
def test_device_entry_rejects_bad_arguments_before_the_device(bad):
    b = _bufs()
    assert _device_call(b, **bad) == _lib.OSK_ERR_INVALID
    assert _err() != "" and _untouched(b)


def test_k_beyond_the_scan_lists_is_unsupported_before_the_device():
    b = _bufs(k=65, size=65)
    for call in (_seg_call, _view_call, _device_call):
        assert call(b, k=65) == _lib.OSK_ERR_UNSUPPORTED
        assert "64" in _err() and _untouched(b)
    assert _seg_call(b, k=0) == _lib.OSK_ERR_INVALID and "k" in _err()
    assert _seg_call(b, nq=0) == _lib.OSK_ERR_INVALID and "n_queries" in _err()


def test_set_parents_rejects_null_arguments():
    h = (C.c_uint8 * 4096)()
    bits = np.ones(4, np.uint64)
    assert _lib.lib().osk_seg_set_parents(None, bits.ctypes.data) == _lib.OSK_ERR_INVALID
    assert _lib.lib().osk_seg_set_parents(C.addressof(h), None) == _lib.OSK_ERR_INVALID
    assert _lib.lib().osk_seg_parents(None, None) == _lib.OSK_ERR_INVALID


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_valid_calls_fail_loudly_without_a_device():
    b = _bufs()
    for call in (_seg_call, _view_call, _device_call):
        assert call(b) == _lib.OSK_ERR_NO_DEVICE and "no HIP device" in _err()
    bits = np.ones(4, np.uint64)
    assert _lib.lib().osk_seg_set_parents(C.addressof(b["h"]), bits.ctypes.data) == _lib.OSK_ERR_NO_DEVICE
    assert _untouched(b)


# ------------------------------------------------------------------------------------------------
# the reference of the GPU tests against Lucene's loop
# ------------------------------------------------------------------------------------------------
def lucene_exact_search(child_docs, scores, accept, parent_mask, k):
    """[L] DiversifyingChildren*KnnVectorQuery.exactSearch: children in doc order; the parent of child d is
    parentBitSet.nextSetBit(d); a parent's entry is replaced only by a strictly greater score (`score >
    currentScore`; false for NaN, and a NaN never opens an entry); the k best entries by score desc, child doc
    asc."""
    best: dict[int, tuple[float, int]] = {}
    visited = 0
    for d, s in sorted(zip(child_docs.tolist(), scores.tolist())):
        if accept is not None and not accept[d]:
            continue
        visited += 1
        parent = d
        while not parent_mask[parent]:          # nextSetBit, inclusive
            parent += 1
        cur = best.get(parent)
        if s != s:
            continue
        if cur is None or s > cur[0]:
            best[parent] = (s, d)
    out = sorted(best.values(), key=lambda e: (-e[0], e[1]))[:k]
    return np.array([e[1] for e in out], np.int64), np.array([e[0] for e in out], np.float32), visited


@pytest.mark.parametrize("seed", range(6))
def test_numpy_reference_matches_the_lucene_loop(seed):
    rng = np.random.default_rng(seed)
    n = 200
    o2d, parents, max_doc = N.families(n, seed, sizes=(1, 2, 3, 5, 17))
    mask = N.parent_mask(parents, max_doc)
    if seed % 2:                                 # some parents carry a vector themselves: a family of one more
        o2d = np.sort(np.concatenate([o2d[: n - 10], parents[:10]])).astype(np.int32)
    scores = rng.integers(0, 12, n).astype(np.float32) / 8            # many ties, inside and across families
    scores[rng.random(n) < 0.1] = np.nan
    accept = None if seed < 2 else rng.random(max_doc) < 0.6
    for k in (1, 2, 10, 64, 500):
        wd, ws, visited = lucene_exact_search(o2d, scores, accept, mask, k)
        keep = np.ones(n, bool) if accept is None else accept[o2d]
        assert visited == int(keep.sum())
        shuffle = rng.permutation(int(keep.sum()))                   # the reference must not depend on row order
        gd, gs = N.nested_reference(o2d[keep][shuffle], scores[keep][shuffle], parents, k)
        assert np.array_equal(gd, wd) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (seed, k)


def test_set_parents_keeps_the_bitset_alive_while_the_library_reads_it(monkeypatch):
    """`_lib.ptr` is an address only: the packed parent words must have an owner for the length of the
    osk_seg_set_parents call.  (They were a temporary once, freed before the call: the allocator's free-list
    words then stood in for the parent bits of docs 0–127, and rows there were credited to other families, so
    tests/test_gpu_nested.py::test_view_batch_and_filter gave a wrong hit now and then.)"""
    import weakref
    from opensearch_amd import lucene as LU

    class Tracked(np.ndarray):
        pass

    state = {}
    real_bits = LU.bits_from_bool

    def tracked_bits(mask):
        a = real_bits(mask).view(Tracked)        # (the view owns a reference to the packed words)
        state["ref"] = weakref.ref(a)
        return a

    class FakeLib:
        def osk_seg_set_parents(self, handle, addr):
            owner = state["ref"]()
            assert owner is not None, "the parent words were freed before the library read them"
            assert addr == owner.ctypes.data
            state["seen"] = np.array(owner, np.uint64)
            return _lib.OSK_OK

    monkeypatch.setattr(LU, "bits_from_bool", tracked_bits)
    monkeypatch.setattr(LU, "lib", lambda: FakeLib())
    r = LU.GpuFlatVectorsReader("v", None, LU.VectorSimilarityFunction.EUCLIDEAN, max_doc=200, _handle=1, _dim=4, _n=150)
    try:
        mask = np.arange(200) % 5 == 4
        r.set_parents(mask)
        assert np.array_equal(state["seen"], real_bits(mask))
        assert np.array_equal(r.parent_mask, mask)
    finally:
        r._h = C.c_void_p(None)                   # (no segment behind the handle: nothing to release)
