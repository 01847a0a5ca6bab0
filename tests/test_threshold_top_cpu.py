"""The top-k similarity-threshold entries of the C-ABI on a machine without a GPU: exported by both libraries, bound
by the ctypes table, by OsKnn.java and by the header with the same widths, argument errors refused before the
device is touched (OSK_ERR_INVALID with a message naming the argument, buffers untouched), and a valid call without
a device fails loudly with OSK_ERR_NO_DEVICE.  The ABI version stays 2: the entries are additions."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from opensearch_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
OSKNN_JAVA = ROOT / "java" / "plugin" / "src" / "main" / "java" / "org" / "opensearch" / "knn" / "gpu" / "OsKnn.java"
# name → (arguments, positions of the int32 arguments)
ENTRIES = {
    # (seg, queries, n_queries, min_scores, k, accept_bits, scores, docs, count, total, visited)
    "osk_seg_search_threshold_top": (11, (2, 4)),
    # (view, queries, n_queries, min_scores, k, from, size, accept, scores, docs, shard_index, count, total_hits, max)
    "osk_view_search_threshold_top": (14, (2, 4, 5, 6)),
    # (view, d_queries, n_queries, d_min_scores, k, d_accept, d_shard_keys, d_shard_counts, d_shard_totals, d_visited,
    #  stream)
    "osk_view_search_threshold_top_device": (11, (2, 4)),
}


def _err() -> str:
    return _lib.lib().osk_last_error().decode()


def _c_params(header: str, name: str) -> list[str]:
    m = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _java_layouts(java: str, name: str) -> list[str]:
    m = re.search(rf'h\(\s*"{name}"\s*,\s*FunctionDescriptor\.of\(([^)]*)\)', java, re.S)
    assert m, name
    return [t.strip() for t in m.group(1).split(",")]


def test_symbols_exported_and_bound_with_the_headers_widths():
    L = C.CDLL(str(_lib.LIB_PATH))
    T = C.CDLL(str(_lib.TESTING_LIB_PATH))
    java = re.sub(r"//[^\n]*", "", OSKNN_JAVA.read_text())
    header = (ROOT / "include" / "osknn.h").read_text()
    for name, (n_args, ints) in ENTRIES.items():
        assert hasattr(L, name) and hasattr(T, name), name
        res, args = _lib.SIGNATURES[name]
        params = _c_params(header, name)
        layouts = _java_layouts(java, name)
        assert res is C.c_int32 and layouts[0] == "JAVA_INT", name
        assert len(args) == len(params) == len(layouts) - 1 == n_args, name
        for i, (a, prm, lay) in enumerate(zip(args, params, layouts[1:])):
            is_int = i in ints
            assert (a is C.c_int32) == is_int and (a is C.c_void_p) == (not is_int), (name, i)
            assert prm.startswith("int32_t ") == is_int and ("*" in prm) == (not is_int), (name, prm)
            assert lay == ("JAVA_INT" if is_int else "ADDRESS"), (name, i, lay)
    # ...as additions: the ABI version stays 2
    assert L.osk_abi_version() == T.osk_abi_version() == 2 == _lib.OSK_ABI_VERSION
    assert re.search(r"#define\s+OSK_ABI_VERSION\s+2\b", header)


K, SIZE = 4, 3


def _bufs(nq=1):
    return dict(h=(C.c_uint8 * 4096)(), q=np.zeros((nq, 8), np.float32), ms=np.full(nq, 0.5, np.float32),
                scores=np.full(nq * K, -7, np.float32), docs=np.full(nq * K, -7, np.int32),
                shard=np.full(nq * K, -7, np.int32), count=np.full(nq, -7, np.int32),
                total=np.full(nq, -7, np.int64), visited=np.full(nq, -7, np.int64), mx=np.full(nq, -7, np.float32),
                keys=np.full(nq * K, 7, np.uint64))


def _untouched(b):
    return (np.all(b["scores"] == -7) and np.all(b["docs"] == -7) and np.all(b["shard"] == -7)
            and np.all(b["count"] == -7) and np.all(b["total"] == -7) and np.all(b["visited"] == -7)
            and np.all(b["mx"] == -7) and np.all(b["keys"] == 7))


def _seg_call(b, **over):
    a = dict(seg=C.addressof(b["h"]), q=b["q"].ctypes.data, nq=1, ms=b["ms"].ctypes.data, k=K, acc=None,
             scores=b["scores"].ctypes.data, docs=b["docs"].ctypes.data, count=b["count"].ctypes.data,
             total=b["total"].ctypes.data, visited=b["visited"].ctypes.data)
    a.update(over)
    return _lib.lib().osk_seg_search_threshold_top(a["seg"], a["q"], a["nq"], a["ms"], a["k"], a["acc"], a["scores"],
                                                   a["docs"], a["count"], a["total"], a["visited"])


def _view_call(b, **over):
    a = dict(view=C.addressof(b["h"]), q=b["q"].ctypes.data, nq=1, ms=b["ms"].ctypes.data, k=K, frm=0, size=SIZE,
             acc=None, scores=b["scores"].ctypes.data, docs=b["docs"].ctypes.data, shard=b["shard"].ctypes.data,
             count=b["count"].ctypes.data, total=b["total"].ctypes.data, mx=b["mx"].ctypes.data)
    a.update(over)
    return _lib.lib().osk_view_search_threshold_top(a["view"], a["q"], a["nq"], a["ms"], a["k"], a["frm"], a["size"],
                                                    a["acc"], a["scores"], a["docs"], a["shard"], a["count"],
                                                    a["total"], a["mx"])


def _device_call(b, **over):
    a = dict(view=C.addressof(b["h"]), q=b["q"].ctypes.data, nq=1, ms=b["ms"].ctypes.data, k=K, acc=None,
             keys=b["keys"].ctypes.data, count=b["count"].ctypes.data, total=b["total"].ctypes.data)
    a.update(over)
    return _lib.lib().osk_view_search_threshold_top_device(a["view"], a["q"], a["nq"], a["ms"], a["k"], a["acc"],
                                                           a["keys"], a["count"], a["total"], None, None)


# (the bad argument, a word its message carries)
COMMON = [(dict(q=None), "null"), (dict(ms=None), "null"), (dict(count=None), "null"), (dict(total=None), "null"),
          (dict(nq=0), "n_queries"), (dict(nq=-3), "n_queries"), (dict(k=0), "k must"), (dict(k=-1), "k must"),
          (dict(k=_lib.OSK_MAX_K + 1), "k must")]
SEG_BAD = COMMON + [(dict(seg=None), "null"), (dict(scores=None), "null"), (dict(docs=None), "null")]
VIEW_BAD = COMMON + [(dict(view=None), "null"), (dict(scores=None), "null"), (dict(docs=None), "null"),
                     (dict(shard=None), "null"), (dict(mx=None), "null"), (dict(frm=-1), "from"),
                     (dict(size=0), "size"), (dict(size=-2), "size")]
DEVICE_BAD = COMMON + [(dict(view=None), "null"), (dict(keys=None), "null")]


def _id(case):
    key, val = next(iter(case[0].items()))
    return f"{key}={val}"


@pytest.mark.parametrize("case", SEG_BAD, ids=_id)
def test_seg_entry_rejects_bad_arguments_before_the_device(case):
    b = _bufs()
    assert _seg_call(b, **case[0]) == _lib.OSK_ERR_INVALID
    assert case[1] in _err(), _err()
    assert _untouched(b)


@pytest.mark.parametrize("case", VIEW_BAD, ids=_id)
def test_view_entry_rejects_bad_arguments_before_the_device(case):
    b = _bufs()
    assert _view_call(b, **case[0]) == _lib.OSK_ERR_INVALID
    assert case[1] in _err(), _err()
    assert _untouched(b)


@pytest.mark.parametrize("case", DEVICE_BAD, ids=_id)
def test_device_entry_rejects_bad_arguments_before_the_device(case):
    b = _bufs()
    assert _device_call(b, **case[0]) == _lib.OSK_ERR_INVALID
    assert case[1] in _err(), _err()
    assert _untouched(b)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_valid_calls_fail_loudly_without_a_device():
    b = _bufs()
    assert _seg_call(b) == _lib.OSK_ERR_NO_DEVICE and "no HIP device" in _err()
    assert _view_call(b) == _lib.OSK_ERR_NO_DEVICE and "no HIP device" in _err()
    assert _device_call(b) == _lib.OSK_ERR_NO_DEVICE and "no HIP device" in _err()
    assert _device_call(b, k=_lib.OSK_MAX_K) == _lib.OSK_ERR_NO_DEVICE   # the largest k is a valid argument
    assert _untouched(b)
