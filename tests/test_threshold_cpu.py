"""The similarity-threshold entries of the C-ABI on a machine without a GPU: exported, bound by the ctypes table
and by OsKnn.java, argument errors refused before the device is touched (OSK_ERR_INVALID with a message), and a
valid call without a device fails loudly with OSK_ERR_NO_DEVICE ([L] AbstractVectorSimilarityQuery's entries:
include/osknn.h)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from opensearch_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
OSKNN_JAVA = ROOT / "java" / "plugin" / "src" / "main" / "java" / "org" / "opensearch" / "knn" / "gpu" / "OsKnn.java"
NAMES = ["osk_seg_search_threshold", "osk_view_search_threshold", "osk_view_search_threshold_device"]


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
    # widths: (seg|view, queries, n_queries, min_scores, accept, cap, docs, scores, count, total[, visited[, stream]])
    assert len(_lib.SIGNATURES["osk_seg_search_threshold"][1]) == 11
    assert len(_lib.SIGNATURES["osk_view_search_threshold"][1]) == 10
    assert len(_lib.SIGNATURES["osk_view_search_threshold_device"][1]) == 12
    for name in NAMES:
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32 and args[2] is C.c_int32 and args[5] is C.c_int32


def _bufs(nq=1, cap=4):
    return dict(h=(C.c_uint8 * 4096)(), q=np.zeros((nq, 8), np.float32), ms=np.full(nq, 0.5, np.float32),
                docs=np.full(nq * cap, -7, np.int32), scores=np.full(nq * cap, -7, np.float32),
                count=np.full(nq, -7, np.int32), total=np.full(nq, -7, np.int64), visited=np.full(nq, -7, np.int64))


def _seg_call(b, **over):
    a = dict(seg=C.addressof(b["h"]), q=b["q"].ctypes.data, nq=1, ms=b["ms"].ctypes.data, acc=None, cap=4,
             docs=b["docs"].ctypes.data, scores=b["scores"].ctypes.data, count=b["count"].ctypes.data,
             total=b["total"].ctypes.data, visited=b["visited"].ctypes.data)
    a.update(over)
    return _lib.lib().osk_seg_search_threshold(a["seg"], a["q"], a["nq"], a["ms"], a["acc"], a["cap"], a["docs"],
                                               a["scores"], a["count"], a["total"], a["visited"])


def _view_call(b, device=False, **over):
    a = dict(view=C.addressof(b["h"]), q=b["q"].ctypes.data, nq=1, ms=b["ms"].ctypes.data, acc=None, cap=4,
             docs=b["docs"].ctypes.data, scores=b["scores"].ctypes.data, count=b["count"].ctypes.data,
             total=b["total"].ctypes.data)
    a.update(over)
    if device:
        return _lib.lib().osk_view_search_threshold_device(a["view"], a["q"], a["nq"], a["ms"], a["acc"], a["cap"],
                                                           a["docs"], a["scores"], a["count"], a["total"], None, None)
    return _lib.lib().osk_view_search_threshold(a["view"], a["q"], a["nq"], a["ms"], a["acc"], a["cap"], a["docs"],
                                                a["scores"], a["count"], a["total"])


BAD = [dict(q=None), dict(ms=None), dict(docs=None), dict(scores=None), dict(count=None), dict(total=None),
       dict(nq=0), dict(nq=-3), dict(cap=0), dict(cap=-1)]


@pytest.mark.parametrize("bad", BAD + [dict(seg=None)], ids=lambda d: next(iter(d)) + "=" + str(next(iter(d.values()))))
def test_seg_entry_rejects_bad_arguments_before_the_device(bad):
    b = _bufs()
    assert _seg_call(b, **bad) == _lib.OSK_ERR_INVALID
    assert _err() != ""
    assert np.all(b["docs"] == -7) and np.all(b["total"] == -7)   # nothing written


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("bad", BAD + [dict(view=None)], ids=lambda d: next(iter(d)) + "=" + str(next(iter(d.values()))))
def test_view_entries_reject_bad_arguments_before_the_device(bad, device):
    b = _bufs()
    assert _view_call(b, device, **bad) == _lib.OSK_ERR_INVALID
    assert _err() != ""
    assert np.all(b["docs"] == -7) and np.all(b["total"] == -7)


def test_error_messages_name_the_argument():
    b = _bufs()
    assert _seg_call(b, cap=0) == _lib.OSK_ERR_INVALID and "cap" in _err()
    assert _seg_call(b, nq=0) == _lib.OSK_ERR_INVALID and "n_queries" in _err()
    assert _view_call(b, q=None) == _lib.OSK_ERR_INVALID and "null" in _err()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_valid_calls_fail_loudly_without_a_device():
    b = _bufs()
    assert _seg_call(b) == _lib.OSK_ERR_NO_DEVICE and "no HIP device" in _err()
    assert _view_call(b) == _lib.OSK_ERR_NO_DEVICE and "no HIP device" in _err()
    assert _view_call(b, device=True) == _lib.OSK_ERR_NO_DEVICE and "no HIP device" in _err()
    assert np.all(b["docs"] == -7) and np.all(b["count"] == -7)
