"""The knobs of the threshold search's certified int8 first pass on a machine without a GPU: `thr_sq8` is a
knob of both libraries, the testing knob `thr_sq8_all_maybe` (every candidate row re-scored exactly) exists only
in libosknn_testing.so, and both are documented in include/osknn.h with the two counters."""
import ctypes as C
from pathlib import Path

from opensearch_amd import _lib

ROOT = Path(__file__).resolve().parent.parent


def _tune(L, key, value):
    L.osk_tune_set.restype = C.c_int32
    L.osk_tune_set.argtypes = [C.c_char_p, C.c_int64]
    return L.osk_tune_set(key.encode(), value)


def test_thr_sq8_is_a_knob_of_both_libraries():
    for path in (_lib.LIB_PATH, _lib.TESTING_LIB_PATH):
        L = C.CDLL(str(path))
        try:
            assert _tune(L, "thr_sq8", 0) == _lib.OSK_OK
            assert _tune(L, "thr_sq8", 2) == _lib.OSK_ERR_INVALID          # 0 or 1
        finally:
            assert _tune(L, "thr_sq8", 1) == _lib.OSK_OK                  # the default


def test_all_maybe_exists_only_in_the_testing_build():
    L = C.CDLL(str(_lib.LIB_PATH))
    assert _tune(L, "thr_sq8_all_maybe", 1) == _lib.OSK_ERR_UNSUPPORTED
    L.osk_last_error.restype = C.c_char_p
    assert b"testing build" in L.osk_last_error()
    T = C.CDLL(str(_lib.TESTING_LIB_PATH))
    try:
        assert _tune(T, "thr_sq8_all_maybe", 1) == _lib.OSK_OK
    finally:
        assert _tune(T, "thr_sq8_all_maybe", 0) == _lib.OSK_OK


def test_the_header_documents_the_knobs_and_counters():
    header = (ROOT / "include" / "osknn.h").read_text()
    for name in ("thr_sq8", "thr_sq8_all_maybe", "threshold_sq8_calls", "threshold_sq8_settled_rows"):
        assert f'"{name}"' in header, name
