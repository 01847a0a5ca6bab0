"""The key of the 6-bit tier's share groups (osk_api.hip Sq6ShareKey), on the host alone: two views
share corpus passes only if their device, shard count, dim, similarity, ordered segment list, tile table and
dispatch order all compare equal.  The entries that split a call exist only in the testing build."""
import ctypes as C

import numpy as np

from opensearch_amd import _lib


def key_equal(a, b):
    T = C.CDLL(str(_lib.TESTING_LIB_PATH))
    out = C.c_int32(-1)
    args = []
    for hdr, segs, tiles, order in (a, b):
        hdr = np.asarray(hdr, np.int32)
        segs = np.asarray(segs, np.uint64)
        tiles = np.ascontiguousarray(tiles, np.int64)
        order = np.asarray(order, np.int32)
        assert tiles.shape == (len(order), 4)
        args += [hdr, segs, tiles, order]
    P = C.c_void_p
    T.osk_testing_sq6_share_key_equal.restype = C.c_int32
    T.osk_testing_sq6_share_key_equal.argtypes = [P, P, C.c_int32, P, P, C.c_int32] * 2 + [P]
    flat = []
    for hdr, segs, tiles, order in zip(*[iter(args)] * 4):
        flat += [hdr.ctypes.data, segs.ctypes.data, len(segs), tiles.ctypes.data, order.ctypes.data, len(order)]
    assert T.osk_testing_sq6_share_key_equal(*flat, C.byref(out)) == 0
    return out.value


BASE = ([0, 2, 768, 2], [0x1000, 0x2000],
        [[0, 0, 0, 512], [0, 0, 512, 1000], [1, 1, 0, 640], [1, 1, 640, 1301]], [0, 2, 1, 3])


def variant(hdr=None, segs=None, tiles=None, order=None):
    return (hdr or BASE[0], segs or BASE[1], tiles or BASE[2], order or BASE[3])


def test_equal_tables_share():
    assert key_equal(BASE, variant()) == 1
    assert key_equal(BASE, ([0, 2, 768, 2], list(BASE[1]), [list(t) for t in BASE[2]], list(BASE[3]))) == 1


def test_a_differing_table_order_or_segment_list_does_not_share():
    t = [list(x) for x in BASE[2]]
    t[1][3] = 1008                                   # a tile boundary
    assert key_equal(BASE, variant(tiles=t)) == 0
    assert key_equal(BASE, variant(tiles=BASE[2][:3], order=[0, 2, 1])) == 0      # fewer tiles
    t = [list(x) for x in BASE[2]]
    t[2][1] = 0                                      # a tile's shard
    assert key_equal(BASE, variant(tiles=t)) == 0
    assert key_equal(BASE, variant(order=[0, 1, 2, 3])) == 0                      # the dispatch order
    assert key_equal(BASE, variant(segs=[0x2000, 0x1000])) == 0                   # the segments' order
    assert key_equal(BASE, variant(segs=[0x1000, 0x3000])) == 0                   # another segment
    assert key_equal(BASE, variant(segs=[0x1000])) == 0
    for i, other in enumerate([1, 3, 512, 0]):       # device, shards, dim, similarity
        hdr = list(BASE[0])
        hdr[i] = other
        assert key_equal(BASE, variant(hdr=hdr)) == 0


def test_split_entries_and_limit_exist_only_in_the_testing_build():
    L, T = C.CDLL(str(_lib.LIB_PATH)), C.CDLL(str(_lib.TESTING_LIB_PATH))
    for lib in (L, T):
        lib.osk_tune_set.argtypes = [C.c_char_p, C.c_int64]
    for name in ("osk_testing_sq6_post", "osk_testing_sq6_resume", "osk_testing_sq6_share_key_equal"):
        assert hasattr(T, name) and not hasattr(L, name)
    assert L.osk_tune_set(b"sq6_share_limit", 1) == _lib.OSK_ERR_UNSUPPORTED
    assert T.osk_tune_set(b"sq6_share_limit", 1) == 0 and T.osk_tune_set(b"sq6_share_limit", -1) == 0
    for lib in (L, T):
        assert lib.osk_tune_set(b"sq6_share", 0) == 0 and lib.osk_tune_set(b"sq6_share", 1) == 0
        assert lib.osk_tune_set(b"sq6_share", 2) == _lib.OSK_ERR_INVALID
        assert lib.osk_tune_set(b"sq6_share_idle", 1) == 0 and lib.osk_tune_set(b"sq6_share_idle", 0) == 0
        assert lib.osk_tune_set(b"sq6_share_min_tiles", 5) == 0 and lib.osk_tune_set(b"sq6_share_min_tiles", 0) == 0
        assert lib.osk_tune_set(b"sq6_share_min_tiles", -1) == _lib.OSK_ERR_INVALID
