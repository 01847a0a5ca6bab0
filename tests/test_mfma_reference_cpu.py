"""oracle/mfma_reference.py held to what osk_mfma.hip's comments claim (no GPU), and the inputs of
test_gpu_mfma_cert.py held to what that file needs of them: on the reference's own approximate scores the
error model holds and at most 1 % of a case's certificates are too close to call."""
import numpy as np
import pytest

import bounds_inputs as BI
import mfma_inputs as MI
from oracle import mfma_reference as MR
from oracle import oracle as O

SIMS = [0, 1, 2, 3]


def normal_values(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 2.0 ** rng.integers(-100, 100, n)).astype(np.float32)


def test_split_leaves_at_most_2_pow_minus_17():
    """|v − hi − lo| ≤ 2^-17·|v| for normal values (hi and lo are each within 2^-9 relative of what they
    round), also at the mantissas built to maximise lo and its residue."""
    v = np.concatenate([normal_values(1, 200000), MI.lolo_vectors(4096, 2, 8).ravel()])
    hi, lo = MR.split(v)
    h, l = MR.bf16_to_f32(hi).astype(np.float64), MR.bf16_to_f32(lo).astype(np.float64)
    assert np.all(np.abs(v.astype(np.float64) - h - l) <= 2.0 ** -17 * np.abs(v.astype(np.float64)))
    # the built mantissas: |lo| within 1 % of its largest value 2^-9·2^e, residue above 0.49 ulp of lo
    w = MI.lolo_vectors(64, 3, 4).ravel()
    hi, lo = MR.split(w)
    h, l = MR.bf16_to_f32(hi).astype(np.float64), MR.bf16_to_f32(lo).astype(np.float64)
    e = np.floor(np.log2(w.astype(np.float64)))
    assert np.all(h <= w) and np.all(l >= 0.99 * 2.0 ** (e - 8)) and np.all(w - h - l >= 0.49 * 2.0 ** (e - 16 - 7))


def test_split_is_bf16_rne_of_the_bits():
    v = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 0.0, -0.0, 3.0e38, 1e-40], np.float32)
    hi, _ = MR.split(v)
    # 1 + 2^-8 is a tie: to even (1.0); 1 + 3·2^-8 is a tie: to even (1 + 2^-6)
    assert list(hi[:4]) == [0x3F80, 0x3F80, 0x3F82, 0xBF80]
    assert hi[4] == 0 and hi[5] == 0x8000


@pytest.mark.parametrize("dim", [3, 100, 768, 4096])
def test_approx_dot_within_3_2_pow_minus_16(dim):
    """|hi·hi + hi·lo + lo·hi − x·q| ≤ 3·2^-16·|x||q| (the source's "≈ 2^-16 relative" with its factor 3)."""
    rng = np.random.default_rng(dim)
    x = np.concatenate([rng.standard_normal((40, dim)).astype(np.float32), MI.special_rows(dim, 5)])
    q = np.concatenate([rng.standard_normal((10, dim)).astype(np.float32), MI.special_queries(dim, 1, 5, 1.0)])
    real = q.astype(np.float64) @ x.astype(np.float64).T
    lim = 3.0 * 2.0 ** -16 * np.linalg.norm(q.astype(np.float64), axis=1)[:, None] * np.linalg.norm(x.astype(np.float64), axis=1)[None, :]
    assert np.all(np.abs(MR.approx_dot(x, q) - real) <= lim)


@pytest.mark.parametrize("sim", SIMS)
def test_u_is_monotone_in_sa(sim):
    sa = np.sort(np.concatenate([np.linspace(1e-9, 1.0, 4001), 2.0 ** np.arange(-60.0, 40.0)]))
    sa = sa[sa <= 1.0] if sim == 0 else sa            # (EUCLIDEAN scores are 1/(1 + d²))
    for xmax, qabs in [(1.0, 1.0), (1e-6, 3.0), (2.0 ** 30, 2.0 ** 30), (0.0, 1.0)]:
        u = MR.U(sim, sa, MR.c(24), xmax, qabs)
        assert np.all(np.diff(u) >= 0) and np.all(u >= sa)


def test_c_of_ks():
    assert MR.ks_of(3) == 4 and MR.ks_of(128) == 4 and MR.ks_of(129) == 8 and MR.ks_of(768) == 24
    assert MR.ks_of(1000) == 32 and MR.ks_of(4096) == 128 and MR.ks_of(100) == 4 and MR.ks_of(17) == 4
    assert MR.c(4) == 1.5 * (3 * 2.0 ** -16 + 4 * 128 * 2.0 ** -24)


def test_fragment_layout_is_a_bijection_onto_the_padded_matrix():
    n, dim = 37, 70
    KS = MR.ks_of(dim)
    ids = np.arange(n * dim, dtype=np.uint16).reshape(n, dim) + 1
    F = MR.fragments((ids, ids + 10000), KS)
    assert F.shape == (3, KS, 2, 64, 8) and F.nbytes == 3 * KS * 2 * 1024
    for part, off in ((0, 0), (1, 10000)):
        got = F[:, :, part]
        vals = np.sort(got[got != 0])
        assert np.array_equal(vals, np.arange(n * dim) + 1 + off)             # every element once
        assert (got == 0).sum() == 3 * 16 * KS * 32 - n * dim                  # and zeros everywhere else
        for rb, ks, lane, j in [(0, 0, 0, 0), (2, 1, 20, 3), (1, 2, 63, 7), (2, 0, 5, 1)]:
            row, d = rb * 16 + (lane & 15), ks * 32 + 8 * (lane >> 4) + j
            want = ids[row, d] + off if row < n and d < dim else 0
            assert got[rb, ks, lane, j] == want


@pytest.mark.parametrize("dim", MI.DIMS)
def test_device_norm2_is_the_oracles(dim):
    """Bit for bit: a power-of-two scaling commutes with every rounding of the sum (no overflow or subnormal on
    the way), and once |v|² ≥ 2^25 the MAXIMUM_INNER_PRODUCT score fl(|v|² + 1) of (v, v) in ORDER_DEVICE is the
    oracle's device-order sum itself (1 is below half an ulp)."""
    v = np.concatenate([O.synth(0, 6, dim, 3, 1), MI.special_rows(dim, 9, tame=True)[::3], MI.pow_vectors(dim, 4, 2, -32)])
    v = v[np.abs(v).max(axis=1) > 0]
    n2 = MR.device_norm2(v).astype(np.float64)
    k = np.ceil((30.0 - np.log2(n2)) / 2.0)
    scaled = (v.astype(np.float64) * 2.0 ** k[:, None]).astype(np.float32)
    assert np.array_equal(scaled.astype(np.float64), v.astype(np.float64) * 2.0 ** k[:, None])
    got = MR.device_norm2(scaled)
    assert (got >= 2.0 ** 25).all() and (got <= 2.0 ** 40).all()
    for i in range(len(v)):
        want = np.float32(O.score(scaled[i], scaled[i], 3, O.ORDER_DEVICE))
        assert got[i].view(np.uint32) == want.view(np.uint32), (i, got[i], want)
    assert np.array_equal(got.astype(np.float64), n2 * 4.0 ** k)


@pytest.mark.parametrize("dim", MI.DIMS)
@pytest.mark.parametrize("sim", SIMS)
def test_inputs_fit_the_gpu_checks(sim, dim):
    """With the reference's approximate scores in place of the device's: the oracle's score never exceeds
    U(approximate score) on the visible view, and the certificates of at most 1 % of a view's (query, shard)
    pairs lie within 2e-6·|U| of their bound."""
    v = MI.visible_view(sim, dim)
    c = MR.c(MR.ks_of(dim))
    sc, vr, cnt = v.reference_keys(False)
    assert np.array_equal(cnt, np.broadcast_to(np.bincount(v.shard_of_row), cnt.shape))
    u = v.bound(sc, c)
    e = np.where(vr >= 0, v.scores[np.arange(len(v.queries))[:, None, None], np.maximum(vr, 0)], np.nan)
    bad = (vr >= 0) & ~np.isnan(e) & ~(e <= u)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[0])
    for view in (v, MI.tiled_view(sim, dim)):
        for filtered in (False, True):
            _, und, _ = view.restated_flags(*view.reference_keys(filtered), c)
            assert und.mean() <= 0.01, (filtered, float(und.mean()))
    p = MI.pilot_view(sim, dim)                      # its 16 best rows, in order, under every query
    order = np.argsort(-p.scores.astype(np.float64), axis=1, kind="stable")[:, :MI.KC]
    assert np.array_equal(order, np.broadcast_to(np.concatenate([np.arange(15), [MI.PILOT_LATE]]), order.shape))
    assert (np.sort(p.scores[:, 128:], axis=1)[:, -2] < np.sort(p.scores[:, :128], axis=1)[:, 0]).all()
    t = MI.tiled_view(sim, dim)
    assert BI.in_range(t.rows).all() and len(t.queries) == MI.N_QUERIES_TILED and len(v.queries) == MI.N_QUERIES_VISIBLE
