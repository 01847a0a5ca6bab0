"""The certificate's float64 reference (oracle/bounds_reference.py) against the oracle, before a GPU is
involved: DESIGN.md §3b claims that the int8 centre ± the Cauchy–Schwarz radius, widened by
gam·(|x|² + |b|²) (g2 relative for EUCLIDEAN), contains the fp32 dot product of "any summation tree".
Every oracle order's score, and the float64 score of the real dot product, must lie inside the score image
of that interval, to 2^-22 relative (Java's transforms round to float at most twice)."""
import numpy as np
import pytest

import bounds_inputs as BI
from oracle import bounds_reference as BR
from oracle import oracle as O

N_BASE = 96


def _check(name, val, lb, ub, q, what):
    """val inside [lb, ub] to BI.REL relative, or NaN (a NaN score is never a hit)."""
    ok = np.isnan(val) | ((val >= lb * (1.0 - BI.REL)) & (val <= ub * (1.0 + BI.REL)))
    if not ok.all():
        r = int(np.nonzero(~ok)[0][0])
        raise AssertionError(f"{name}: query {q} row {r} {what} {val[r]!r} outside [{lb[r]!r}, {ub[r]!r}]; "
                             f"{int((~ok).sum())} rows")


@pytest.mark.parametrize("dim", [1, 3, 17, 100, 768, 4096])
@pytest.mark.parametrize("sim", [0, 1, 2, 3], ids=["EUCLIDEAN", "DOT_PRODUCT", "COSINE", "MAXIMUM_INNER_PRODUCT"])
def test_every_order_inside_the_full_interval(sim, dim):
    rows = BI.make_rows(N_BASE, dim, sim, 900 + dim)
    queries = BI.make_queries(dim, sim, 900 + dim)
    R, Q = BR.Quantised(rows), BR.Quantised(queries)
    lo, hi, _, _ = BR.full_interval(sim, R, Q, dim)
    rlo, rhi, _, _ = BR.real_interval(sim, R, Q)
    with np.errstate(all="ignore"):
        real = Q.x @ R.x.T
        if sim == BR.EUCLIDEAN:
            real = R.x2[None, :] + Q.x2[:, None] - 2.0 * real
    for qi in range(len(queries)):
        lb, ub = BR.score_image(sim, lo[qi], hi[qi], Q.x2[qi], R.x2, dim)
        # the real dot product (float64: its own rounding is far inside the radius) lies in the real interval
        slack = 1e-12 * (np.abs(rlo[qi]) + np.abs(rhi[qi]))
        assert np.all((real[qi] >= rlo[qi] - slack) & (real[qi] <= rhi[qi] + slack)), (qi, "real dot")
        _check("float64", BR.score64(sim, real[qi], Q.x2[qi], R.x2), lb, ub, qi, "score of the real dot")
        for order in BI.ORDERS:
            sc, got = BI.oracle_scores(rows, queries[qi], sim, order)
            assert np.all(got | np.isnan(sc))
            _check(f"order {order}", sc.astype(np.float64), lb, ub, qi, "oracle score")


def test_quantisation_is_the_devices_definition():
    """s = max|x|/127 in float32, codes clamp(rint(x/s), ±127); ±max rows have δ = 0, midpoint rows |δ| = s/2·√(d−1)."""
    dim = 64
    e = BI.edge_rows(dim, 5)
    Q = BR.Quantised(e)
    assert Q.s[0] == 0 and not Q.q[0].any() and Q.A[0] == 0 and Q.B[0] == 0
    # (δ = 0 up to the float32 rounding of s = 1/127)
    assert np.array_equal(np.abs(Q.q[3]), np.full(dim, 127.0)) and Q.B[3] <= 2.0 ** -24 * np.sqrt(dim)
    assert Q.s[4] == 2.0 ** -7 and np.isclose(Q.B[4], 2.0 ** -8 * np.sqrt(dim - 1), rtol=1e-12)
    assert np.count_nonzero(Q.q[5]) == 1
    assert np.all(np.abs(Q.q) <= 127)
    s = np.float32(np.abs(e[6]).max()) / np.float32(127)
    assert Q.s[6] == np.float64(s)


def test_sortable_round_trip():
    v = np.array([0.0, 1.0, 0.5, np.inf, 1e-40, 3e38], np.float32)
    b = BR.sortable(v)
    assert np.all(np.diff(np.sort(b).astype(np.int64)) > 0) and np.array_equal(BR.from_sortable(b).view(np.uint32),
                                                                               v.view(np.uint32))
    assert np.array_equal(np.argsort(b), np.argsort(v))
