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


# ---- the 6-bit tier's reference (rows at 31 levels, the query at 119), on test_gpu_sq6_bounds.py's inputs ----

SIM_IDS = ["EUCLIDEAN", "DOT_PRODUCT", "COSINE", "MAXIMUM_INNER_PRODUCT"]


def test_quantised_levels():
    """`levels` is the device's definition for the 6-bit forms too: s = max|x|/levels as one float32 division,
    codes clamp(rint(x/s), ±levels); 127 stays the default."""
    e = BI.edge_rows(64, 5)
    for levels in (31, 119):
        Q = BR.Quantised(e, levels)
        assert np.all(np.abs(Q.q) <= levels) and np.abs(Q.q[6]).max() == levels
        assert Q.s[6] == np.float64(np.float32(np.abs(e[6]).max()) / np.float32(levels))
        assert np.array_equal(np.abs(Q.q[3]), np.full(64, float(levels)))
    assert np.array_equal(BR.Quantised(e).q, BR.Quantised(e, 127).q)


def test_nibble_identity():
    """osk_sq6.hip's header: a row code q = 4h + l (h = q >> 2 ∈ [-8, 7], l = q & 3), a query code b = 16·bh + bl
    (bl = ((b + 8) & 15) − 8 ∈ [-8, 7], |bh| ≤ 7), so q·b = 64·h·bh + 4·h·bl + 16·l·bh + l·bl for every pair."""
    q = np.arange(-31, 32)[:, None]
    b = np.arange(-119, 120)[None, :]
    (h, l), (bh, bl) = BR.sq6_row_split(q), BR.sq6_query_split(b)
    assert h.min() == -8 and h.max() == 7 and l.min() == 0 and l.max() == 3 and np.array_equal(4 * h + l, q)
    assert bl.min() == -8 and bl.max() == 7 and np.abs(bh).max() == 7 and np.array_equal(16 * bh + bl, b)
    assert np.array_equal(64 * h * bh + 4 * h * bl + 16 * l * bh + l * bl, q * b)


def test_sq6_dims_have_a_tier_and_cover_every_chunk_count():
    assert all(BI.sq6_supported(d) for d in BI.SQ6_DIMS) and not BI.sq6_supported(464)
    for c in range(2, 7):
        mine = [d for d in BI.SQ6_DIMS if (d + 255) // 256 == c]
        assert any(d % 4 for d in mine) and any(d % 16 == 0 for d in mine), c


@pytest.mark.parametrize("dim", BI.SQ6_DIMS)
@pytest.mark.parametrize("sim", [0, 1, 2, 3], ids=SIM_IDS)
def test_sq6_intervals_on_the_full_record_inputs(sim, dim):
    """The 6-bit real interval contains the float64 dot (d²), every oracle order's score lies inside the full
    interval's image, and for query 0 every planted row's lower bound tops its list (so the GPU test knows
    which row a floor bucket came from)."""
    c = BI.Sq6FullInputs(sim, dim)
    ref = BI.sq6_reference(sim, c.rows, c.queries, dim)
    slack = 1e-12 * (np.abs(ref["rlo"]) + np.abs(ref["rhi"]))
    assert np.all((ref["real"] >= ref["rlo"] - slack) & (ref["real"] <= ref["rhi"] + slack))
    S = [BI.oracle_scores_batch(c.rows, c.queries, sim, order) for order in BI.ORDERS]
    for qi in range(len(c.queries)):
        lb, ub = BR.score_image(sim, ref["flo"][qi], ref["fhi"][qi], ref["Q"].x2[qi], ref["R"].x2, dim)
        for order, sc in zip(BI.ORDERS, S):
            _check(f"order {order}", sc[qi].astype(np.float64), lb, ub, qi, "oracle score")
    margins = c.plant_margin(ref, BI.bucket_low_limit(sim, ref, dim, 0))
    assert len(margins) == sum(len(v) > 0 for _, v in c.lists) == 17
    for l, least, others in margins:
        assert least > others * (1.0 + BI.REL), (l, least, others)
    if sim != BR.EUCLIDEAN:      # the far shard: every dot negative, upper sides included
        far = np.concatenate([v for s, v in c.lists if s == 2])
        assert np.all(ref["rhi"][0][far] < 0)


@pytest.mark.parametrize("ragged", [False, True], ids=["flat", "ragged"])
@pytest.mark.parametrize("dim", BI.SQ6_FLOOR_DIMS)
@pytest.mark.parametrize("sim", [0, 1, 2, 3], ids=SIM_IDS)
def test_sq6_floored_views_can_show_a_tight_bound(sim, dim, ragged):
    """The floored views of test_gpu_sq6_bounds.py must not pass on nothing: already at the pilot's floor the
    reference drops ≥ 20 % of the rows (the device's floor lies between the pilot's and the final one), and at
    either floor ≥ 5 % of the rows have an upper image within 2 % of it, the band where an upper bound that is
    too tight would drop a row it must keep.  k = 1 is held to the band at the pilot's floor only: its final
    floor is the best row's own lower bound, which up to 100 % of these rows lie below, and in some views as
    few as 0–4 % are within 2 % of it, fewer still with more rows (the GPU test pools its band over the view's
    searches)."""
    c = BI.Sq6FlooredInputs(sim, dim, ragged)
    ref = BI.sq6_reference(sim, c.rows, c.queries, dim)
    for k in (1, 10, 12):
        for qi in range(len(c.queries)):
            pilot, final = c.reference_floors(ref, qi, k)
            assert np.all(pilot > 0) and np.all(final >= pilot)
            (dp, bp), (df, bf) = c.shares(ref, qi, pilot), c.shares(ref, qi, final)
            print(f"sim {sim} dim {dim} ragged {ragged} k {k} query {qi}: dropped {dp:.2f} .. {df:.2f}, "
                  f"within 2 % of the floor {bp:.2f} .. {bf:.2f}")
            assert dp >= 0.20 and df >= dp, (k, qi, dp, df)
            assert bp >= 0.05 and (bf >= 0.05 or k == 1), (k, qi, bp, bf)
