"""Float64 numpy restatement of the int8 prefilter's certificate.

TEST INFRASTRUCTURE ONLY, like oracle.py.  Written from the design's inequality, not from the kernels:

    x = s_x·(q_x + δ_x),  b = s_b·(q_b + δ_b),  I = Σ q_x·q_b  (an exact integer)
    |x·b − s_x·s_b·I| ≤ s_x|q_x|·|δ_b| + |δ_x|·(s_b|q_b| + |δ_b|)                       (Cauchy–Schwarz)
    |dot_fp32 − x·b|  ≤ gam·(|x|² + |b|²),  gam = (n + 8)·2^-24                          (any summation tree)
    |d²_fp32 − d²|    ≤ g2·d²,              g2  = (n + 8)·2^-23,  n = the dim padded to 4

Here |δ| stands for the real norm |x − s·q| (the design's s·|δ|).  The quantisation itself is the device's
definition (s = max|x|/127 as a float32 division, codes = clamp(rint(x/s), ±127) in float32); every norm is
the real one in float64, with none of the round-ups or slacks the kernels add.  So a device record [LB, UB]
must contain the score image of `real_interval` (a dropped or down-rounded bound term breaks that on every
row), must contain every fp32 score, and may exceed the score image of `full_interval` only by the slack the
kernels declare.
"""
from __future__ import annotations

import numpy as np

EUCLIDEAN, DOT_PRODUCT, COSINE, MAXIMUM_INNER_PRODUCT = 0, 1, 2, 3


def padded_dim(dim: int) -> int:
    return (dim + 3) // 4 * 4


def gam(dim: int) -> float:
    return (padded_dim(dim) + 8) * 2.0 ** -24


def g2(dim: int) -> float:
    return (padded_dim(dim) + 8) * 2.0 ** -23


class Quantised:
    """The quantised form of float32 vectors [n, dim]: scale s = max|x|/levels (float32 value, held in
    float64), integer codes q ∈ [-levels, levels] (float64), and the real norms A = s·|q|, B = |x − s·q|,
    x2 = |x|².  levels 127: the int8 copy and query; the 6-bit tier (osk_sq6.hip) keeps its rows at 31 and
    quantises its query at 119.  The Cauchy–Schwarz bound of `real_interval` holds for any quantiser, so
    the intervals below are the 6-bit tier's as they stand."""

    def __init__(self, x: np.ndarray, levels: int = 127):
        x = np.ascontiguousarray(x, np.float32)
        assert x.ndim == 2
        with np.errstate(all="ignore"):
            m = np.abs(x).max(axis=1) if x.shape[1] else np.zeros(len(x), np.float32)
            s = (m / np.float32(levels)).astype(np.float32)           # one float32 division
            pos = s > 0
            ratio = np.zeros_like(x)
            np.divide(x, s[:, None], out=ratio, where=pos[:, None])   # float32 division
            q = np.clip(np.rint(ratio), np.float32(-levels), np.float32(levels))
        q = np.where(pos[:, None], q, np.float32(0.0)).astype(np.float64)
        x64 = x.astype(np.float64)
        s64 = s.astype(np.float64)
        self.s = s64
        self.q = q
        self.A = s64 * np.sqrt((q * q).sum(axis=1))
        d = x64 - s64[:, None] * q
        self.B = np.sqrt((d * d).sum(axis=1))
        self.x2 = (x64 * x64).sum(axis=1)
        self.x = x64


def real_interval(sim: int, rows: Quantised, qry: Quantised):
    """[lo, hi] ∋ the real x·b (or the real d² for EUCLIDEAN), shape [n_queries, n_rows]: the int8 centre
    ± the Cauchy–Schwarz radius.  Also returns (c, r) of the dot for the tightness slack."""
    I = qry.q @ rows.q.T                                              # exact: |I| ≤ 4096·127² < 2^53
    c = (qry.s[:, None] * rows.s[None, :]) * I
    r = rows.A[None, :] * qry.B[:, None] + rows.B[None, :] * (qry.A[:, None] + qry.B[:, None])
    if sim == EUCLIDEAN:
        base = rows.x2[None, :] + qry.x2[:, None]
        return np.maximum(base - 2.0 * (c + r), 0.0), base - 2.0 * (c - r), c, r
    return c - r, c + r, c, r


FLT_MAX = float(np.finfo(np.float32).max)


def eta(dim: int) -> float:
    """fp32 underflow: an operation whose result is subnormal errs by ≤ 2^-150 absolutely instead of 2^-24
    relatively (fl(a∘b) = (a∘b)(1 + δ) + η), and a sum of n products has at most n such results that are not
    exact (sums of subnormals are).  2× margin, as gam has.  Invisible (≪ 2^-24·1) in every score but
    COSINE's, whose quotient sees it when |x|²·|b|² is itself near the subnormal range."""
    return padded_dim(dim) * 2.0 ** -149


def full_interval(sim: int, rows: Quantised, qry: Quantised, dim: int):
    """The real interval widened by the fp32 rounding of any summation tree: [lo, hi] ∋ every fp32 dot
    (d²) of the pair.  No slack for the bound's own float arithmetic.

    The design's gam / g2 model assumes the fp32 range.  Outside it the interval says what fp32 can still
    return: `eta` where results underflow; and where a partial sum can pass FLT_MAX (dot: Σ|x_i·b_i| ≤
    |x||b|; d²: the sum itself) the open end(s), since fp32 then returns ±inf (or NaN from inf − inf)."""
    lo, hi, c, r = real_interval(sim, rows, qry)
    with np.errstate(all="ignore"):
        if sim == EUCLIDEAN:
            lo, hi = np.maximum(lo * (1.0 - g2(dim)) - eta(dim), 0.0), hi * (1.0 + g2(dim)) + eta(dim)
            hi = np.where(hi >= FLT_MAX, np.inf, hi)
            return lo, hi, c, r
        w = gam(dim) * (rows.x2[None, :] + qry.x2[:, None]) + eta(dim)
        lo, hi = lo - w, hi + w
        over = np.sqrt(rows.x2[None, :] * qry.x2[:, None]) * (1.0 + gam(dim)) >= FLT_MAX
        return np.where(over, -np.inf, lo), np.where(over, np.inf, hi), c, r


def norm_interval(x2, dim: int):
    """[lo, hi] ∋ |x|² as fp32 sums it in any order, outside the fp32 range only (inside it the norms' rounding
    is part of what gam's 2× margin covers): ± eta, and +inf once the sum can pass FLT_MAX."""
    x2 = np.asarray(x2, np.float64)
    hi = x2 + eta(dim)
    return np.maximum(x2 - eta(dim), 0.0), np.where(x2 * (1.0 + gam(dim)) >= FLT_MAX, np.inf, hi)


def score64(sim: int, raw, qn=None, xn=None):
    """Lucene's four float score transforms of the raw dot (d²) in float64.  COSINE takes |q|², |x|²."""
    raw = np.asarray(raw, np.float64)
    with np.errstate(all="ignore"):
        if sim == EUCLIDEAN:
            return 1.0 / (1.0 + raw)
        if sim == DOT_PRODUCT:
            return np.maximum((1.0 + raw) / 2.0, 0.0)
        if sim == COSINE:
            v = (1.0 + raw / np.sqrt(np.asarray(qn, np.float64) * np.asarray(xn, np.float64))) / 2.0
            return np.where(v >= 0.0, v, np.where(np.isnan(v), v, 0.0))   # Java's Math.max keeps NaN
        return np.where(raw < 0.0, 1.0 / (1.0 - raw), raw + 1.0)


def score_image(sim: int, lo, hi, qn=None, xn=None, dim=None):
    """(lb, ub) scores of a raw interval: the transforms are monotone, decreasing for EUCLIDEAN.  COSINE
    takes the real |q|², |x|²; with `dim` they range over `norm_interval` (the same wherever |x|² is inside
    the fp32 range), and a pair whose norm product may be 0 or inf/inf in fp32 has the image [0, inf]."""
    if sim == COSINE and dim is not None:
        (ql, qh), (xl, xh) = norm_interval(qn, dim), norm_interval(xn, dim)
        with np.errstate(all="ignore"):
            dl, dh = np.sqrt(ql * xl), np.sqrt(qh * xh)
            lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
            cl = np.minimum(lo / dl, lo / dh)
            ch = np.maximum(hi / dl, hi / dh)
            open_ = ~(dl > 0) | np.isnan(cl) | np.isnan(ch)
            a = np.where(open_, 0.0, np.maximum((1.0 + cl) / 2.0, 0.0))
            b = np.where(open_, np.inf, np.maximum((1.0 + ch) / 2.0, 0.0))
            # a zero vector scores NaN in every order (0/0): no image
            zero = (np.asarray(qn, np.float64) == 0) | (np.asarray(xn, np.float64) == 0)
            return np.where(zero, np.nan, a), np.where(zero, np.nan, b)
    a, b = score64(sim, lo, qn, xn), score64(sim, hi, qn, xn)
    return (b, a) if sim == EUCLIDEAN else (a, b)


def floor_image(sim: int, lo, hi, qn=None, xn=None):
    """The score every order's score of the row is at least, as the 6-bit tier's floor uses it (osk_sq6.hip
    floor_lb_score): the score image of the interval's low side (its high side for EUCLIDEAN, whose transform
    decreases), in float64 with the real norms."""
    return score_image(sim, lo, hi, qn, xn)[0]


SQ6_ROW_LEVELS, SQ6_QUERY_LEVELS = 31, 119


def sq6_row_split(q):
    """A row code q ∈ [-31, 31] as osk_sq6.hip's header states it: q = 4h + l, h = q >> 2 ∈ [-8, 7], l = q & 3."""
    q = np.asarray(q, np.int64)
    return q >> 2, q & 3


def sq6_query_split(b):
    """A query code b ∈ [-119, 119]: b = 16·bh + bl, bl = ((b + 8) & 15) − 8 ∈ [-8, 7], |bh| ≤ 7."""
    b = np.asarray(b, np.int64)
    bl = ((b + 8) & 15) - 8
    return (b - bl) >> 4, bl


def sortable(scores) -> np.ndarray:
    """float32 → the u32 whose unsigned order is the float order (the device's hit-key form)."""
    u = np.ascontiguousarray(scores, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def from_sortable(bits) -> np.ndarray:
    u = np.ascontiguousarray(bits, np.uint32)
    b = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32)
    return b.view(np.float32)
