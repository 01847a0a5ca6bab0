"""The bf16×3 batched path (opensearch_amd/csrc/osk_mfma.hip) restated in plain numpy: the bf16 hi/lo split,
the fragment order of `split_rows`, the three-product dot, the approximate score transforms and the
certificate's bound U of `rescore`.  float64 unless stated; tests/test_mfma_reference_cpu.py holds it to what
the source's comments claim and tests/test_gpu_mfma_cert.py holds the device to it.
"""
import numpy as np

EUCLIDEAN, DOT_PRODUCT, COSINE, MIP = 0, 1, 2, 3
KC = 16            # osk_internal.h kKC: candidates per (query, shard)
KS_ALIGN = 4       # osk_internal.h kKsAlign


def _bf16_rne_bits(v32: np.ndarray) -> np.ndarray:
    u = v32.view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF) >> 16).astype(np.uint16)


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def split(v):
    """(hi, lo) uint16: hi = bf16 round-to-nearest-even of the float32 bits, lo = RNE(v − hi), the subtraction
    in float32 — exactly what bf16_rne_bits stores."""
    v = np.ascontiguousarray(v, np.float32)
    hi = _bf16_rne_bits(v)
    with np.errstate(all="ignore"):
        r = (v - bf16_to_f32(hi)).astype(np.float32)
    return hi, _bf16_rne_bits(np.ascontiguousarray(r))


def ks_of(dim: int) -> int:
    """K-steps of 32 dims per padded row: ⌈⌈units/8⌉/4⌉·4, units = ⌈dim/4⌉ float4s."""
    units = (dim + 3) // 4
    return ((units + 7) // 8 + KS_ALIGN - 1) // KS_ALIGN * KS_ALIGN


def fragments(hi_lo, KS: int, n_rb: int | None = None) -> np.ndarray:
    """The 1 KiB block order of split_rows as uint16 [n_rb, KS, 2, 64, 8]: block (rb, ks, part), part 0 = hi,
    1 = lo; lane l holds row rb·16 + (l & 15), dims ks·32 + 8·(l >> 4) … +7.  Rows and dims beyond the input
    are zero."""
    hi, lo = hi_lo
    n, dim = hi.shape
    n_rb = (n + 15) // 16 if n_rb is None else n_rb
    assert n <= n_rb * 16 and dim <= KS * 32
    out = []
    for part in (hi, lo):
        P = np.zeros((n_rb * 16, KS * 32), np.uint16)
        P[:n, :dim] = part
        # [rb, row 16, ks, group 4, j 8] → [rb, ks, group, row, j]: lane = group·16 + row
        out.append(P.reshape(n_rb, 16, KS, 4, 8).transpose(0, 2, 3, 1, 4).reshape(n_rb, KS, 64, 8))
    return np.ascontiguousarray(np.stack(out, axis=2))


def approx_dot(x, q) -> np.ndarray:
    """hi·hi + hi·lo + lo·hi of every (query, row), exact products summed in float64: [nq, n]."""
    xh, xl = (bf16_to_f32(p).astype(np.float64) for p in split(x))
    qh, ql = (bf16_to_f32(p).astype(np.float64) for p in split(q))
    with np.errstate(all="ignore"):
        return qh @ xh.T + ql @ xh.T + qh @ xl.T


def approx_score(sim: int, d, qn, xn) -> np.ndarray:
    """osk_mfma.hip approx_score in float32, operation by operation (rsqrtf as 1/√, correctly rounded)."""
    d, qn, xn = (np.asarray(a, np.float32) for a in (d, qn, xn))
    one, two, half, inf = np.float32(1.0), np.float32(2.0), np.float32(0.5), np.float32(np.inf)
    nan_to_inf = lambda s: np.where(np.isnan(s), inf, s).astype(np.float32)
    with np.errstate(all="ignore"):
        if sim == EUCLIDEAN:
            d2 = xn + qn - two * d
            d2 = np.where(d2 > 0, d2, np.float32(0.0)).astype(np.float32)        # fmaxf(·, 0): NaN → 0
            return one / (one + d2)
        if sim == DOT_PRODUCT:
            return np.maximum(nan_to_inf((one + d) * half), np.float32(0.0))
        if sim == COSINE:
            rq, rx = one / np.sqrt(qn), one / np.sqrt(xn)
            s = nan_to_inf((one + d * rq * rx) * half)
            lim = np.float32(2.0 ** -64)
            return np.where((qn >= lim) & (xn >= lim), s, inf).astype(np.float32)
        return nan_to_inf(np.where(d < 0, one / (one - d), d + one).astype(np.float32))


def c(KS: int) -> float:
    """osk_derived.hip ensure_mfma: 1.5·(3·2^-16 + 4·Kpad·2^-24), Kpad = 32·KS."""
    return 1.5 * (3.0 * 2.0 ** -16 + 4.0 * (32.0 * KS) * 2.0 ** -24)


def U(sim: int, sa, c_: float, xmax, qabs) -> np.ndarray:
    """The certificate's bound exactly as `rescore` writes it, in double: no row whose approximate score is
    ≤ sa may have an exact score above U.  xmax = √(max |x|² of the shard), qabs = √|q|²."""
    sa, xmax, qabs = (np.asarray(a, np.float64) for a in (sa, xmax, qabs))
    with np.errstate(all="ignore"):
        e_dot = c_ * xmax * qabs
        if sim == DOT_PRODUCT:
            u = sa + 0.5 * e_dot
        elif sim == COSINE:
            u = sa + 0.5 * c_ + np.zeros_like(e_dot)
        elif sim == MIP:
            u = sa + e_dot
        else:
            e_d2 = 2.0 * e_dot + 1e-6 * (xmax * xmax + qabs * qabs)
            inv = 1.0 / sa - e_d2
            u = np.where(inv <= 1.0, 1.0, 1.0 / inv)
        return u + (1e-6 * np.abs(u) + 1e-12)


# ---------------------------------------------------------------------------------------------------------
# |v|² in the device's lane order (oracle/lucene_oracle.c device_sum of (v, v)), float32 bit for bit
# ---------------------------------------------------------------------------------------------------------
def lane_cfg(units: int):
    for lim, L, V in zip([8, 16, 32, 64, 128, 192, 256, 512, 1 << 30], [4, 8, 8, 16, 16, 16, 32, 64, 64],
                         [2, 2, 4, 4, 8, 12, 8, 8, 16]):
        if units <= lim:
            return L, V


def fma_sq32(x: np.ndarray, acc: np.ndarray) -> np.ndarray:
    """fmaf(x, x, acc) of float32 arrays, one rounding: the square is exact in double, the sum is rounded to
    odd at 53 bits (two-sum), which then rounds to float32 as the exact sum would."""
    p = x.astype(np.float64) * x.astype(np.float64)
    a = acc.astype(np.float64)
    with np.errstate(all="ignore"):
        s = p + a
        bb = s - p
        err = (p - (s - bb)) + (a - bb)
    fix = np.isfinite(s) & (err != 0)
    toward_zero = fix & ((err > 0) != (s > 0))           # the exact sum lies nearer zero than s: truncate
    s = np.where(toward_zero, np.nextafter(s, 0.0), s)
    bits = s.view(np.int64) if s.flags["C_CONTIGUOUS"] else np.ascontiguousarray(s).view(np.int64)
    bits = np.where(fix, bits | 1, bits)
    with np.errstate(all="ignore"):
        return bits.view(np.float64).astype(np.float32)


def device_norm2(vecs) -> np.ndarray:
    """|v|² of each row as the device sums it: lane t keeps 4 fma chains over units t, t + L, …; (x + y) +
    (z + w) per lane; an xor-butterfly over the L lanes.  float32 [n]."""
    vecs = np.asarray(vecs, np.float32)
    n, dim = vecs.shape
    L, V = lane_cfg((dim + 3) // 4)
    W = 4 * L
    P = np.zeros((n, V * W), np.float32)
    P[:, :dim] = vecs
    acc = np.zeros((n, W), np.float32)
    for j in range(V):
        acc = fma_sq32(P[:, j * W:(j + 1) * W], acc)
    with np.errstate(all="ignore"):
        a = acc.reshape(n, L, 4)
        p = (a[:, :, 0] + a[:, :, 1]) + (a[:, :, 2] + a[:, :, 3])
        m = 1
        while m < L:
            p = p + p[:, np.arange(L) ^ m]
            m <<= 1
    return np.ascontiguousarray(p[:, 0], np.float32)
