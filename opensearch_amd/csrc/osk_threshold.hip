// osk_threshold.hip — exact similarity-threshold (radial) search: every accepted row whose score is
// ≥ min_score, in ascending doc order, with an exact count ([L] AbstractVectorSimilarityQuery /
// FloatVectorSimilarityQuery / ByteVectorSimilarityQuery over a flat field; OpenSearch's k-NN
// `min_score`).  DESIGN.md §3h.
//
//   thr_scan_f32 / thr_scan_i8   the only pass that reads the corpus: scan_f32 / scan_i8's tiles, lane
//                                layout, filter pushdown and score arithmetic, with the wave top-k list
//                                replaced by `hit = valid && score >= min_score` → one ballot per row
//                                group → 64-bit mask words + a per-(query, tile, wave) hit count.
//                                No score round-trips through HBM.
//   thr_scan_sq8 + thr_settle_f32  float32 views whose int8 prefilter copy certifies (tune thr_sq8): the same
//                                mask and counts from ¼ of the bytes — the int8 copy's certified score
//                                interval decides every row it can (sure hit / sure miss), the rows whose
//                                interval straddles min_score go to a second mask and are re-scored exactly.
//   thr_offsets                  per (query, shard): exclusive prefix sum of the wave counts in tile
//                                order (= segment by doc_base, then row, order) → each wave's output
//                                offset, the shard's exact total, min(total, cap), and the unused
//                                output slots' sentinels.
//   thr_emit_f32 / thr_emit_i8   per (query, tile, wave): walk the mask words and re-score each set bit's
//                                row with the same function (L lanes per row); doc + score go to
//                                offset + rank when that is < cap.  The hit decision is the mask's.
//   thr_top_f32 / thr_top_i8     the osk_*_search_threshold_top entries, in place of the emit: the same walk,
//                                each hit's key offered to the scans' wave list → the best k ≤ 64 per (query,
//                                tile) in scan_f32's cand layout → merge_shards.  thr_offsets writes the totals.
//   thr_keys_f32 / thr_keys_i8   ...for 64 < k ≤ OSK_MAX_K: each hit's key stored by view row, the select
//                                path's exact-key records → launch_select_one without its own writer.
//
// Mask word ownership: a wave's row range is a multiple of R = 64/L rows, not of 64, and under a filter
// on a dense field the walk visits compacted rows — so every wave owns `wpw` words of its own
// (bit = row − the wave's first row) and no two waves ever store the same word.  The mask is zeroed
// by the host before the scan; a wave stores only its non-zero words (plain vector stores).
#include <hip/hip_ext.h>

#include <algorithm>

#include "osk_device.h"
#include "osk_internal.h"
#include "osk_rowscore.h"
#include "osk_wave.h"

namespace osk {

namespace {

// (the per-row arithmetic — thr_load_row_*, thr_qnorm_*, thr_score_*, thr_wave_range — is in
// osk_rowscore.h, shared with the nested k-NN kernels)

// ------------------------------------------------------------------------------------------------
// The hit mask of a wave for NQ queries: the word in progress per query (wave-uniform), flushed when
// the walk moves to another word.  Every row group of one walk step lies inside ONE word: unfiltered
// steps are R | 64 consecutive rows starting at a multiple of R from the wave's first row; compacted
// steps (walk_rows under a filter on a dense field) take their rows from one 64-row window that starts
// at a multiple of 64 from it.
// ------------------------------------------------------------------------------------------------
template <int NQ>
struct ThrMask {
    uint64_t bits[NQ];
    uint32_t cnt[NQ];
    int idx;
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int b = 0; b < NQ; ++b) { bits[b] = 0ull; cnt[b] = 0u; }
        idx = 0;
    }
    // mw: this wave's words of query 0; query b's are at mw + b·qstride
    __device__ __forceinline__ void flush(uint64_t* mw, size_t qstride, int wpw, int q_count, int lane) {
#pragma unroll
        for (int b = 0; b < NQ; ++b) {
            if (bits[b] != 0ull && b < q_count && idx < wpw) {
                if (lane == 0) mw[b * qstride + idx] = bits[b];
                cnt[b] += (uint32_t)__popcll(bits[b]);
            }
            bits[b] = 0ull;
        }
    }
};

// One walk step's hits of query b → bits of the step's word.  `hit` is the same in all L lanes of a
// row group.  contiguous: group g is bit (rel0 & 63) + g; else each hit row sets its own bit.
template <int L>
__device__ __forceinline__ uint64_t thr_step_bits(bool hit, bool contiguous, int rel, int lane, int t) {
    constexpr int R = 64 / L;
    if (contiguous) {
        const int hg = __shfl((int)hit, (lane & (R - 1)) * L);
        const uint64_t m = __ballot(hg != 0 && lane < R);
        const int rel0 = __builtin_amdgcn_readfirstlane(rel);   // lane 0 = group 0 = the step's first row
        return m << (rel0 & 63);
    }
    uint64_t out = 0ull;
    uint64_t hm = __ballot(t == 0 && hit);
    while (hm) {
        const int src = __builtin_ctzll(hm);
        const int r = __builtin_amdgcn_readlane(rel, src);
        out |= 1ull << (r & 63);
        hm &= hm - 1ull;
    }
    return out;
}

// ------------------------------------------------------------------------------------------------
// scan, float32
// ------------------------------------------------------------------------------------------------
template <int L, int V, int NQ, bool L2K, bool NT>
__global__ __launch_bounds__(kBlock) void thr_scan_f32(ThrParams p) {
    constexpr int R = 64 / L;
    constexpr int UP = L * V;
    constexpr bool QREG = NQ * V * 4 <= 64;   // query fragments in VGPRs, else read from LDS (scan_f32's rule)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4* sq = reinterpret_cast<float4*>(smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = lane & (L - 1), g = lane / L;
    const TileDev tile = p.tiles[blockIdx.x];
    const SegDev seg = p.segs[tile.seg];
    const float4* __restrict__ X = static_cast<const float4*>(seg.rows);
    const float4* __restrict__ Q = static_cast<const float4*>(p.q);
    const int units = p.units;

    float4 qf[QREG ? NQ : 1][QREG ? V : 1];
    if constexpr (QREG) {
#pragma unroll
        for (int b = 0; b < NQ; ++b)
#pragma unroll
            for (int j = 0; j < V; ++j) qf[b][j] = Q[b * UP + t + j * L];
    } else {
        for (int i = tid; i < NQ * UP; i += kBlock) sq[i] = Q[i];
        __syncthreads();
    }
    auto qat = [&](int b, int j) -> float4 {
        if constexpr (QREG) return qf[b][j];
        else return sq[b * UP + t + j * L];
    };
    const int sim = p.sim;
    float qn[NQ], ms[NQ];
#pragma unroll
    for (int b = 0; b < NQ; ++b) {
        qn[b] = 0.0f;
        if (!L2K && sim == SIM_COSINE) qn[b] = thr_qnorm_f32<L, V>([&](int j) { return qat(b, j); });
        ms[b] = b < p.q_count ? p.min_score[b] : __builtin_nanf("");
    }

    int64_t wb, we;
    thr_wave_range<R>(tile, wave, wb, we);
    const uint64_t* abits = p.accept ? p.accept[tile.seg] : nullptr;
    const size_t qstride = (size_t)p.n_tiles * 4 * p.wpw;
    const size_t wi = (size_t)blockIdx.x * 4 + wave;
    uint64_t* mw = p.mask + wi * p.wpw;

    ThrMask<NQ> hm;
    hm.init();
    uint32_t nvis = 0;

    walk_rows<R>(wb, we, abits, seg.ord_to_doc, lane, g, [&](const int64_t row, bool valid, bool accepted_known) {
        int32_t doc = 0;
        if (valid) {
            doc = seg.ord_to_doc ? seg.ord_to_doc[row] : (int32_t)row;
            if (abits && !accepted_known) valid = (abits[doc >> 6] >> (doc & 63)) & 1ull;
        }
        float4 xv[V];
        thr_load_row_f32<L, V, NT>(X + row * units, valid, units, t, xv);
        float xn = 0.0f;
        if (!L2K && sim == SIM_COSINE && valid) xn = seg.xnorm_f[row];
        nvis += __popcll(__ballot(t == 0 && valid));

        const int rel = (int)(row - wb);
        const int widx = __builtin_amdgcn_readfirstlane(rel) >> 6;
        if (widx != hm.idx) {
            hm.flush(mw, qstride, p.wpw, p.q_count, lane);
            hm.idx = widx;
        }
#pragma unroll
        for (int b = 0; b < NQ; ++b) {
            const float sc = thr_score_f32<L, V, L2K>(xv, [&](int j) { return qat(b, j); }, sim, qn[b], xn);
            const bool hit = valid && sc >= ms[b];   // IEEE compare: NaN on either side is no hit, −0 == +0
            hm.bits[b] |= thr_step_bits<L>(hit, !accepted_known, rel, lane, t);
        }
    });
    hm.flush(mw, qstride, p.wpw, p.q_count, lane);

    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < NQ; ++b)
            if (b < p.q_count) p.counts[(size_t)b * p.n_tiles * 4 + wi] = (int32_t)hm.cnt[b];
    }
    if (p.visited && p.q0 == 0) add_visited_wg(&p.visited[tile.seg], nvis);
}

// ------------------------------------------------------------------------------------------------
// scan, int8 (exact int32 sums)
// ------------------------------------------------------------------------------------------------
template <int L, int V, int NQ>
__global__ __launch_bounds__(kBlock) void thr_scan_i8(ThrParams p) {
    constexpr int R = 64 / L;
    constexpr int UP = L * V;
    constexpr bool QREG = NQ * V * 4 <= 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int4* sq = reinterpret_cast<int4*>(smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = lane & (L - 1), g = lane / L;
    const TileDev tile = p.tiles[blockIdx.x];
    const SegDev seg = p.segs[tile.seg];
    const int4* __restrict__ X = static_cast<const int4*>(seg.rows);
    const int4* __restrict__ Q = static_cast<const int4*>(p.q);
    const int units = p.units;

    int4 qf[QREG ? NQ : 1][QREG ? V : 1];
    if constexpr (QREG) {
#pragma unroll
        for (int b = 0; b < NQ; ++b)
#pragma unroll
            for (int j = 0; j < V; ++j) qf[b][j] = Q[b * UP + t + j * L];
    } else {
        for (int i = tid; i < NQ * UP; i += kBlock) sq[i] = Q[i];
        __syncthreads();
    }
    auto qat = [&](int b, int j) -> int4 {
        if constexpr (QREG) return qf[b][j];
        else return sq[b * UP + t + j * L];
    };
    const int sim = p.sim, dim = p.dim;
    int32_t qn[NQ];
    float ms[NQ];
#pragma unroll
    for (int b = 0; b < NQ; ++b) {
        qn[b] = thr_qnorm_i8<L, V>([&](int j) { return qat(b, j); });
        ms[b] = b < p.q_count ? p.min_score[b] : __builtin_nanf("");
    }

    int64_t wb, we;
    thr_wave_range<R>(tile, wave, wb, we);
    const uint64_t* abits = p.accept ? p.accept[tile.seg] : nullptr;
    const size_t qstride = (size_t)p.n_tiles * 4 * p.wpw;
    const size_t wi = (size_t)blockIdx.x * 4 + wave;
    uint64_t* mw = p.mask + wi * p.wpw;

    ThrMask<NQ> hm;
    hm.init();
    uint32_t nvis = 0;

    walk_rows<R>(wb, we, abits, seg.ord_to_doc, lane, g, [&](const int64_t row, bool valid, bool accepted_known) {
        int32_t doc = 0;
        if (valid) {
            doc = seg.ord_to_doc ? seg.ord_to_doc[row] : (int32_t)row;
            if (abits && !accepted_known) valid = (abits[doc >> 6] >> (doc & 63)) & 1ull;
        }
        int4 xv[V];
        thr_load_row_i8<L, V>(X + row * units, valid, units, t, xv);
        const int32_t xn = valid ? seg.xnorm_i[row] : 0;
        nvis += __popcll(__ballot(t == 0 && valid));

        const int rel = (int)(row - wb);
        const int widx = __builtin_amdgcn_readfirstlane(rel) >> 6;
        if (widx != hm.idx) {
            hm.flush(mw, qstride, p.wpw, p.q_count, lane);
            hm.idx = widx;
        }
#pragma unroll
        for (int b = 0; b < NQ; ++b) {
            const float sc = thr_score_i8<L, V>(xv, [&](int j) { return qat(b, j); }, sim, qn[b], xn, dim);
            const bool hit = valid && sc >= ms[b];
            hm.bits[b] |= thr_step_bits<L>(hit, !accepted_known, rel, lane, t);
        }
    });
    hm.flush(mw, qstride, p.wpw, p.q_count, lane);

    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < NQ; ++b)
            if (b < p.q_count) p.counts[(size_t)b * p.n_tiles * 4 + wi] = (int32_t)hm.cnt[b];
    }
    if (p.visited && p.q0 == 0) add_visited_wg(&p.visited[tile.seg], nvis);
}

// ------------------------------------------------------------------------------------------------
// scan, float32 views, certified int8 first pass: the select path's bounds writer (sel_bounds: int8 lane
// configs by 16-byte units, U row groups loaded — unconditional, clamped, masked — before any is reduced,
// non-temporal int4 loads, sdot4, one float4 of bound terms per row) with the records replaced by a
// classification of each accepted row against min_score:
//   sure   cand && lb >= ms                    (score ≥ lb ≥ ms)   → the hit mask and the wave's count
//   maybe  cand && !(lb >= ms) && !(ub < ms)   → the maybe mask: thr_settle_f32 re-scores the row exactly
// and everything else no hit (!cand: a NaN bound, whose exact score is NaN too).  Both comparisons are false
// for a NaN ms, which would make every row a maybe: a NaN ms is tested once per query and makes every row
// a miss.  An out-of-range query's interval is [0, +inf]: every row a maybe (exact, and slow).
//
// Wave split: the masks are addressed per wave (wpw words, bit = row − the wave's first row) and the settle
// and the emit find a wave's rows with thr_wave_range<R> of the view's FLOAT32 lane config.  This kernel's
// R8 = 64 / L differs, so it takes the fp32 config's R (p.wave_R) for the split and steps by R8·U rows
// inside the wave's range: R8·U divides 64 and the steps start at multiples of it from the wave's first
// row, so a step's rows lie in one word, and no two waves ever store the same word.
// ------------------------------------------------------------------------------------------------
template <int L, int V, int NQ, bool FILT>
__global__ __launch_bounds__(kBlock) void thr_scan_sq8(ThrParams p) {
    constexpr int R = 64 / L;
    constexpr int U = 2;
    constexpr int S = R * U;   // rows per step
    static_assert(64 % S == 0 && U * NQ * 2 <= 32, "a step's rows in one word, its classes in one dword");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = lane & (L - 1), g = lane / L;
    const TileDev tile = p.tiles[blockIdx.x];
    const SegDev seg = p.segs[tile.seg];
    const uint64_t* abits = (FILT && p.accept) ? p.accept[tile.seg] : nullptr;
    const int4* __restrict__ X = p.rows8[tile.seg];
    const float4* __restrict__ AX = p.aux[tile.seg];
    const int u8 = p.units8, sim = p.sim;

    int4 qf[NQ][V];
    float4 qc[NQ];
    float qnd[NQ], ms[NQ];
    bool qopen[NQ], live[NQ];
#pragma unroll
    for (int b = 0; b < NQ; ++b) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int f = t + j * L;
            const int msk = f < u8 ? -1 : 0;
            const int4 v = p.q8[(size_t)b * u8 + (f < u8 ? f : 0)];
            qf[b][j] = make_int4(v.x & msk, v.y & msk, v.z & msk, v.w & msk);
        }
        const bool inq = b < p.q_count;
        qc[b] = p.qc[b];
        qnd[b] = sim == SIM_COSINE ? p.qnorm[b] : 0.0f;
        qopen[b] = inq && (p.qflags[b] & kQueryOutOfRange) != 0;
        ms[b] = inq ? p.min_score[b] : __builtin_nanf("");
        live[b] = ms[b] == ms[b];   // (wave-uniform) a NaN threshold: no row is a hit, none needs a re-score
    }

    int64_t wb, we;
    thr_wave_range_rt(tile, wave, p.wave_R, wb, we);
    const size_t qstride = (size_t)p.n_tiles * 4 * p.wpw;
    const size_t wi = (size_t)blockIdx.x * 4 + wave;
    uint64_t* hw = p.mask + wi * p.wpw;
    uint64_t* mw = p.maybe + wi * p.wpw;

    ThrMask<NQ> hm, mm;
    hm.init();
    mm.init();
    uint32_t nvis = 0;

    // one row group's classes against the NQ thresholds: bit 2b sure, bit 2b + 1 maybe (every lane calls it)
    auto classify = [&](const int4 (&x)[V], float4 axr, float xnd, bool valid) -> uint32_t {
        uint32_t cls = 0u;
#pragma unroll
        for (int b = 0; b < NQ; ++b) {
            int acc = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                acc = __builtin_amdgcn_sdot4(x[j].x, qf[b][j].x, acc, false);
                acc = __builtin_amdgcn_sdot4(x[j].y, qf[b][j].y, acc, false);
                acc = __builtin_amdgcn_sdot4(x[j].z, qf[b][j].z, acc, false);
                acc = __builtin_amdgcn_sdot4(x[j].w, qf[b][j].w, acc, false);
            }
            acc = lane_sum<L>(acc);
            float lb, ub;
            const bool cand =
                sq8_score_interval<true>(sim, acc, axr, qc[b], p.gam, p.g2, qnd[b], xnd, valid, qopen[b], lb, ub);
            // An out-of-range query's [0, +inf] is no certificate — its exact score may even be NaN — so none
            // of its rows is sure, whatever ms: every one is re-scored.  Nor is a COSINE row sure when |q|² or
            // |x|² is 0 (or not finite): the exact score is NaN, never a hit, while the transform of ±x/0
            // gives the interval [0, +inf], not NaN.
            const bool degen = sim == SIM_COSINE && !(qnd[b] > 0.0f && qnd[b] < __builtin_inff() && xnd > 0.0f &&
                                                      xnd < __builtin_inff());
            bool sure = cand && !qopen[b] && !degen && lb >= ms[b];
            bool maybe = cand && live[b] && !sure && !(ub < ms[b]);
            if (p.all_maybe) {   // (testing build) the settle decides every candidate row
                sure = false;
                maybe = cand;
            }
            cls |= ((sure ? 1u : 0u) | (maybe ? 2u : 0u)) << (2 * b);
        }
        return cls;
    };

    if (FILT && abits && !seg.ord_to_doc) {
        // a filter on a dense segment: walk_rows' compaction, as thr_scan_f32 — only accepted rows are read
        // (at 1 % selectivity 1 % of the bytes), R per step out of one 64-row window that starts at a multiple
        // of 64 from the wave's first row, each row setting its own bit
        walk_rows<R>(wb, we, abits, nullptr, lane, g, [&](const int64_t row, bool valid, bool) {
            const int64_t rc = valid ? row : wb;   // (a lane group past the window's accepted rows)
            const int4* xr = X + rc * u8;
            int4 x[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int f = t + j * L;
                const int4 xl = load_i4_nt(xr + (f < u8 ? f : 0));
                const int m = (valid && f < u8) ? -1 : 0;
                x[j] = make_int4(xl.x & m, xl.y & m, xl.z & m, xl.w & m);
            }
            const float4 axr = AX[rc];
            const float xnd = (sim == SIM_COSINE && valid) ? seg.xnorm_f[rc] : 0.0f;
            nvis += __popcll(__ballot(t == 0 && valid));
            const int rel = (int)(rc - wb);
            const int widx = __builtin_amdgcn_readfirstlane(rel) >> 6;   // lane 0's group is always a valid row
            if (widx != hm.idx) {
                hm.flush(hw, qstride, p.wpw, p.q_count, lane);
                mm.flush(mw, qstride, p.wpw, p.q_count, lane);
                hm.idx = mm.idx = widx;
            }
            const uint32_t cls = classify(x, axr, xnd, valid);
#pragma unroll
            for (int b = 0; b < NQ; ++b) {
                hm.bits[b] |= thr_step_bits<L>(((cls >> (2 * b)) & 1u) != 0u, false, rel, lane, t);
                mm.bits[b] |= thr_step_bits<L>(((cls >> (2 * b + 1)) & 1u) != 0u, false, rel, lane, t);
            }
        });
    } else {
        for (int64_t r0 = wb; r0 < we; r0 += S) {
            int64_t row[U];
            bool valid[U];
            int4 xv[U][V];
            float4 ax[U];
            bool some = false;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                row[u] = r0 + u * R + g;
                valid[u] = row[u] < we;
                if constexpr (FILT) {   // (a sparse segment, or a leaf without a bitset in a filtered call)
                    if (abits && valid[u]) {
                        const int32_t doc = seg.ord_to_doc ? seg.ord_to_doc[row[u]] : (int32_t)row[u];
                        valid[u] = (abits[doc >> 6] >> (doc & 63)) & 1ull;
                    }
                    some = some || valid[u];
                }
            }
            // under a filter a step without an accepted row is skipped before its loads are issued (one test
            // per step, ahead of all U groups' loads: those still overlap)
            if constexpr (FILT)
                if (!__ballot(some)) continue;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                // loads on a clamped row, results masked (no load under a branch: those serialise)
                const int64_t rc = row[u] < we ? row[u] : wb;
                const int4* xr = X + rc * u8;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int f = t + j * L;
                    const int4 x = load_i4_nt(xr + (f < u8 ? f : 0));
                    const int m = (valid[u] && f < u8) ? -1 : 0;
                    xv[u][j] = make_int4(x.x & m, x.y & m, x.z & m, x.w & m);
                }
                ax[u] = AX[rc];
            }
            const int rel0 = __builtin_amdgcn_readfirstlane((int)(r0 - wb));   // (wave-uniform) the step's first bit
            if ((rel0 >> 6) != hm.idx) {
                hm.flush(hw, qstride, p.wpw, p.q_count, lane);
                mm.flush(mw, qstride, p.wpw, p.q_count, lane);
                hm.idx = mm.idx = rel0 >> 6;
            }
            uint32_t cls = 0u;   // this lane's row groups: bit 2(u·NQ + b) sure, the next maybe
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float xnd = (sim == SIM_COSINE && valid[u]) ? seg.xnorm_f[row[u]] : 0.0f;
                nvis += __popcll(__ballot(t == 0 && valid[u]));
                cls |= classify(xv[u], ax[u], xnd, valid[u]) << (2 * NQ * u);
            }
            // lane j < R takes row group j's classes (every lane of a group holds the same); the step's rows
            // r0 + u·R + j are bits (rel0 & 63) + u·R + j of the word
            const uint32_t c = (uint32_t)__shfl((int)cls, (lane & (R - 1)) * L);
#pragma unroll
            for (int b = 0; b < NQ; ++b) {
                uint64_t sb = 0ull, mb = 0ull;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = 2 * (u * NQ + b);
                    sb |= __ballot(lane < R && ((c >> k) & 1u)) << (u * R);
                    mb |= __ballot(lane < R && ((c >> (k + 1)) & 1u)) << (u * R);
                }
                hm.bits[b] |= sb << (rel0 & 63);
                mm.bits[b] |= mb << (rel0 & 63);
            }
        }
    }
    hm.flush(hw, qstride, p.wpw, p.q_count, lane);
    mm.flush(mw, qstride, p.wpw, p.q_count, lane);

    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < NQ; ++b)
            if (b < p.q_count) p.counts[(size_t)b * p.n_tiles * 4 + wi] = (int32_t)hm.cnt[b];
    }
    if (p.visited && p.q0 == 0) add_visited_wg(&p.visited[tile.seg], nvis);
}

// ------------------------------------------------------------------------------------------------
// settle: one workgroup per (tile, query of the pass).  A wave whose maybe words are all zero has nothing
// to do; otherwise it walks them (walk_rows' compaction visits exactly the set bits), re-scores each row
// with the fp32 scan's arithmetic, ORs the rows with score ≥ min_score into its own hit-mask words and adds
// them to its count.  The rows it re-scored go to the view's device counter.
// ------------------------------------------------------------------------------------------------
template <int L, int V, bool L2K>
__global__ __launch_bounds__(kBlock) void thr_settle_f32(ThrParams p) {
    constexpr int R = 64 / L;
    constexpr int UP = L * V;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = lane & (L - 1), g = lane / L;
    const int b = blockIdx.y;
    const size_t wi = ((size_t)b * p.n_tiles + blockIdx.x) * 4 + wave;
    const uint64_t* my = p.maybe + wi * p.wpw;
    bool any = false;
    for (int i0 = 0; i0 < p.wpw; i0 += 64)
        if (i0 + lane < p.wpw) any = any || my[i0 + lane] != 0ull;
    uint32_t nset = 0;
    if (__ballot(any)) {   // (wave-uniform)
        const TileDev tile = p.tiles[blockIdx.x];
        const SegDev seg = p.segs[tile.seg];
        const float4* __restrict__ X = static_cast<const float4*>(seg.rows);
        const float4* __restrict__ Q = static_cast<const float4*>(p.q) + (size_t)b * UP;
        const int units = p.units, sim = p.sim;
        float4 qf[V];
#pragma unroll
        for (int j = 0; j < V; ++j) qf[j] = Q[t + j * L];
        auto qat = [&](int j) -> float4 { return qf[j]; };
        float qn = 0.0f;
        if (!L2K && sim == SIM_COSINE) qn = thr_qnorm_f32<L, V>(qat);
        const float ms = p.min_score[b];
        int64_t wb, we;
        thr_wave_range<R>(tile, wave, wb, we);
        uint64_t* hw = p.mask + wi * p.wpw;
        uint64_t bits = 0ull;   // the hit word in progress (wave-uniform)
        int idx = 0;
        uint32_t cnt = 0;
        auto flush = [&]() {
            if (bits != 0ull && idx < p.wpw) {
                if (lane == 0) hw[idx] |= bits;   // this wave's own word: the scan's sure bits stay
                cnt += (uint32_t)__popcll(bits);
            }
            bits = 0ull;
        };
        walk_rows<R>(0, we - wb, my, nullptr, lane, g, [&](const int64_t rel, bool valid, bool) {
            const int64_t row = wb + rel;
            float4 xv[V];
            thr_load_row_f32<L, V, false>(X + row * units, valid, units, t, xv);
            float xn = 0.0f;
            if (!L2K && sim == SIM_COSINE && valid) xn = seg.xnorm_f[row];
            const float sc = thr_score_f32<L, V, L2K>(xv, qat, sim, qn, xn);
            nset += __popcll(__ballot(t == 0 && valid));
            const int widx = __builtin_amdgcn_readfirstlane((int)rel) >> 6;   // lane 0: the step's first row
            if (widx != idx) {
                flush();
                idx = widx;
            }
            const bool hit = valid && sc >= ms;
            bits |= thr_step_bits<L>(hit, false, (int)rel, lane, t);
        });
        flush();
        if (lane == 0 && cnt) p.counts[wi] += (int32_t)cnt;
    }
    add_visited_wg(p.settled, nset);
}

// ------------------------------------------------------------------------------------------------
// offsets: one workgroup per (shard, query of the pass)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void thr_offsets(ThrParams p) {
    __shared__ long long s_wave[kBlock / 64];
    const int s = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t0 = p.shard_tile_begin[s], t1 = p.shard_tile_begin[s + 1];
    const int64_t n = (int64_t)(t1 - t0) * 4;
    const size_t base = ((size_t)b * p.n_tiles + t0) * 4;
    long long carry = 0;
    for (int64_t i0 = 0; i0 < n; i0 += kBlock) {
        const int64_t i = i0 + tid;
        const long long v = i < n ? (long long)p.counts[base + i] : 0ll;
        long long x = v;   // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        long long pre = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) {
            if (w < wave) pre += s_wave[w];
            all += s_wave[w];
        }
        if (i < n) p.offsets[base + i] = carry + pre + x - v;
        carry += all;
        __syncthreads();
    }
    const size_t o = (size_t)(p.q0 + b) * p.n_shards + s;
    const long long cnt = carry < (long long)p.cap ? carry : (long long)p.cap;
    if (tid == 0) {
        p.out_total[o] = carry;
        if (p.out_count) p.out_count[o] = (int32_t)cnt;
    }
    if (!p.out_docs) return;   // the top-k collector: no positional output (its lists carry their own zeros)
    // unused slots, as osk_seg_search leaves them
    for (int64_t i = cnt + tid; i < p.cap; i += kBlock) {
        p.out_docs[o * p.cap + i] = 0x7FFFFFFF;
        p.out_scores[o * p.cap + i] = -__builtin_inff();
    }
}

// ------------------------------------------------------------------------------------------------
// emit: one workgroup per (tile, query of the pass); each wave re-scores its own mask's rows
// ------------------------------------------------------------------------------------------------
template <int L, int V, bool L2K>
__global__ __launch_bounds__(kBlock) void thr_emit_f32(ThrParams p) {
    constexpr int R = 64 / L;
    constexpr int UP = L * V;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = lane & (L - 1), g = lane / L;
    const int b = blockIdx.y;
    const size_t wi = ((size_t)b * p.n_tiles + blockIdx.x) * 4 + wave;
    if (p.counts[wi] == 0) return;
    int64_t rank = p.offsets[wi];
    if (rank >= p.cap) return;   // past the capacity: counted, not returned
    const TileDev tile = p.tiles[blockIdx.x];
    const SegDev seg = p.segs[tile.seg];
    const float4* __restrict__ X = static_cast<const float4*>(seg.rows);
    const float4* __restrict__ Q = static_cast<const float4*>(p.q) + (size_t)b * UP;
    const int units = p.units, sim = p.sim;
    float4 qf[V];
#pragma unroll
    for (int j = 0; j < V; ++j) qf[j] = Q[t + j * L];
    auto qat = [&](int j) -> float4 { return qf[j]; };
    float qn = 0.0f;
    if (!L2K && sim == SIM_COSINE) qn = thr_qnorm_f32<L, V>(qat);
    int64_t wb, we;
    thr_wave_range<R>(tile, wave, wb, we);
    const size_t o = ((size_t)(p.q0 + b) * p.n_shards + tile.shard) * (size_t)p.cap;
    // the wave's mask words are a bitset over its rows relative to wb: walk_rows' compaction visits
    // exactly the set bits, in ascending order, R per step
    walk_rows<R>(0, we - wb, p.mask + wi * p.wpw, nullptr, lane, g, [&](const int64_t rel, bool valid, bool) {
        const int64_t row = wb + rel;
        float4 xv[V];
        thr_load_row_f32<L, V, false>(X + row * units, valid, units, t, xv);
        float xn = 0.0f;
        if (!L2K && sim == SIM_COSINE && valid) xn = seg.xnorm_f[row];
        const float sc = thr_score_f32<L, V, L2K>(xv, qat, sim, qn, xn);
        const uint64_t vm = __ballot(t == 0 && valid);
        const int64_t pos = rank + __popcll(vm & ((1ull << lane) - 1ull));
        if (t == 0 && valid && pos < p.cap) {
            const int32_t doc = seg.ord_to_doc ? seg.ord_to_doc[row] : (int32_t)row;
            p.out_docs[o + pos] = seg.doc_base + doc;
            p.out_scores[o + pos] = sc;
        }
        rank += __popcll(vm);
    });
}

template <int L, int V>
__global__ __launch_bounds__(kBlock) void thr_emit_i8(ThrParams p) {
    constexpr int R = 64 / L;
    constexpr int UP = L * V;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = lane & (L - 1), g = lane / L;
    const int b = blockIdx.y;
    const size_t wi = ((size_t)b * p.n_tiles + blockIdx.x) * 4 + wave;
    if (p.counts[wi] == 0) return;
    int64_t rank = p.offsets[wi];
    if (rank >= p.cap) return;
    const TileDev tile = p.tiles[blockIdx.x];
    const SegDev seg = p.segs[tile.seg];
    const int4* __restrict__ X = static_cast<const int4*>(seg.rows);
    const int4* __restrict__ Q = static_cast<const int4*>(p.q) + (size_t)b * UP;
    const int units = p.units, sim = p.sim, dim = p.dim;
    int4 qf[V];
#pragma unroll
    for (int j = 0; j < V; ++j) qf[j] = Q[t + j * L];
    auto qat = [&](int j) -> int4 { return qf[j]; };
    const int32_t qn = thr_qnorm_i8<L, V>(qat);
    int64_t wb, we;
    thr_wave_range<R>(tile, wave, wb, we);
    const size_t o = ((size_t)(p.q0 + b) * p.n_shards + tile.shard) * (size_t)p.cap;
    walk_rows<R>(0, we - wb, p.mask + wi * p.wpw, nullptr, lane, g, [&](const int64_t rel, bool valid, bool) {
        const int64_t row = wb + rel;
        int4 xv[V];
        thr_load_row_i8<L, V>(X + row * units, valid, units, t, xv);
        const int32_t xn = valid ? seg.xnorm_i[row] : 0;
        const float sc = thr_score_i8<L, V>(xv, qat, sim, qn, xn, dim);
        const uint64_t vm = __ballot(t == 0 && valid);
        const int64_t pos = rank + __popcll(vm & ((1ull << lane) - 1ull));
        if (t == 0 && valid && pos < p.cap) {
            const int32_t doc = seg.ord_to_doc ? seg.ord_to_doc[row] : (int32_t)row;
            p.out_docs[o + pos] = seg.doc_base + doc;
            p.out_scores[o + pos] = sc;
        }
        rank += __popcll(vm);
    });
}

// ------------------------------------------------------------------------------------------------
// collect: the best hits by score instead of all of them by position.  The emit's walk — a wave visits
// exactly its own mask's rows and re-scores them with the scan's functions, so the score bits are the k-NN
// entries' — with each hit's key make_key(score, doc_base + doc) going to `sink(key, row, owner)`: every
// lane calls it, key is 0 in the lanes past the step's rows and `owner` holds in one lane per row group.
// A wave without hits does no loads.  No comparison against min_score: a hit is the mask's decision.
// ------------------------------------------------------------------------------------------------
template <int L, int V, bool L2K, class Sink>
__device__ __forceinline__ void thr_hit_keys_f32(const ThrParams& p, int b, size_t wi, const TileDev& tile,
                                                 const SegDev& seg, int wave, int lane, Sink&& sink) {
    constexpr int R = 64 / L;
    constexpr int UP = L * V;
    const int t = lane & (L - 1), g = lane / L;
    const float4* __restrict__ X = static_cast<const float4*>(seg.rows);
    const float4* __restrict__ Q = static_cast<const float4*>(p.q) + (size_t)b * UP;
    const int units = p.units, sim = p.sim;
    float4 qf[V];
#pragma unroll
    for (int j = 0; j < V; ++j) qf[j] = Q[t + j * L];
    auto qat = [&](int j) -> float4 { return qf[j]; };
    float qn = 0.0f;
    if (!L2K && sim == SIM_COSINE) qn = thr_qnorm_f32<L, V>(qat);
    int64_t wb, we;
    thr_wave_range<R>(tile, wave, wb, we);
    walk_rows<R>(0, we - wb, p.mask + wi * p.wpw, nullptr, lane, g, [&](const int64_t rel, bool valid, bool) {
        const int64_t row = wb + rel;
        float4 xv[V];
        thr_load_row_f32<L, V, false>(X + row * units, valid, units, t, xv);
        float xn = 0.0f;
        if (!L2K && sim == SIM_COSINE && valid) xn = seg.xnorm_f[row];
        const float sc = thr_score_f32<L, V, L2K>(xv, qat, sim, qn, xn);
        uint64_t key = 0ull;
        if (valid) {
            const int32_t doc = seg.ord_to_doc ? seg.ord_to_doc[row] : (int32_t)row;
            key = make_key(sc, (uint32_t)(seg.doc_base + doc));
        }
        sink(key, row, t == 0);
    });
}

template <int L, int V, class Sink>
__device__ __forceinline__ void thr_hit_keys_i8(const ThrParams& p, int b, size_t wi, const TileDev& tile,
                                                const SegDev& seg, int wave, int lane, Sink&& sink) {
    constexpr int R = 64 / L;
    constexpr int UP = L * V;
    const int t = lane & (L - 1), g = lane / L;
    const int4* __restrict__ X = static_cast<const int4*>(seg.rows);
    const int4* __restrict__ Q = static_cast<const int4*>(p.q) + (size_t)b * UP;
    const int units = p.units, sim = p.sim, dim = p.dim;
    int4 qf[V];
#pragma unroll
    for (int j = 0; j < V; ++j) qf[j] = Q[t + j * L];
    auto qat = [&](int j) -> int4 { return qf[j]; };
    const int32_t qn = thr_qnorm_i8<L, V>(qat);
    int64_t wb, we;
    thr_wave_range<R>(tile, wave, wb, we);
    walk_rows<R>(0, we - wb, p.mask + wi * p.wpw, nullptr, lane, g, [&](const int64_t rel, bool valid, bool) {
        const int64_t row = wb + rel;
        int4 xv[V];
        thr_load_row_i8<L, V>(X + row * units, valid, units, t, xv);
        const int32_t xn = valid ? seg.xnorm_i[row] : 0;
        const float sc = thr_score_i8<L, V>(xv, qat, sim, qn, xn, dim);
        uint64_t key = 0ull;
        if (valid) {
            const int32_t doc = seg.ord_to_doc ? seg.ord_to_doc[row] : (int32_t)row;
            key = make_key(sc, (uint32_t)(seg.doc_base + doc));
        }
        sink(key, row, t == 0);
    });
}

// top: one workgroup per (tile, query of the pass), k ≤ kScanMaxK.  Each wave keeps the best k of its hits in
// lanes 0..k-1 (the scans' wave list), the four lists are folded by wave 0 and stored as the tile's list
// in scan_f32's cand layout — all k slots, zeros past the hits: the buffer is not cleared.
// F32: thr_hit_keys_f32<L, V, L2K>; else thr_hit_keys_i8<L, V> (L2K unused).
template <int L, int V, bool L2K, bool F32>
__device__ __forceinline__ void thr_top_tile(const ThrParams& p) {
    __shared__ uint64_t slist[4 * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, k = p.top_k;
    const size_t wi = ((size_t)b * p.n_tiles + blockIdx.x) * 4 + wave;
    uint64_t lk = 0ull, thr = 0ull;
    if (__builtin_amdgcn_readfirstlane(p.counts[wi]) != 0) {   // (wave-uniform; every wave reaches the barrier)
        const TileDev tile = p.tiles[blockIdx.x];
        const SegDev seg = p.segs[tile.seg];
        auto offer = [&](uint64_t key, int64_t, bool owner) { wave_offer(key, owner, lk, thr, lane, k); };
        if constexpr (F32) thr_hit_keys_f32<L, V, L2K>(p, b, wi, tile, seg, wave, lane, offer);
        else thr_hit_keys_i8<L, V>(p, b, wi, tile, seg, wave, lane, offer);
    }
    slist[wave * 64 + lane] = lane < k ? lk : 0ull;
    __syncthreads();
    if (wave == 0) {
        block_fold(slist, lk, thr, lane, k);
        if (lane < k) p.top_cand[((size_t)(p.q0 + b) * p.n_tiles + blockIdx.x) * k + lane] = lk;
    }
}
template <int L, int V, bool L2K>
__global__ __launch_bounds__(kBlock) void thr_top_f32(ThrParams p) {
    thr_top_tile<L, V, L2K, true>(p);
}
template <int L, int V>
__global__ __launch_bounds__(kBlock) void thr_top_i8(ThrParams p) {
    thr_top_tile<L, V, false, false>(p);
}

// keys: one workgroup per tile, the pass's query key_b, any k.  Each hit's key goes to its view row's slot
// of the select path's exact-key records (zeroed by the host before: every other row stays "no record").
template <int L, int V, bool L2K, bool F32>
__device__ __forceinline__ void thr_keys_tile(const ThrParams& p) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = p.key_b;
    const size_t wi = ((size_t)b * p.n_tiles + blockIdx.x) * 4 + wave;
    if (__builtin_amdgcn_readfirstlane(p.counts[wi]) == 0) return;
    const TileDev tile = p.tiles[blockIdx.x];
    const SegDev seg = p.segs[tile.seg];
    uint64_t* keys = p.top_keys + p.seg_vrow[tile.seg];
    auto store = [&](uint64_t key, int64_t row, bool owner) {
        if (owner && key != 0ull) keys[row] = key;
    };
    if constexpr (F32) thr_hit_keys_f32<L, V, L2K>(p, b, wi, tile, seg, wave, lane, store);
    else thr_hit_keys_i8<L, V>(p, b, wi, tile, seg, wave, lane, store);
}
template <int L, int V, bool L2K>
__global__ __launch_bounds__(kBlock) void thr_keys_f32(ThrParams p) {
    thr_keys_tile<L, V, L2K, true>(p);
}
template <int L, int V>
__global__ __launch_bounds__(kBlock) void thr_keys_i8(ThrParams p) {
    thr_keys_tile<L, V, false, false>(p);
}

// ------------------------------------------------------------------------------------------------
// dispatch: the scans' lane configs × NQ ∈ {1, kThrNQ} × {L2, dot-family} × {plain, non-temporal}
// ------------------------------------------------------------------------------------------------
using ThrFn = void (*)(ThrParams);
constexpr size_t kLdsMax = 160 * 1024;   // LDS per workgroup on gfx950

#define OSK_THR_F32_NT(L, V, NT)                                                                        \
    thr_scan_f32<L, V, 1, true, NT>, thr_scan_f32<L, V, kThrNQ, true, NT>, thr_scan_f32<L, V, 1, false, NT>, \
        thr_scan_f32<L, V, kThrNQ, false, NT>
#define OSK_THR_F32(L, V) {OSK_THR_F32_NT(L, V, false), OSK_THR_F32_NT(L, V, true)}
#define OSK_THR_I8(L, V) {thr_scan_i8<L, V, 1>, thr_scan_i8<L, V, kThrNQ>}
#define OSK_THR_EMIT(L, V) {thr_emit_f32<L, V, true>, thr_emit_f32<L, V, false>}

const ThrFn kThrScanF32[9][8] = {OSK_THR_F32(4, 2),  OSK_THR_F32(8, 2),   OSK_THR_F32(8, 4),
                                 OSK_THR_F32(16, 4), OSK_THR_F32(16, 8),  OSK_THR_F32(16, 12),
                                 OSK_THR_F32(32, 8), OSK_THR_F32(64, 8),  OSK_THR_F32(64, 16)};
const ThrFn kThrScanI8[9][2] = {OSK_THR_I8(4, 2),  OSK_THR_I8(8, 2),  OSK_THR_I8(8, 4),
                                OSK_THR_I8(16, 4), OSK_THR_I8(16, 8), OSK_THR_I8(16, 12),
                                OSK_THR_I8(32, 8), OSK_THR_I8(64, 8), OSK_THR_I8(64, 16)};
const ThrFn kThrEmitF32[9][2] = {OSK_THR_EMIT(4, 2),  OSK_THR_EMIT(8, 2),  OSK_THR_EMIT(8, 4),
                                 OSK_THR_EMIT(16, 4), OSK_THR_EMIT(16, 8), OSK_THR_EMIT(16, 12),
                                 OSK_THR_EMIT(32, 8), OSK_THR_EMIT(64, 8), OSK_THR_EMIT(64, 16)};
const ThrFn kThrEmitI8[9] = {thr_emit_i8<4, 2>,  thr_emit_i8<8, 2>,  thr_emit_i8<8, 4>,
                             thr_emit_i8<16, 4>, thr_emit_i8<16, 8>, thr_emit_i8<16, 12>,
                             thr_emit_i8<32, 8>, thr_emit_i8<64, 8>, thr_emit_i8<64, 16>};

// the int8 first pass: the prefilter's lane configs by 16-byte units (sel_bounds_cfg's) × NQ × filter
#define OSK_THR_SQ8(L, V)                                                                 \
    {{thr_scan_sq8<L, V, 1, false>, thr_scan_sq8<L, V, 1, true>},                         \
     {thr_scan_sq8<L, V, kThrNQ, false>, thr_scan_sq8<L, V, kThrNQ, true>}}
#define OSK_THR_SETTLE(L, V) {thr_settle_f32<L, V, true>, thr_settle_f32<L, V, false>}
const ThrFn kThrScanSq8[8][2][2] = {OSK_THR_SQ8(4, 1),  OSK_THR_SQ8(8, 1),  OSK_THR_SQ8(16, 1), OSK_THR_SQ8(16, 2),
                                    OSK_THR_SQ8(16, 3), OSK_THR_SQ8(16, 4), OSK_THR_SQ8(32, 4), OSK_THR_SQ8(64, 4)};
const ThrFn kThrSettleF32[9][2] = {OSK_THR_SETTLE(4, 2),  OSK_THR_SETTLE(8, 2),  OSK_THR_SETTLE(8, 4),
                                   OSK_THR_SETTLE(16, 4), OSK_THR_SETTLE(16, 8), OSK_THR_SETTLE(16, 12),
                                   OSK_THR_SETTLE(32, 8), OSK_THR_SETTLE(64, 8), OSK_THR_SETTLE(64, 16)};
int thr_sq8_cfg(int u8) {
    return u8 <= 4 ? 0 : u8 <= 8 ? 1 : u8 <= 16 ? 2 : u8 <= 32 ? 3 : u8 <= 48 ? 4 : u8 <= 64 ? 5 : u8 <= 128 ? 6 : 7;
}

// the collector over the pass's mask, by lane config: {L2, dot-family} for float32
#define OSK_THR_TOP(L, V) {thr_top_f32<L, V, true>, thr_top_f32<L, V, false>}
#define OSK_THR_KEYS(L, V) {thr_keys_f32<L, V, true>, thr_keys_f32<L, V, false>}
const ThrFn kThrTopF32[9][2] = {OSK_THR_TOP(4, 2),  OSK_THR_TOP(8, 2),  OSK_THR_TOP(8, 4),
                                OSK_THR_TOP(16, 4), OSK_THR_TOP(16, 8), OSK_THR_TOP(16, 12),
                                OSK_THR_TOP(32, 8), OSK_THR_TOP(64, 8), OSK_THR_TOP(64, 16)};
const ThrFn kThrTopI8[9] = {thr_top_i8<4, 2>,  thr_top_i8<8, 2>,  thr_top_i8<8, 4>,
                            thr_top_i8<16, 4>, thr_top_i8<16, 8>, thr_top_i8<16, 12>,
                            thr_top_i8<32, 8>, thr_top_i8<64, 8>, thr_top_i8<64, 16>};
const ThrFn kThrKeysF32[9][2] = {OSK_THR_KEYS(4, 2),  OSK_THR_KEYS(8, 2),  OSK_THR_KEYS(8, 4),
                                 OSK_THR_KEYS(16, 4), OSK_THR_KEYS(16, 8), OSK_THR_KEYS(16, 12),
                                 OSK_THR_KEYS(32, 8), OSK_THR_KEYS(64, 8), OSK_THR_KEYS(64, 16)};
const ThrFn kThrKeysI8[9] = {thr_keys_i8<4, 2>,  thr_keys_i8<8, 2>,  thr_keys_i8<8, 4>,
                             thr_keys_i8<16, 4>, thr_keys_i8<16, 8>, thr_keys_i8<16, 12>,
                             thr_keys_i8<32, 8>, thr_keys_i8<64, 8>, thr_keys_i8<64, 16>};

// a pass's outputs: the positional entries' four arrays and a capacity, or (top_k ≥ 1) the totals alone
bool thr_out_ok(const ThrParams& p) {
    if (p.top_k == 0) return p.cap >= 1 && p.out_docs && p.out_scores && p.out_count && p.out_total;
    return p.top_k >= 1 && p.cap == 0 && !p.out_docs && !p.out_scores && !p.out_count &&
           p.out_total;
}

// what every launch of a pass must satisfy; anything else is refused, never guessed
bool thr_params_ok(int enc, int cfg, const ThrParams& p) {
    return (enc == ENC_FLOAT32 || enc == ENC_BYTE) && cfg >= 0 && cfg < 9 && p.sim >= 0 && p.sim <= 3 &&
           p.q_count >= 1 && p.q_count <= kThrNQ && p.n_shards >= 1 &&
           p.wpw >= 1 && p.n_tiles >= 0 && p.units >= 1 && p.units <= cfg_padded_units(cfg) &&
           p.segs && p.tiles && p.q && p.min_score && p.mask && p.counts && p.offsets && p.shard_tile_begin &&
           thr_out_ok(p);
}

}  // namespace

int thr_words_per_wave(int cfg, int64_t max_tile_rows) {
    if (cfg < 0 || cfg >= 9 || max_tile_rows < 1) return 1;
    const int64_t R = 64 / kCfgLV[cfg][0];
    const int64_t per_wave = ((max_tile_rows + 4 * R - 1) / (4 * R)) * R;
    return (int)std::min<int64_t>(0x7FFFFFFF, (per_wave + 63) / 64);
}

hipError_t launch_thr_scan(int enc, int cfg, const ThrParams& p, hipStream_t s, hipEvent_t ev_start,
                           hipEvent_t ev_stop) {
    if (!thr_params_ok(enc, cfg, p) || p.n_tiles < 1) return hipErrorInvalidValue;
    const int slot = p.q_count <= 1 ? 0 : 1;
    const int NQ = slot ? kThrNQ : 1;
    const int L = kCfgLV[cfg][0], V = kCfgLV[cfg][1];
    const bool qreg = NQ * V * 4 <= 64;
    const size_t lds = qreg ? 0 : (size_t)NQ * L * V * 16;
    if (lds > kLdsMax) return hipErrorInvalidValue;
    ThrFn fn;
    if (enc == ENC_FLOAT32)
        fn = kThrScanF32[cfg][(g_tuning.scan_nt ? 4 : 0) + (p.sim == SIM_EUCLIDEAN ? 0 : 2) + slot];
    else
        fn = kThrScanI8[cfg][slot];
    if (ev_start || ev_stop)
        hipExtLaunchKernelGGL(fn, dim3(p.n_tiles), dim3(kBlock), lds, s, ev_start, ev_stop, 0, p);
    else
        hipLaunchKernelGGL(fn, dim3(p.n_tiles), dim3(kBlock), lds, s, p);
    return hipGetLastError();
}

// the int8 pass's own arguments: the view's float32 config must be the one that splits the tiles
static bool thr_sq8_params_ok(int cfg, const ThrParams& p) {
    return thr_params_ok(ENC_FLOAT32, cfg, p) && p.n_tiles >= 1 && p.maybe && p.maybe != p.mask && p.rows8 &&
           p.aux && p.q8 && p.qc && p.qnorm && p.qflags && p.settled && p.units8 >= 1 && p.units8 <= 256 &&
           p.units8 == (p.dim + 15) / 16 && p.wave_R == 64 / kCfgLV[cfg][0];
}

hipError_t launch_thr_scan_sq8(int cfg, const ThrParams& p, hipStream_t s, hipEvent_t ev_start,
                               hipEvent_t ev_stop) {
    if (!thr_sq8_params_ok(cfg, p)) return hipErrorInvalidValue;
    const ThrFn fn = kThrScanSq8[thr_sq8_cfg(p.units8)][p.q_count <= 1 ? 0 : 1][p.accept ? 1 : 0];
    if (ev_start || ev_stop)
        hipExtLaunchKernelGGL(fn, dim3(p.n_tiles), dim3(kBlock), 0, s, ev_start, ev_stop, 0, p);
    else
        hipLaunchKernelGGL(fn, dim3(p.n_tiles), dim3(kBlock), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_thr_settle(int cfg, const ThrParams& p, hipStream_t s) {
    if (!thr_sq8_params_ok(cfg, p)) return hipErrorInvalidValue;
    const ThrFn fn = kThrSettleF32[cfg][p.sim == SIM_EUCLIDEAN ? 0 : 1];
    hipLaunchKernelGGL(fn, dim3(p.n_tiles, p.q_count), dim3(kBlock), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_thr_offsets(const ThrParams& p, hipStream_t s) {
    if (p.q_count < 1 || p.q_count > kThrNQ || p.n_shards < 1 || p.n_tiles < 0 || !p.counts || !p.offsets ||
        !p.shard_tile_begin || !thr_out_ok(p))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(thr_offsets, dim3(p.n_shards, p.q_count), dim3(kBlock), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_thr_emit(int enc, int cfg, const ThrParams& p, hipStream_t s) {
    // (top_k == 0: the positional outputs are there; the collector's form of the parameters has none)
    if (!thr_params_ok(enc, cfg, p) || p.n_tiles < 1 || p.top_k != 0) return hipErrorInvalidValue;
    const ThrFn fn = enc == ENC_FLOAT32 ? kThrEmitF32[cfg][p.sim == SIM_EUCLIDEAN ? 0 : 1] : kThrEmitI8[cfg];
    hipLaunchKernelGGL(fn, dim3(p.n_tiles, p.q_count), dim3(kBlock), 0, s, p);
    return hipGetLastError();
}

// thr_emit's grid; the wave lists hold top_k ≤ kScanMaxK keys and the fold's LDS is static (4 lists of 64)
hipError_t launch_thr_top(int enc, int cfg, const ThrParams& p, hipStream_t s) {
    if (!thr_params_ok(enc, cfg, p) || p.n_tiles < 1 || p.top_k < 1 || p.top_k > kScanMaxK || !p.top_cand)
        return hipErrorInvalidValue;
    const ThrFn fn = enc == ENC_FLOAT32 ? kThrTopF32[cfg][p.sim == SIM_EUCLIDEAN ? 0 : 1] : kThrTopI8[cfg];
    hipLaunchKernelGGL(fn, dim3(p.n_tiles, p.q_count), dim3(kBlock), 0, s, p);
    return hipGetLastError();
}

// one query of the pass (key_b) over every tile
hipError_t launch_thr_keys(int enc, int cfg, const ThrParams& p, hipStream_t s) {
    if (!thr_params_ok(enc, cfg, p) || p.n_tiles < 1 || p.top_k < 1 || !p.top_keys || !p.seg_vrow || p.key_b < 0 ||
        p.key_b >= p.q_count)
        return hipErrorInvalidValue;
    const ThrFn fn = enc == ENC_FLOAT32 ? kThrKeysF32[cfg][p.sim == SIM_EUCLIDEAN ? 0 : 1] : kThrKeysI8[cfg];
    hipLaunchKernelGGL(fn, dim3(p.n_tiles), dim3(kBlock), 0, s, p);
    return hipGetLastError();
}

}  // namespace osk
