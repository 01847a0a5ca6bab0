// osk_nested.hip — exact nested k-NN: the k best parents, each represented by its best accepted child
// ([L] DiversifyingChildrenFloatKnnVectorQuery / DiversifyingChildrenByteKnnVectorQuery.exactSearch; what
// OpenSearch k-NN builds for a `knn` query inside a `nested` query).  DESIGN.md §3i.
//
//   nest_parents                 at registration: row → the rank of its parent among the segment's parents
//                                (the number of parent bits strictly below the row's doc = the rank of
//                                nextSetBit(doc)): a per-word rank plus a popcount of the masked word.
//   nest_scan_f32 / nest_scan_i8 the only pass that reads the corpus: scan_f32 / scan_i8's tiles, lane layout,
//                                filter pushdown and score arithmetic (osk_rowscore.h), with the wave top-k
//                                list replaced by a per-parent maximum of the hit key.  The hit key orders
//                                hits as Lucene does (score desc, doc asc), so "best child" (highest score,
//                                then lowest doc) is the 64-bit maximum; a NaN score has key 0 = no hit.
//                                Rows of one walk step ascend, so equal parents are adjacent: a segmented max
//                                over the step's R row groups (shuffles), then each run's last lane issues
//                                one no-return 64-bit atomic max into best[query][parent slot].  A missed
//                                merge (adjacency broken) only costs an extra atomic, never a wrong result.
//   nest_scan_sq8 + nest_settle_f32  float32 views whose int8 prefilter copy certifies (tune nest_sq8): the same
//                                best-child keys for every family that can reach the top k, from ¼ of the
//                                bytes — the int8 pass leaves each row's upper bound and each family's best
//                                lower bound LBp, nest_topk + merge_shards over the LBp keys give each shard's
//                                floor T (its k-th best LBp), and the settle re-scores exactly the rows with
//                                ub ≥ T and ub ≥ their family's LBp.
//   nest_topk                    per (parent tile, query): the top k of ≤ kNestPtile contiguous parent slots
//                                of one shard → cand[query][parent tile][k]; merge_shards then folds a
//                                shard's parent tiles exactly as it folds scan tiles.
#include <hip/hip_ext.h>

#include "osk_device.h"
#include "osk_internal.h"
#include "osk_rowscore.h"
#include "osk_wave.h"

namespace osk {

namespace {

// ------------------------------------------------------------------------------------------------
// registration: row → parent rank
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void nest_parents(const uint64_t* __restrict__ bits,
                                                       const int32_t* __restrict__ word_rank, int64_t n_words,
                                                       const int32_t* __restrict__ ord_to_doc, int64_t n_rows,
                                                       int32_t* __restrict__ row_parent) {
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= n_rows) return;
    const int64_t doc = ord_to_doc ? ord_to_doc[row] : row;
    const int64_t w = doc >> 6;
    int32_t pid = 0;
    if (w < n_words) pid = word_rank[w] + (int32_t)__popcll(bits[w] & ((1ull << (doc & 63)) - 1ull));
    row_parent[row] = pid;
}

// ------------------------------------------------------------------------------------------------
// The runs of one walk step: group g's row belongs to parent pid (−1: no row).  merge bit i: the group
// 2^i below holds the same parent (then so does every group between, when rows ascend); tail: the next
// group holds another parent.  Computed once per step, used for every query of the pass.
// ------------------------------------------------------------------------------------------------
template <int L>
struct NestRuns {
    int merge;
    bool tail;
    __device__ __forceinline__ void init(int pid, int g) {
        constexpr int R = 64 / L;
        merge = 0;
        tail = true;
        if constexpr (R > 1) {
            int i = 0;
#pragma unroll
            for (int d = 1; d < R; d <<= 1, ++i) {
                const int op = __shfl_up(pid, d * L);
                if (g >= d && op == pid) merge |= 1 << i;
            }
            const int np = __shfl_down(pid, L);
            tail = g == R - 1 || np != pid;
        }
    }
    // inclusive segmented prefix maximum over the step's groups: a run's tail ends with the run's maximum
    __device__ __forceinline__ unsigned long long fold(unsigned long long key) const {
        constexpr int R = 64 / L;
        if constexpr (R > 1) {
            int i = 0;
#pragma unroll
            for (int d = 1; d < R; d <<= 1, ++i) {
                const unsigned long long ok = __shfl_up(key, d * L);
                if (((merge >> i) & 1) && ok > key) key = ok;
            }
        }
        return key;
    }
    // ...of a 32-bit value (the int8 pass's sortable lower bounds)
    __device__ __forceinline__ uint32_t fold(uint32_t v) const {
        constexpr int R = 64 / L;
        if constexpr (R > 1) {
            int i = 0;
#pragma unroll
            for (int d = 1; d < R; d <<= 1, ++i) {
                const uint32_t ov = (uint32_t)__shfl_up((int)v, d * L);
                if (((merge >> i) & 1) && ov > v) v = ov;
            }
        }
        return v;
    }
};

// ------------------------------------------------------------------------------------------------
// scan, float32
// ------------------------------------------------------------------------------------------------
template <int L, int V, int NQ, bool L2K, bool NT>
__global__ __launch_bounds__(kBlock) void nest_scan_f32(NestParams p) {
    constexpr int R = 64 / L;
    constexpr int UP = L * V;
    constexpr bool QREG = NQ * V * 4 <= 64;   // query fragments in VGPRs, else read from LDS (scan_f32's rule)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4* sq = reinterpret_cast<float4*>(smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = lane & (L - 1), g = lane / L;
    const TileDev tile = p.tiles[blockIdx.x];
    const SegDev seg = p.segs[tile.seg];
    const NestSeg nseg = p.nsegs[tile.seg];
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
    float qn[NQ];
#pragma unroll
    for (int b = 0; b < NQ; ++b) {
        qn[b] = 0.0f;
        if (!L2K && sim == SIM_COSINE) qn[b] = thr_qnorm_f32<L, V>([&](int j) { return qat(b, j); });
    }

    int64_t wb, we;
    thr_wave_range<R>(tile, wave, wb, we);
    const uint64_t* abits = p.accept ? p.accept[tile.seg] : nullptr;
    uint32_t nvis = 0;

    walk_rows<R>(wb, we, abits, seg.ord_to_doc, lane, g, [&](const int64_t row, bool valid, bool accepted_known) {
        int32_t doc = 0;
        int pid = -1;
        if (valid) {
            pid = nseg.row_parent[row];   // (before the accept test: a rejected row keeps its family's run whole)
            doc = seg.ord_to_doc ? seg.ord_to_doc[row] : (int32_t)row;
            if (abits && !accepted_known) valid = (abits[doc >> 6] >> (doc & 63)) & 1ull;
        }
        float4 xv[V];
        thr_load_row_f32<L, V, NT>(X + row * units, valid, units, t, xv);
        float xn = 0.0f;
        if (!L2K && sim == SIM_COSINE && valid) xn = seg.xnorm_f[row];
        nvis += __popcll(__ballot(t == 0 && valid));

        NestRuns<L> runs;
        runs.init(pid, g);
        const int64_t slot = nseg.pbase + pid;
        const bool issue = t == 0 && runs.tail && pid >= 0 && slot < p.n_parents;
#pragma unroll
        for (int b = 0; b < NQ; ++b) {
            const float sc = thr_score_f32<L, V, L2K>(xv, [&](int j) { return qat(b, j); }, sim, qn[b], xn);
            unsigned long long key = valid ? make_key(sc, (uint32_t)(seg.doc_base + doc)) : 0ull;
            key = runs.fold(key);
            if (issue && key != 0ull && b < p.q_count)
                (void)__hip_atomic_fetch_max(p.best + (size_t)b * p.n_parents + slot, key, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        }
    });
    if (p.visited && p.q0 == 0) add_visited_wg(&p.visited[tile.seg], nvis);
}

// ------------------------------------------------------------------------------------------------
// scan, int8 (exact int32 sums)
// ------------------------------------------------------------------------------------------------
template <int L, int V, int NQ>
__global__ __launch_bounds__(kBlock) void nest_scan_i8(NestParams p) {
    constexpr int R = 64 / L;
    constexpr int UP = L * V;
    constexpr bool QREG = NQ * V * 4 <= 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int4* sq = reinterpret_cast<int4*>(smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = lane & (L - 1), g = lane / L;
    const TileDev tile = p.tiles[blockIdx.x];
    const SegDev seg = p.segs[tile.seg];
    const NestSeg nseg = p.nsegs[tile.seg];
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
#pragma unroll
    for (int b = 0; b < NQ; ++b) qn[b] = thr_qnorm_i8<L, V>([&](int j) { return qat(b, j); });

    int64_t wb, we;
    thr_wave_range<R>(tile, wave, wb, we);
    const uint64_t* abits = p.accept ? p.accept[tile.seg] : nullptr;
    uint32_t nvis = 0;

    walk_rows<R>(wb, we, abits, seg.ord_to_doc, lane, g, [&](const int64_t row, bool valid, bool accepted_known) {
        int32_t doc = 0;
        int pid = -1;
        if (valid) {
            pid = nseg.row_parent[row];
            doc = seg.ord_to_doc ? seg.ord_to_doc[row] : (int32_t)row;
            if (abits && !accepted_known) valid = (abits[doc >> 6] >> (doc & 63)) & 1ull;
        }
        int4 xv[V];
        thr_load_row_i8<L, V>(X + row * units, valid, units, t, xv);
        const int32_t xn = valid ? seg.xnorm_i[row] : 0;
        nvis += __popcll(__ballot(t == 0 && valid));

        NestRuns<L> runs;
        runs.init(pid, g);
        const int64_t slot = nseg.pbase + pid;
        const bool issue = t == 0 && runs.tail && pid >= 0 && slot < p.n_parents;
#pragma unroll
        for (int b = 0; b < NQ; ++b) {
            const float sc = thr_score_i8<L, V>(xv, [&](int j) { return qat(b, j); }, sim, qn[b], xn, dim);
            unsigned long long key = valid ? make_key(sc, (uint32_t)(seg.doc_base + doc)) : 0ull;
            key = runs.fold(key);
            if (issue && key != 0ull && b < p.q_count)
                (void)__hip_atomic_fetch_max(p.best + (size_t)b * p.n_parents + slot, key, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        }
    });
    if (p.visited && p.q0 == 0) add_visited_wg(&p.visited[tile.seg], nvis);
}

// ------------------------------------------------------------------------------------------------
// scan, float32 views, certified int8 first pass: thr_scan_sq8's loop — int8 lane configs by
// 16-byte units, U row groups loaded (unconditional, clamped, masked) before any is reduced, non-temporal
// int4 loads, sdot4, one float4 of bound terms per row, sq8_score_interval — with the classification
// replaced by
//   the ub record   sortable(ub) per (query, view row), 0 = no record (a row that is not accepted, or whose
//                   bound is NaN: its exact score is NaN too).  Unfiltered calls store every row's record, a
//                   step's contiguous run at once; under a filter only the steps that hold an accepted row
//                   store, so the host clears the records before a filtered scan: a row that is not accepted
//                   has no record and is never settled.
//   the LBp fold    sortable(lb) of every row that holds a real certificate (not an out-of-range query's
//                   [0, +inf], not a COSINE row with a degenerate norm; 0 otherwise), NestRuns' segmented maximum
//                   over each row group set (32-bit shuffles), one no-return atomic max per run tail of the key
//                   (max << 32) | (0xFFFFFFFF − the tail row's doc) into lbkey[query][parent slot].  Only the
//                   high word is a bound; the low word — a doc of that family — keeps the keys of different
//                   parents distinct for nest_topk / merge_shards.
// The settle finds its rows through the records, which are addressed by view row: it does not depend on this
// kernel's wave split, so the split is this lane config's own.
// ------------------------------------------------------------------------------------------------
template <int L, int V, int NQ, bool FILT>
__global__ __launch_bounds__(kBlock) void nest_scan_sq8(NestParams p) {
    constexpr int R = 64 / L;
    constexpr int U = 2;
    constexpr int S = R * U;   // rows per step
    static_assert(S <= 64, "a step's records are stored by one wave instruction");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = lane & (L - 1), g = lane / L;
    const TileDev tile = p.tiles[blockIdx.x];
    const SegDev seg = p.segs[tile.seg];
    const NestSeg nseg = p.nsegs[tile.seg];
    const uint64_t* abits = (FILT && p.accept) ? p.accept[tile.seg] : nullptr;
    const int4* __restrict__ X = p.rows8[tile.seg];
    const float4* __restrict__ AX = p.aux[tile.seg];
    uint32_t* __restrict__ ubs = p.ub + p.seg_vrow[tile.seg];   // query b's records at ubs + b·n_rows
    const int u8 = p.units8, sim = p.sim;

    int4 qf[NQ][V];
    float4 qc[NQ];
    float qnd[NQ];
    bool qopen[NQ], qdeg[NQ];
#pragma unroll
    for (int b = 0; b < NQ; ++b) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int f = t + j * L;
            const int msk = f < u8 ? -1 : 0;
            const int4 v = p.q8[(size_t)b * u8 + (f < u8 ? f : 0)];
            qf[b][j] = make_int4(v.x & msk, v.y & msk, v.z & msk, v.w & msk);
        }
        qc[b] = p.qc[b];
        qnd[b] = sim == SIM_COSINE ? p.qnorm[b] : 0.0f;
        qopen[b] = b < p.q_count && (p.qflags[b] & kQueryOutOfRange) != 0;
        qdeg[b] = sim == SIM_COSINE && !(qnd[b] > 0.0f && qnd[b] < __builtin_inff());
    }

    int64_t wb, we;
    thr_wave_range<R>(tile, wave, wb, we);
    uint32_t nvis = 0;

    // one row group against the NQ queries (every lane calls it): rec[b] = the row's ub record, lk[b] = its
    // LBp key (0: no real certificate)
    auto bound = [&](const int4 (&x)[V], float4 axr, float xnd, bool valid, uint32_t (&rec)[NQ], uint32_t (&lk)[NQ]) {
        const bool xdeg = sim == SIM_COSINE && !(xnd > 0.0f && xnd < __builtin_inff());
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
            // An out-of-range query's [0, +inf] is no certificate, nor is the interval of a COSINE row when |q|²
            // or |x|² is 0 or not finite (the exact score is NaN, the transform of ±x/0 gives [0, +inf]): such a
            // row keeps its record — it is always settled — and contributes nothing to LBp.
            const bool real = cand && !qopen[b] && !qdeg[b] && !xdeg;
            rec[b] = cand ? float_to_sortable(ub) : 0u;
            lk[b] = real ? float_to_sortable(lb) : 0u;   // (never 0 for a number)
        }
    };
    // the runs of one row group set → lbkey
    auto fold = [&](int pid, uint32_t dockey, const uint32_t (&lk)[NQ]) {
        NestRuns<L> runs;
        runs.init(pid, g);
        const int64_t slot = nseg.pbase + pid;
        const bool issue = t == 0 && runs.tail && pid >= 0 && slot < p.n_parents;
#pragma unroll
        for (int b = 0; b < NQ; ++b) {
            const uint32_t best = runs.fold(lk[b]);
            if (issue && best != 0u && b < p.q_count)
                (void)__hip_atomic_fetch_max(p.lbkey + (size_t)b * p.n_parents + slot,
                                             ((unsigned long long)best << 32) | (unsigned long long)dockey,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };

    if (FILT && abits && !seg.ord_to_doc) {
        // a filter on a dense segment: walk_rows' compaction — only accepted rows are read, each stores its own
        // record (the records were cleared)
        walk_rows<R>(wb, we, abits, nullptr, lane, g, [&](const int64_t row, bool valid, bool) {
            const int64_t rc = valid ? row : wb;   // (a lane group past the window's accepted rows)
            const int pid = valid ? nseg.row_parent[rc] : -1;
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
            uint32_t rec[NQ];
            uint32_t lk[NQ];
            bound(x, axr, xnd, valid, rec, lk);
            if (t == 0 && valid) {
#pragma unroll
                for (int b = 0; b < NQ; ++b)
                    if (b < p.q_count) ubs[(size_t)b * p.n_rows + rc] = rec[b];
            }
            fold(pid, 0xFFFFFFFFu - (uint32_t)(seg.doc_base + (int32_t)rc), lk);
        });
    } else {
        // (rows as 32-bit offsets from the wave's first row: a tile holds < 2^31 rows)
        const int nw = (int)(we - wb);
        X += wb * u8;
        AX += wb;
        const int32_t* __restrict__ rp = nseg.row_parent + wb;
        const int32_t* __restrict__ o2d = seg.ord_to_doc ? seg.ord_to_doc + wb : nullptr;
        const float* __restrict__ xnf = sim == SIM_COSINE ? seg.xnorm_f + wb : nullptr;
        const uint32_t dk0 = 0xFFFFFFFFu - (uint32_t)seg.doc_base;
        uint32_t* __restrict__ ubw = ubs + wb;
        for (int r0 = 0; r0 < nw; r0 += S) {
            bool valid[U];
            int pid[U];
            uint32_t dockey[U];
            int4 xv[U][V];
            float4 ax[U];
            bool some = false;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int row = r0 + u * R + g;
                valid[u] = row < nw;
                pid[u] = -1;
                dockey[u] = 0u;
                if (valid[u]) {
                    pid[u] = rp[row];   // (before the accept test: a rejected row keeps its family's run whole)
                    const int32_t doc = o2d ? o2d[row] : (int32_t)(wb + row);
                    dockey[u] = dk0 - (uint32_t)doc;
                    if constexpr (FILT)   // (a sparse segment, or a leaf without a bitset in a filtered call)
                        if (abits) valid[u] = (abits[doc >> 6] >> (doc & 63)) & 1ull;
                }
                if constexpr (FILT) some = some || valid[u];
            }
            // under a filter a step without an accepted row is skipped before its loads are issued; its rows'
            // records stay cleared
            if constexpr (FILT)
                if (!__ballot(some)) continue;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                // loads on a clamped row, results masked (no load under a branch: those serialise)
                const int row = r0 + u * R + g;
                const int rc = row < nw ? row : 0;
                const int4* xr = X + (int64_t)rc * u8;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int f = t + j * L;
                    const int4 x = load_i4_nt(xr + (f < u8 ? f : 0));
                    const int m = (valid[u] && f < u8) ? -1 : 0;
                    xv[u][j] = make_int4(x.x & m, x.y & m, x.z & m, x.w & m);
                }
                ax[u] = AX[rc];
            }
            uint32_t rec[U][NQ];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float xnd = (xnf && valid[u]) ? xnf[r0 + u * R + g] : 0.0f;
                nvis += __popcll(__ballot(t == 0 && valid[u]));
                uint32_t lk[NQ];
                bound(xv[u], ax[u], xnd, valid[u], rec[u], lk);
                fold(pid[u], dockey[u], lk);
            }
            // lane j < S takes row r0 + j's records (row group j mod R of set j / R; every lane of a group holds
            // the same): the step's contiguous run, one store per query
            const int src = (lane & (R - 1)) * L;
            const bool mine = lane < S && r0 + lane < nw;
#pragma unroll
            for (int b = 0; b < NQ; ++b) {
                uint32_t val = 0u;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t ru = (uint32_t)__shfl((int)rec[u][b], src);
                    if (lane / R == u) val = ru;
                }
                if (mine && b < p.q_count) ubw[(size_t)b * p.n_rows + r0 + lane] = val;
            }
        }
    }
    if (p.visited && p.q0 == 0) add_visited_wg(&p.visited[tile.seg], nvis);
}

// ------------------------------------------------------------------------------------------------
// settle: one workgroup per (scan tile, query of the pass), in the view's float32 lane config.  T = the k-th
// best LBp key's score bits of the tile's shard (0 when the shard has fewer than k).  Each wave walks its rows
// 64 at a time: lane i reads row i's record, its parent's LBp, and one ballot gives the rows with
// record ≠ 0, ub ≥ T and ub ≥ LBp — the only rows that can be the best child of a top-k family.  Those are
// compacted (walk_rows' permutation), re-scored R per step with the fp32 scan's arithmetic and folded into
// best by the same 64-bit atomic max as nest_scan_f32's.
// ------------------------------------------------------------------------------------------------
template <int L, int V, bool L2K>
__global__ __launch_bounds__(kBlock) void nest_settle_f32(NestParams p) {
    constexpr int R = 64 / L;
    constexpr int UP = L * V;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = lane & (L - 1), g = lane / L;
    const int b = blockIdx.y;
    const TileDev tile = p.tiles[blockIdx.x];
    const SegDev seg = p.segs[tile.seg];
    const NestSeg nseg = p.nsegs[tile.seg];
    const float4* __restrict__ X = static_cast<const float4*>(seg.rows);
    const float4* __restrict__ Q = static_cast<const float4*>(p.q) + (size_t)b * UP;
    const uint32_t* __restrict__ ubs = p.ub + (size_t)b * p.n_rows + p.seg_vrow[tile.seg];
    const unsigned long long* __restrict__ lbq = p.lbkey + (size_t)b * p.n_parents;
    unsigned long long* __restrict__ bq = p.best + (size_t)b * p.n_parents;
    const int units = p.units, sim = p.sim;
    const size_t fo = (size_t)b * p.n_shards + tile.shard;
    const uint32_t T = p.floor_counts[fo] == p.k ? (uint32_t)(p.floor_keys[fo * p.k + (p.k - 1)] >> 32) : 0u;

    float4 qf[V];
#pragma unroll
    for (int j = 0; j < V; ++j) qf[j] = Q[t + j * L];
    auto qat = [&](int j) -> float4 { return qf[j]; };
    float qn = 0.0f;
    if (!L2K && sim == SIM_COSINE) qn = thr_qnorm_f32<L, V>(qat);

    int64_t wb, we;
    thr_wave_range<R>(tile, wave, wb, we);
    uint32_t nset = 0;
    for (int64_t w0 = wb; w0 < we; w0 += 64) {
        const int64_t mine = w0 + lane;
        const uint32_t rec = mine < we ? ubs[mine] : 0u;
        bool want = rec != 0u;
        if (want && !p.all_settle) {
            const int64_t slot = nseg.pbase + nseg.row_parent[mine];
            const uint32_t lbp = slot < p.n_parents ? (uint32_t)(lbq[slot] >> 32) : 0u;
            want = rec >= T && rec >= lbp;
        }
        const uint64_t m = __ballot(want);
        if (m == 0ull) continue;
        const int n = __popcll(m);
        nset += (uint32_t)n;
        // the positions of the n set bits into lanes 0..n-1 (walk_rows' permutation)
        const bool bit = (m >> lane) & 1ull;
        const int below = __popcll(m & ((1ull << lane) - 1ull));
        const int dst = bit ? below : n + (lane - below);
        const int pos = __builtin_amdgcn_ds_permute(dst << 2, lane);
        for (int i0 = 0; i0 < n; i0 += R) {
            const int idx = i0 + g;
            const bool valid = idx < n;
            const int64_t row = w0 + __shfl(pos, idx < 64 ? idx : 0);   // (a set bit's row, or some row of the window < we)
            float4 xv[V];
            thr_load_row_f32<L, V, false>(X + row * units, valid, units, t, xv);
            float xn = 0.0f;
            if (!L2K && sim == SIM_COSINE && valid) xn = seg.xnorm_f[row];
            const float sc = thr_score_f32<L, V, L2K>(xv, qat, sim, qn, xn);
            if (t == 0 && valid) {
                const int32_t doc = seg.ord_to_doc ? seg.ord_to_doc[row] : (int32_t)row;
                const int64_t slot = nseg.pbase + nseg.row_parent[row];
                const unsigned long long key = make_key(sc, (uint32_t)(seg.doc_base + doc));
                if (key != 0ull && slot < p.n_parents)
                    (void)__hip_atomic_fetch_max(bq + slot, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    add_visited_wg(p.settled, nset);   // (wave-uniform; lane 0 of each wave adds it)
}

// ------------------------------------------------------------------------------------------------
// top k of a parent tile: one workgroup per (parent tile, query of the pass)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void nest_topk(NestParams p) {
    __shared__ uint64_t lists[4 * 64];
    const int pt = blockIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const NestPtile r = p.ptiles[pt];
    const int64_t end = min(r.end, p.n_parents);
    const unsigned long long* __restrict__ bq = p.best + (size_t)b * p.n_parents;
    const int k = p.k;
    uint64_t lk = 0ull, thr = 0ull;
    for (int64_t base = r.begin + (int64_t)wave * 64; base < end; base += kBlock) {
        const int64_t i = base + lane;
        const uint64_t key = i < end ? bq[i] : 0ull;
        wave_offer(key, true, lk, thr, lane, k);
    }
    lists[wave * 64 + lane] = lane < k ? lk : 0ull;
    __syncthreads();
    if (wave == 0) {
        block_fold(lists, lk, thr, lane, k);
        if (lane < k) p.cand[((size_t)(p.q0 + b) * p.n_ptiles + pt) * k + lane] = lk;
    }
}

// ------------------------------------------------------------------------------------------------
// dispatch: the scans' lane configs × NQ ∈ {1, kMaxNQ} × {L2, dot-family} × {plain, non-temporal}
// ------------------------------------------------------------------------------------------------
using NestFn = void (*)(NestParams);
constexpr size_t kLdsMax = 160 * 1024;   // LDS per workgroup on gfx950

#define OSK_NEST_F32_NT(L, V, NT)                                                                               \
    nest_scan_f32<L, V, 1, true, NT>, nest_scan_f32<L, V, kMaxNQ, true, NT>, nest_scan_f32<L, V, 1, false, NT>, \
        nest_scan_f32<L, V, kMaxNQ, false, NT>
#define OSK_NEST_F32(L, V) {OSK_NEST_F32_NT(L, V, false), OSK_NEST_F32_NT(L, V, true)}
#define OSK_NEST_I8(L, V) {nest_scan_i8<L, V, 1>, nest_scan_i8<L, V, kMaxNQ>}

const NestFn kNestScanF32[9][8] = {OSK_NEST_F32(4, 2),  OSK_NEST_F32(8, 2),  OSK_NEST_F32(8, 4),
                                   OSK_NEST_F32(16, 4), OSK_NEST_F32(16, 8), OSK_NEST_F32(16, 12),
                                   OSK_NEST_F32(32, 8), OSK_NEST_F32(64, 8), OSK_NEST_F32(64, 16)};
const NestFn kNestScanI8[9][2] = {OSK_NEST_I8(4, 2),  OSK_NEST_I8(8, 2),  OSK_NEST_I8(8, 4),
                                  OSK_NEST_I8(16, 4), OSK_NEST_I8(16, 8), OSK_NEST_I8(16, 12),
                                  OSK_NEST_I8(32, 8), OSK_NEST_I8(64, 8), OSK_NEST_I8(64, 16)};

// the int8 first pass: the prefilter's lane configs by 16-byte units (thr_scan_sq8's) × NQ × filter; the settle
// in the view's float32 lane config
#define OSK_NEST_SQ8(L, V)                                                                    \
    {{nest_scan_sq8<L, V, 1, false>, nest_scan_sq8<L, V, 1, true>},                           \
     {nest_scan_sq8<L, V, kNestSq8NQ, false>, nest_scan_sq8<L, V, kNestSq8NQ, true>}}
#define OSK_NEST_SETTLE(L, V) {nest_settle_f32<L, V, true>, nest_settle_f32<L, V, false>}
const NestFn kNestScanSq8[8][2][2] = {OSK_NEST_SQ8(4, 1),  OSK_NEST_SQ8(8, 1),  OSK_NEST_SQ8(16, 1),
                                      OSK_NEST_SQ8(16, 2), OSK_NEST_SQ8(16, 3), OSK_NEST_SQ8(16, 4),
                                      OSK_NEST_SQ8(32, 4), OSK_NEST_SQ8(64, 4)};
const NestFn kNestSettleF32[9][2] = {OSK_NEST_SETTLE(4, 2),  OSK_NEST_SETTLE(8, 2),  OSK_NEST_SETTLE(8, 4),
                                     OSK_NEST_SETTLE(16, 4), OSK_NEST_SETTLE(16, 8), OSK_NEST_SETTLE(16, 12),
                                     OSK_NEST_SETTLE(32, 8), OSK_NEST_SETTLE(64, 8), OSK_NEST_SETTLE(64, 16)};
int nest_sq8_cfg(int u8) {
    return u8 <= 4 ? 0 : u8 <= 8 ? 1 : u8 <= 16 ? 2 : u8 <= 32 ? 3 : u8 <= 48 ? 4 : u8 <= 64 ? 5 : u8 <= 128 ? 6 : 7;
}

// what both launches of an int8 pass must satisfy; anything else is refused, never guessed
bool nest_sq8_params_ok(int cfg, const NestParams& p) {
    return cfg >= 0 && cfg < 9 && p.sim >= 0 && p.sim <= 3 && p.q_count >= 1 && p.q_count <= kNestSq8NQ &&
           p.n_tiles >= 1 && p.n_parents >= 1 && p.n_rows >= 1 && p.n_shards >= 1 && p.k >= 1 && p.k <= kScanMaxK &&
           p.units >= 1 && p.units <= cfg_padded_units(cfg) && p.units8 >= 1 && p.units8 <= 256 &&
           p.units8 == (p.dim + 15) / 16 && p.segs && p.tiles && p.nsegs && p.q && p.best && p.ub && p.lbkey &&
           p.seg_vrow && p.rows8 && p.aux && p.q8 && p.qc && p.qnorm && p.qflags && p.settled;
}

}  // namespace

hipError_t launch_nest_parents(const uint64_t* parent_bits, const int32_t* word_rank, int64_t n_words,
                               const int32_t* ord_to_doc, int64_t n_rows, int32_t* row_parent, hipStream_t s) {
    if (!parent_bits || !word_rank || !row_parent || n_words < 1 || n_rows < 1) return hipErrorInvalidValue;
    const int64_t grid = (n_rows + kBlock - 1) / kBlock;
    if (grid > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nest_parents, dim3((unsigned)grid), dim3(kBlock), 0, s, parent_bits, word_rank, n_words,
                       ord_to_doc, n_rows, row_parent);
    return hipGetLastError();
}

hipError_t launch_nest_scan(int enc, int cfg, const NestParams& p, hipStream_t s, hipEvent_t ev_start,
                            hipEvent_t ev_stop) {
    if ((enc != ENC_FLOAT32 && enc != ENC_BYTE) || cfg < 0 || cfg >= 9 || p.sim < 0 || p.sim > 3 || p.q_count < 1 ||
        p.q_count > kMaxNQ || p.n_tiles < 1 || p.n_parents < 1 || p.units < 1 ||
        p.units > cfg_padded_units(cfg) || !p.segs || !p.tiles || !p.nsegs || !p.q || !p.best)
        return hipErrorInvalidValue;
    const int slot = p.q_count <= 1 ? 0 : 1;
    const int NQ = slot ? kMaxNQ : 1;
    const int L = kCfgLV[cfg][0], V = kCfgLV[cfg][1];
    const bool qreg = NQ * V * 4 <= 64;
    const size_t lds = qreg ? 0 : (size_t)NQ * L * V * 16;
    if (lds + 64 > kLdsMax) return hipErrorInvalidValue;
    NestFn fn;
    if (enc == ENC_FLOAT32)
        fn = kNestScanF32[cfg][(g_tuning.scan_nt ? 4 : 0) + (p.sim == SIM_EUCLIDEAN ? 0 : 2) + slot];
    else
        fn = kNestScanI8[cfg][slot];
    if (ev_start || ev_stop)
        hipExtLaunchKernelGGL(fn, dim3(p.n_tiles), dim3(kBlock), lds, s, ev_start, ev_stop, 0, p);
    else
        hipLaunchKernelGGL(fn, dim3(p.n_tiles), dim3(kBlock), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_nest_scan_sq8(int cfg, const NestParams& p, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (!nest_sq8_params_ok(cfg, p)) return hipErrorInvalidValue;
    const NestFn fn = kNestScanSq8[nest_sq8_cfg(p.units8)][p.q_count <= 1 ? 0 : 1][p.accept ? 1 : 0];
    if (ev_start || ev_stop)
        hipExtLaunchKernelGGL(fn, dim3(p.n_tiles), dim3(kBlock), 0, s, ev_start, ev_stop, 0, p);
    else
        hipLaunchKernelGGL(fn, dim3(p.n_tiles), dim3(kBlock), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_nest_settle(int cfg, const NestParams& p, hipStream_t s) {
    if (!nest_sq8_params_ok(cfg, p) || !p.floor_keys || !p.floor_counts) return hipErrorInvalidValue;
    const NestFn fn = kNestSettleF32[cfg][p.sim == SIM_EUCLIDEAN ? 0 : 1];
    hipLaunchKernelGGL(fn, dim3(p.n_tiles, p.q_count), dim3(kBlock), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_nest_topk(const NestParams& p, hipStream_t s) {
    if (p.q_count < 1 || p.q_count > kMaxNQ || p.n_ptiles < 1 || p.n_parents < 1 || p.k < 1 || p.k > kScanMaxK ||
        p.q0 < 0 || !p.best || !p.ptiles || !p.cand)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(nest_topk, dim3(p.n_ptiles, p.q_count), dim3(kBlock), 0, s, p);
    return hipGetLastError();
}

}  // namespace osk
