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

hipError_t launch_nest_topk(const NestParams& p, hipStream_t s) {
    if (p.q_count < 1 || p.q_count > kMaxNQ || p.n_ptiles < 1 || p.n_parents < 1 || p.k < 1 || p.k > kScanMaxK ||
        p.q0 < 0 || !p.best || !p.ptiles || !p.cand)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(nest_topk, dim3(p.n_ptiles, p.q_count), dim3(kBlock), 0, s, p);
    return hipGetLastError();
}

}  // namespace osk
