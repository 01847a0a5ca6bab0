// osk_hamming.hip — exact Hamming k-NN over packed bits (OSK_BYTE / OSK_HAMMING fields, osknn.h).
//
//   scan_ham          scan_i8's job: ≤ kMaxNQ queries per launch (p.q0 / p.q_count), accept bitsets through
//                     walk_rows (with the dense-field compaction), ord_to_doc, doc_base, visited; a top-k
//                     list per wave (wave_offer), folded to k keys per (query, tile) in p.cand (block_fold).
//   scan_ham_stream   scan_i8_stream's job: one query, no filter; U row groups loaded (non-temporal, clamped
//                     rows, masked values) before any is scored, so a wave keeps ≈ U·V KiB in flight.
//   sel_keys_ham      the select path's exact key writer (k > kScanMaxK): one key per row into p.keys.
//
// A row is `units` 16-byte units of packed bits (zero padded by staging); d(q, x) = popcount(q XOR x), an exact
// integer, and the score is score_hamming(d) (osk_common.h).  Per unit and query: four v_xor_b32 and four
// v_bcnt_u32_b32, the count's add folded into v_bcnt's second operand.  Sums are exact, so the
// lane layout changes no result, only the speed.  All three kernels share one table of exact-width lane
// configs, L lanes per row × V units per lane, by the row's units (ham_cfg):
//
//   units      1      2      3–4    5–8    9–16    17–32   33–48   49–64   65–128  129–256
//   bytes     ≤16    ≤32    ≤64    ≤128   ≤256    ≤512    ≤768    ≤1024   ≤2048   ≤4096
//   (L, V)   (1,1)  (2,1)  (4,1)  (8,1)  (16,1)  (16,2)  (16,3)  (16,4)  (32,4)  (64,4)
//   rows/wave  64     32     16      8      4       4       4       4       2       1
//
// One row per lane at 1 unit: the query's four dwords are wave-uniform (scalar registers), no cross-lane
// reduction, all 64 lanes offer keys.  Every load instruction of every config reads 1 KiB of contiguous row
// bytes.  Units at or past `units` (L·V > units) are masked to zero on both sides, so padding adds nothing to
// a distance and nothing past a row is relied on.  A tile is any row range of one segment: the four waves split
// it by this file's own R = 64 / L.
#include <hip/hip_ext.h>

#include "osk_device.h"
#include "osk_internal.h"
#include "osk_wave.h"

namespace osk {

namespace {

// acc + popcount(a XOR b): v_xor_b32 + v_bcnt_u32_b32 with acc as the count's second operand.  The empty asm
// pins the sum as one chain: left free, the compiler re-associates the adds into a tree of bare counts
// (v_bcnt …, 0) and separate adds.
__device__ __forceinline__ int ham_word(int a, int b, int acc) {
    acc = __builtin_popcount((uint32_t)(a ^ b)) + acc;
    asm("" : "+v"(acc));
    return acc;
}
// acc + popcount(x XOR q) over one 16-byte unit
__device__ __forceinline__ int ham_unit(const int4& x, const int4& q, int acc) {
    acc = ham_word(x.x, q.x, acc);
    acc = ham_word(x.y, q.y, acc);
    acc = ham_word(x.z, q.z, acc);
    acc = ham_word(x.w, q.w, acc);
    return acc;
}
__device__ __forceinline__ int4 mask4(const int4& v, bool keep) {
    const int m = keep ? -1 : 0;
    return make_int4(v.x & m, v.y & m, v.z & m, v.w & m);
}

template <int L, int V, int NQ>
__global__ __launch_bounds__(kBlock) void scan_ham(HamParams p) {
    constexpr int R = 64 / L;
    constexpr int LV = L * V;
    constexpr bool QREG = NQ * V * 4 <= 64;   // query fragments in registers, else read from LDS
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int4* sq = reinterpret_cast<int4*>(smem);
    uint64_t* slist = reinterpret_cast<uint64_t*>(smem + (QREG ? 0 : NQ * LV * 16));

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform: scalar loop control
    const int t = L == 1 ? 0 : (lane & (L - 1)), g = lane / L;
    const TileDev tile = p.tiles[blockIdx.x];
    const SegDev seg = p.segs[tile.seg];
    const int4* __restrict__ X = static_cast<const int4*>(seg.rows);
    const int4* __restrict__ Q = static_cast<const int4*>(p.q);
    const int units = p.units, qs = p.q_units;

    int4 qf[QREG ? NQ : 1][QREG ? V : 1];
    if constexpr (QREG) {
#pragma unroll
        for (int b = 0; b < NQ; ++b)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int f = t + j * L;
                qf[b][j] = mask4(Q[b * qs + (f < units ? f : 0)], f < units);
            }
    } else {
        for (int i = tid; i < NQ * LV; i += kBlock) {
            const int b = i / LV, f = i - b * LV;
            sq[i] = mask4(Q[b * qs + (f < units ? f : 0)], f < units);
        }
        __syncthreads();
    }

    const int64_t rows = tile.row_end - tile.row_begin;
    const int64_t per_wave = ((rows + 4 * R - 1) / (4 * R)) * R;
    const int64_t wb = tile.row_begin + wave * per_wave;
    const int64_t we = min(wb + per_wave, tile.row_end);
    const uint64_t* abits = p.accept ? p.accept[tile.seg] : nullptr;
    const int k = p.k;

    uint64_t lk[NQ], thr[NQ];
#pragma unroll
    for (int b = 0; b < NQ; ++b) { lk[b] = 0ull; thr[b] = 0ull; }
    uint32_t nvis = 0;

    walk_rows<R>(wb, we, abits, seg.ord_to_doc, lane, g, [&](const int64_t row, bool valid, bool accepted_known) {
        int32_t doc = 0;
        if (valid) {
            doc = seg.ord_to_doc ? seg.ord_to_doc[row] : (int32_t)row;
            if (abits && !accepted_known) valid = (abits[doc >> 6] >> (doc & 63)) & 1ull;
        }
        int4 xv[V];
        const int4* xr = X + row * units;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int f = t + j * L;
            xv[j] = (valid && f < units) ? xr[f] : make_int4(0, 0, 0, 0);
        }
        nvis += __popcll(__ballot(t == 0 && valid));

#pragma unroll
        for (int b = 0; b < NQ; ++b) {
            int acc = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int4 qv = QREG ? qf[QREG ? b : 0][QREG ? j : 0] : sq[b * LV + t + j * L];
                acc = ham_unit(xv[j], qv, acc);
            }
            acc = lane_sum<L>(acc);
            const uint64_t key = valid ? make_key(score_hamming(acc), (uint32_t)(seg.doc_base + doc)) : 0ull;
            wave_offer(key, t == 0, lk[b], thr[b], lane, k);
        }
    });

    if (p.visited && p.q0 == 0) add_visited_wg(&p.visited[tile.seg], (uint32_t)nvis);

#pragma unroll
    for (int b = 0; b < NQ; ++b) slist[(b * 4 + wave) * 64 + lane] = lane < k ? lk[b] : 0ull;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int b = 0; b < NQ; ++b) {
            block_fold(slist + b * 4 * 64, lk[b], thr[b], lane, k);
            if (b < p.q_count && lane < k)
                p.cand[((size_t)(p.q0 + b) * p.n_tiles + blockIdx.x) * k + lane] = lk[b];
        }
    }
}

template <int L, int V, int U>
__global__ __launch_bounds__(kBlock) void scan_ham_stream(HamParams p) {
    constexpr int R = 64 / L;
    __shared__ uint64_t slist[4 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform: scalar loop control
    const int t = L == 1 ? 0 : (lane & (L - 1)), g = lane / L;
    const TileDev tile = p.tiles[blockIdx.x];
    const SegDev seg = p.segs[tile.seg];
    const int4* __restrict__ X = static_cast<const int4*>(seg.rows);
    const int4* __restrict__ Q = static_cast<const int4*>(p.q);
    const int units = p.units;
    int4 qf[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int f = t + j * L;
        qf[j] = mask4(Q[f < units ? f : 0], f < units);
    }
    const int64_t rows = tile.row_end - tile.row_begin;
    const int64_t per_wave = ((rows + 4 * R - 1) / (4 * R)) * R;
    const int64_t wb = tile.row_begin + wave * per_wave;
    const int64_t we = min(wb + per_wave, tile.row_end);
    const int k = p.k;
    uint64_t lk = 0ull, thr = 0ull;
    uint32_t nvis = 0;
    for (int64_t r0 = wb; r0 < we; r0 += R * U) {
        int64_t row[U];
        bool valid[U];
        int4 xv[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            row[u] = r0 + u * R + g;
            valid[u] = row[u] < we;
            const int64_t rc = valid[u] ? row[u] : wb;   // clamped row: every load is unconditional
            const int4* xr = X + rc * units;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int f = t + j * L;
                xv[u][j] = mask4(load_i4_nt(xr + (f < units ? f : 0)), f < units);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int acc = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) acc = ham_unit(xv[u][j], qf[j], acc);
            acc = lane_sum<L>(acc);
            nvis += __popcll(__ballot(t == 0 && valid[u]));
            const int32_t doc = seg.ord_to_doc ? seg.ord_to_doc[valid[u] ? row[u] : wb] : (int32_t)row[u];
            const uint64_t key = valid[u] ? make_key(score_hamming(acc), (uint32_t)(seg.doc_base + doc)) : 0ull;
            wave_offer(key, t == 0, lk, thr, lane, k);
        }
    }
    if (p.visited && p.q0 == 0) add_visited_wg(&p.visited[tile.seg], (uint32_t)nvis);
    slist[wave * 64 + lane] = lane < k ? lk : 0ull;
    __syncthreads();
    if (wave == 0) {
        block_fold(slist, lk, thr, lane, k);
        if (lane < k) p.cand[((size_t)p.q0 * p.n_tiles + blockIdx.x) * k + lane] = lk;
    }
}

// The select path's writer: every row of the tile gets its key (0 = not accepted) at p.keys[view row]; lane
// t == 0 of a row's group stores it, so an iteration's R contiguous rows' keys go out together.
template <int L, int V, int U>
__global__ __launch_bounds__(kBlock) void sel_keys_ham(SelParams p) {
    constexpr int R = 64 / L;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform: scalar loop control
    const int t = L == 1 ? 0 : (lane & (L - 1)), g = lane / L;
    const TileDev tile = p.tiles[blockIdx.x];
    const SegDev seg = p.segs[tile.seg];
    const uint64_t* abits = p.accept ? p.accept[tile.seg] : nullptr;
    const int4* __restrict__ X = static_cast<const int4*>(seg.rows);
    const int4* __restrict__ Q = static_cast<const int4*>(p.q);
    const int units = p.units;
    int4 qf[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int f = t + j * L;
        qf[j] = mask4(Q[f < units ? f : 0], f < units);
    }
    const int64_t vbase = p.seg_vrow[tile.seg];
    const int64_t rows = tile.row_end - tile.row_begin;
    const int64_t per_wave = ((rows + 4 * R - 1) / (4 * R)) * R;
    const int64_t wb = tile.row_begin + wave * per_wave;
    const int64_t we = min(wb + per_wave, tile.row_end);
    uint32_t nvis = 0;
    for (int64_t r0 = wb; r0 < we; r0 += R * U) {
        int4 xv[U][V];
        int32_t doc[U];
        bool in[U], valid[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = r0 + u * R + g;
            in[u] = row < we;
            const int64_t rc = in[u] ? row : wb;
            doc[u] = seg.ord_to_doc ? seg.ord_to_doc[rc] : (int32_t)rc;
            valid[u] = in[u] && (!abits || ((abits[doc[u] >> 6] >> (doc[u] & 63)) & 1ull));
            const int4* xr = X + rc * units;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int f = t + j * L;
                xv[u][j] = mask4(load_i4_nt(xr + (f < units ? f : 0)), f < units);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int acc = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) acc = ham_unit(xv[u][j], qf[j], acc);
            acc = lane_sum<L>(acc);
            nvis += __popcll(__ballot(t == 0 && valid[u]));
            const uint64_t key = valid[u] ? make_key(score_hamming(acc), (uint32_t)(seg.doc_base + doc[u])) : 0ull;
            if (in[u] && t == 0) p.keys[vbase + r0 + u * R + g] = key;
        }
    }
    if (p.visited) add_visited_wg(&p.visited[tile.seg], (uint32_t)nvis);
}

using HamFn = void (*)(HamParams);
using SelFn = void (*)(SelParams);
constexpr int kHamCfgs = 10;
#define OSK_HAM_ROW(L, V) {scan_ham<L, V, 1>, scan_ham<L, V, 2>, scan_ham<L, V, 4>, scan_ham<L, V, 8>}
const HamFn kScanHam[kHamCfgs][4] = {OSK_HAM_ROW(1, 1),  OSK_HAM_ROW(2, 1),  OSK_HAM_ROW(4, 1),  OSK_HAM_ROW(8, 1),
                                     OSK_HAM_ROW(16, 1), OSK_HAM_ROW(16, 2), OSK_HAM_ROW(16, 3), OSK_HAM_ROW(16, 4),
                                     OSK_HAM_ROW(32, 4), OSK_HAM_ROW(64, 4)};
const HamFn kScanHamStream[kHamCfgs] = {scan_ham_stream<1, 1, 4>,  scan_ham_stream<2, 1, 4>,  scan_ham_stream<4, 1, 4>,
                                        scan_ham_stream<8, 1, 4>,  scan_ham_stream<16, 1, 4>, scan_ham_stream<16, 2, 4>,
                                        scan_ham_stream<16, 3, 4>, scan_ham_stream<16, 4, 4>, scan_ham_stream<32, 4, 4>,
                                        scan_ham_stream<64, 4, 4>};
const SelFn kSelKeysHam[kHamCfgs] = {sel_keys_ham<1, 1, 4>,  sel_keys_ham<2, 1, 4>,  sel_keys_ham<4, 1, 4>,
                                     sel_keys_ham<8, 1, 4>,  sel_keys_ham<16, 1, 4>, sel_keys_ham<16, 2, 4>,
                                     sel_keys_ham<16, 3, 4>, sel_keys_ham<16, 4, 4>, sel_keys_ham<32, 4, 4>,
                                     sel_keys_ham<64, 4, 4>};
constexpr int kHamLV[kHamCfgs][2] = {{1, 1}, {2, 1}, {4, 1}, {8, 1}, {16, 1}, {16, 2}, {16, 3}, {16, 4}, {32, 4}, {64, 4}};

// the lane config of a row of u units (the table in the file header); −1 = no config
int ham_cfg(int u) {
    if (u < 1 || u > 256) return -1;
    return u <= 1 ? 0 : u <= 2 ? 1 : u <= 4 ? 2 : u <= 8 ? 3 : u <= 16 ? 4 : u <= 32 ? 5 : u <= 48 ? 6 : u <= 64 ? 7
                                                                                             : u <= 128 ? 8 : 9;
}

}  // namespace

hipError_t launch_scan_ham(int nq, const HamParams& p, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop) {
    const int cfg = ham_cfg(p.units);
    if (cfg < 0 || nq < 1 || nq > kMaxNQ || p.q_count < 1 || p.q_count > nq || p.k < 1 || p.k > kScanMaxK ||
        p.n_tiles < 1 || p.q_units < p.units)
        return hipErrorInvalidValue;
    const int slot = nq <= 1 ? 0 : nq <= 2 ? 1 : nq <= 4 ? 2 : 3;
    const int NQ = 1 << slot;
    const int L = kHamLV[cfg][0], V = kHamLV[cfg][1];
    HamFn fn;
    size_t lds;
    if (NQ == 1 && !p.accept && g_tuning.ham_stream) {
        fn = kScanHamStream[cfg];
        lds = 0;
    } else {
        fn = kScanHam[cfg][slot];
        lds = (NQ * V * 4 <= 64 ? 0 : (size_t)NQ * L * V * 16) + (size_t)NQ * 4 * 64 * 8;
    }
    if (ev_start || ev_stop)
        hipExtLaunchKernelGGL(fn, dim3(p.n_tiles), dim3(kBlock), lds, s, ev_start, ev_stop, 0, p);
    else
        hipLaunchKernelGGL(fn, dim3(p.n_tiles), dim3(kBlock), lds, s, p);
    return hipGetLastError();
}

SelKeysFn sel_keys_ham_fn(int units) {
    const int cfg = ham_cfg(units);
    return cfg < 0 ? nullptr : kSelKeysHam[cfg];
}

}  // namespace osk
