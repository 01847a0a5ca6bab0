// osk_rowscore.h — the streaming scans' per-row arithmetic (scan_f32 / scan_i8's, operation for operation)
// as functions: the threshold kernels (osk_threshold.hip) and the nested k-NN kernels (osk_nested.hip) call
// these, so a row's score has the same bits in every one of them — and the bits of the k-NN scans.
#pragma once
#include "osk_device.h"
#include "osk_internal.h"
#include "osk_wave.h"

namespace osk {

template <bool NT>
__device__ __forceinline__ float4 thr_load4(const float4* p) {
    if constexpr (NT) {
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p));
        return make_float4(v.x, v.y, v.z, v.w);
    } else {
        return *p;
    }
}

template <int L, int V, bool NT>
__device__ __forceinline__ void thr_load_row_f32(const float4* xr, bool valid, int units, int t, float4 (&xv)[V]) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int f = t + j * L;
        xv[j] = (valid && f < units) ? thr_load4<NT>(xr + f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// |q|² in the row norms' lane layout (COSINE)
template <int L, int V, class QAt>
__device__ __forceinline__ float thr_qnorm_f32(QAt&& qat) {
    float ax = 0.f, ay = 0.f, az = 0.f, aw = 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float4 qv = qat(j);
        ax = fmaf(qv.x, qv.x, ax); ay = fmaf(qv.y, qv.y, ay);
        az = fmaf(qv.z, qv.z, az); aw = fmaf(qv.w, qv.w, aw);
    }
    float s = (ax + ay) + (az + aw);
    return lane_sum<L>(s);
}

template <int L, int V, bool L2K, class QAt>
__device__ __forceinline__ float thr_score_f32(const float4 (&xv)[V], QAt&& qat, int sim, float qn, float xn) {
    float ax = 0.f, ay = 0.f, az = 0.f, aw = 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float4 qv = qat(j);
        if constexpr (L2K) {
            const float dx = xv[j].x - qv.x, dy = xv[j].y - qv.y;
            const float dz = xv[j].z - qv.z, dw = xv[j].w - qv.w;
            ax = fmaf(dx, dx, ax); ay = fmaf(dy, dy, ay);
            az = fmaf(dz, dz, az); aw = fmaf(dw, dw, aw);
        } else {
            ax = fmaf(xv[j].x, qv.x, ax); ay = fmaf(xv[j].y, qv.y, ay);
            az = fmaf(xv[j].z, qv.z, az); aw = fmaf(xv[j].w, qv.w, aw);
        }
    }
    float s = (ax + ay) + (az + aw);
    s = lane_sum<L>(s);
    if constexpr (L2K) return score_f32_l2(s);
    else return score_f32(sim, s, qn, xn);
}

__device__ __forceinline__ int thr_dot4(int a, int b, int c) { return __builtin_amdgcn_sdot4(a, b, c, false); }

template <int L, int V>
__device__ __forceinline__ void thr_load_row_i8(const int4* xr, bool valid, int units, int t, int4 (&xv)[V]) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int f = t + j * L;
        xv[j] = (valid && f < units) ? xr[f] : make_int4(0, 0, 0, 0);
    }
}

template <int L, int V, class QAt>
__device__ __forceinline__ int32_t thr_qnorm_i8(QAt&& qat) {   // Σq² (exact)
    int acc = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int4 qv = qat(j);
        acc = thr_dot4(qv.x, qv.x, acc); acc = thr_dot4(qv.y, qv.y, acc);
        acc = thr_dot4(qv.z, qv.z, acc); acc = thr_dot4(qv.w, qv.w, acc);
    }
    return lane_sum<L>(acc);
}

template <int L, int V, class QAt>
__device__ __forceinline__ float thr_score_i8(const int4 (&xv)[V], QAt&& qat, int sim, int32_t qn, int32_t xn, int dim) {
    int acc = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int4 qv = qat(j);
        acc = thr_dot4(xv[j].x, qv.x, acc);
        acc = thr_dot4(xv[j].y, qv.y, acc);
        acc = thr_dot4(xv[j].z, qv.z, acc);
        acc = thr_dot4(xv[j].w, qv.w, acc);
    }
    acc = lane_sum<L>(acc);
    const int32_t s = sim == SIM_EUCLIDEAN ? qn + xn - 2 * acc : acc;
    return score_i8(sim, s, qn, xn, dim);
}

// A wave's rows of a tile (the k-NN scans' split: 4 waves, each a multiple of R rows)
template <int R>
__device__ __forceinline__ void thr_wave_range(const TileDev& tile, int wave, int64_t& wb, int64_t& we) {
    const int64_t rows = tile.row_end - tile.row_begin;
    const int64_t per_wave = ((rows + 4 * R - 1) / (4 * R)) * R;
    wb = min(tile.row_begin + wave * per_wave, tile.row_end);
    we = min(wb + per_wave, tile.row_end);
}
// ...the same split for a kernel that walks the rows in another lane config than the one whose R splits
// the tile (thr_scan_sq8: the int8 configs' R differs from the float32 config's)
__device__ __forceinline__ void thr_wave_range_rt(const TileDev& tile, int wave, int R, int64_t& wb, int64_t& we) {
    const int64_t rows = tile.row_end - tile.row_begin;
    const int64_t per_wave = ((rows + 4 * R - 1) / (4 * R)) * R;
    wb = min(tile.row_begin + wave * per_wave, tile.row_end);
    we = min(wb + per_wave, tile.row_end);
}

}  // namespace osk
