// osk_derived.hip — the lifetime of the object model (osk_seg, osk_view: osk_objects.h) and the structures
// built once per segment or view: a segment's rows, norms and derived copies (the int8 prefilter copy, its
// tiled and group-scaled twins, the 6-bit tier, the bf16 hi/lo split), a view's pointer tables, MFMA units,
// wide tiles, settle slices, gather tiles and nested tables.  Every builder allocates into local DevBufs and
// stores into the object only after its last step that can fail, so an early return frees what it built.
// Nothing here depends on the C-ABI (osk_api.hip) or has an OSK_TESTING variant.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "osk_objects.h"

using namespace osk;

osk_seg::~osk_seg() {
    if (self_view) delete self_view;   // holds no reference on this segment
    // Wait for the device before anything goes: the members free themselves after this body, and both steps
    // below need every launch that reads the segment to have completed.
    int cur = -1;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    // the 6-bit copy: stream-ordered pool allocations (ensure_sq8_seg); nothing reads them any more
    if (d_q6) (void)hipFreeAsync(d_q6, nullptr);
    if (d_q6aux) (void)hipFreeAsync(d_q6aux, nullptr);
    if (d_q6 || d_q6aux) (void)hipStreamSynchronize(nullptr);
    if (cur >= 0) (void)hipSetDevice(cur);
    sq6_forget_segment(this);   // (a later segment at this address must not wait on this one's launches)
}

int64_t osk_seg::hbm_bytes() const {
    int64_t b = 0;
    for (const DevBuf* d : {&d_rows, &d_xnorm_f, &d_xnorm_i, &d_ord_to_doc, &d_split, &d_maxnorm2, &d_xsqrt, &d_q8,
                            &d_q8aux, &d_q8t, &d_q8w, &d_q8auxt, &d_row_parent})
        b += (int64_t)d->cap;
    if (d_q6) b += sq6_bytes(n_rows, dim);
    return b;
}

osk_view::~osk_view() {
    for (osk_view* r : replicas) delete r;   // (no lease is live: the caller's release contract)
    sq6_share_detach(this);   // (waits for the group's scans: they may be writing this view's lists)
    for (hipStream_t st : lease_streams)
        if (st) (void)hipStreamDestroy(st);
    if (xs_event) (void)hipEventDestroy(xs_event);
    if (ev_probe) {   // a calibration read-back may still be landing in h_seg_rebound
        if (probe_pending) (void)hipEventSynchronize(ev_probe);
        (void)hipEventDestroy(ev_probe);
    }
    for (hipEvent_t e : ev_call)
        if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < kEvRing; ++i) {
        if (ev_start[i]) (void)hipEventDestroy(ev_start[i]);
        if (ev_stop[i]) (void)hipEventDestroy(ev_stop[i]);
    }
    if (holds_refs)
        for (osk_seg* s : segs) osk::seg_unref(s);
}

void osk::seg_unref(osk_seg* s) {
    if (s && s->refs.fetch_sub(1) == 1) {
        (void)hipSetDevice(s->device);
        delete s;
    }
}

namespace osk {

// The device view of a view's segments (pointers re-read: staging may add row norms later).
std::vector<SegDev> seg_devs(const osk_view* v) {
    std::vector<SegDev> sd(v->segs.size());
    for (size_t i = 0; i < v->segs.size(); ++i) {
        const osk_seg* s = v->segs[i];
        sd[i] = SegDev{s->d_rows.p, s->d_xnorm_f.as<float>(), s->d_xnorm_i.as<int32_t>(),
                       s->d_ord_to_doc.as<int32_t>(), s->n_rows, v->seg_doc_base[i], v->seg_shard[i]};
    }
    return sd;
}

// The rest of staging once the rows are on the device: row norms, ord→doc map, the int8 prefilter copy.
int32_t seg_finish(osk_seg* s, const int32_t* ord_to_doc, hipStream_t st) {
    const size_t n = (size_t)std::max<int64_t>(1, s->n_rows);
    DevBuf xnorm_f, xnorm_i, o2d;
    // row norms
    if (s->enc == ENC_FLOAT32 && s->sim == SIM_COSINE) {
        OSK_HIP(xnorm_f.reserve(n * sizeof(float)));
        if (s->n_rows > 0)
            OSK_HIP(launch_row_norms_f32(s->d_rows.as<const float4>(), s->n_rows, s->units, s->cfg,
                                         xnorm_f.as<float>(), st));
    }
    // (a Hamming segment keeps no Σx²: its kernels have no use for it, and 4 B per row is a quarter of a 128-bit row)
    if (s->enc == ENC_BYTE && s->sim != SIM_HAMMING) {
        OSK_HIP(xnorm_i.reserve(n * sizeof(int32_t)));
        if (s->n_rows > 0)
            OSK_HIP(launch_row_norms_i8(s->d_rows.as<const int4>(), s->n_rows, s->units, xnorm_i.as<int32_t>(), st));
    }
    if (ord_to_doc) {
        for (int64_t i = 0; i < s->n_rows; ++i) {
            if (ord_to_doc[i] < 0 || ord_to_doc[i] >= s->max_doc ||
                (i > 0 && ord_to_doc[i] <= ord_to_doc[i - 1])) {
                set_error("ord_to_doc must be strictly ascending docIDs in [0, max_doc)");
                return OSK_ERR_INVALID;
            }
        }
        OSK_HIP(o2d.reserve(n * sizeof(int32_t)));
        OSK_HIP(hipMemcpyAsync(o2d.p, ord_to_doc, s->n_rows * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    OSK_HIP(hipStreamSynchronize(st));
    s->d_xnorm_f = std::move(xnorm_f);
    s->d_xnorm_i = std::move(xnorm_i);
    s->d_ord_to_doc = std::move(o2d);
    // the certified int8 prefilter copy is the default path of float32 searches: built with the segment
    // (staging = the reader's constructor / warmer, S/index/engine/InternalEngine.java:2409-2432), so
    // no search pays for it and the segment's HBM footprint is known at staging
    if (s->enc == ENC_FLOAT32) return ensure_sq8_seg(s, st);
    return OSK_OK;
}

// A new segment with its padded rows allocated (arguments checked; the device made current).
int32_t seg_alloc(int device, int64_t n_rows, int dim, int enc, int sim, int max_doc,
                  const int32_t* ord_to_doc, std::unique_ptr<osk_seg>& out) {
    OSK_REQUIRE(n_rows >= 0, "n_rows must be >= 0");
    OSK_REQUIRE(dim >= 1 && dim <= OSK_MAX_DIM, "dim must be in [1, 4096]");
    OSK_REQUIRE(enc == ENC_FLOAT32 || enc == ENC_BYTE, "unknown encoding");
    OSK_REQUIRE(sim >= 0 && sim <= SIM_HAMMING, "unknown similarity");
    OSK_REQUIRE(sim != SIM_HAMMING || enc == ENC_BYTE,
                "hamming similarity needs a byte field: OSK_HAMMING is served for OSK_BYTE (packed bits) only");
    OSK_REQUIRE(n_rows <= 0x7FFFFFFFll, "a Lucene segment holds < 2^31 docs");
    if (ord_to_doc == nullptr) OSK_REQUIRE(max_doc >= n_rows, "max_doc < n_rows for a dense field");
    int32_t rc = check_device(device);
    if (rc) return rc;
    const int units = units_for(dim, enc);
    DevBuf rows;
    hipError_t e = rows.reserve((size_t)std::max<int64_t>(1, n_rows) * units * 16);
    if (e != hipSuccess) {
        set_error(std::string("hipMalloc of segment rows failed: ") + hipGetErrorString(e));
        return OSK_ERR_OOM;
    }
    auto s = std::make_unique<osk_seg>();
    s->device = device;
    s->n_rows = n_rows;
    s->dim = dim;
    s->enc = enc;
    s->sim = sim;
    s->max_doc = max_doc;
    s->units = units;
    s->cfg = cfg_index(units);
    s->d_rows = std::move(rows);
    out = std::move(s);
    return OSK_OK;
}

// the device's CUs (cached; the persistent kernels' grids and the wide tile table are sized by them)
int view_cus(osk_view* v) {
    if (v->n_cus <= 0 &&
        (hipDeviceGetAttribute(&v->n_cus, hipDeviceAttributeMultiprocessorCount, v->device) != hipSuccess ||
         v->n_cus <= 0))
        v->n_cus = 256;
    return v->n_cus;
}

// The view's tables of the nested search (caller holds v->mu): every segment's row→parent table and its
// parent-slot base — segments in the tile table's order (by shard, then segment), so a shard's parent slots
// are contiguous — and the parent tiles: runs of ≤ kNestPtile slots of one shard.  Built once.
int32_t ensure_nested(osk_view* v, hipStream_t st) {
    if (v->nest_ready) return OSK_OK;
    const int ns = (int)v->segs.size(), S = v->n_shards;
    std::vector<NestSeg> nsegs(ns);
    std::vector<NestPtile> ptiles;
    std::vector<int32_t> spb(S + 1, 0);
    int64_t slots = 0;
    for (int sh = 0; sh < S; ++sh) {
        spb[sh] = (int32_t)ptiles.size();
        const int64_t first = slots;
        for (int i = 0; i < ns; ++i) {
            if (v->seg_shard[i] != sh) continue;
            osk_seg* sg = v->segs[i];
            std::lock_guard<std::mutex> lk(sg->mu);
            OSK_REQUIRE(sg->n_parents > 0 && sg->d_row_parent.p != nullptr,
                        "nested search: a segment of the view has no parents registered (osk_seg_set_parents)");
            nsegs[i] = NestSeg{sg->d_row_parent.as<int32_t>(), slots};
            slots += sg->n_parents;
        }
        for (int64_t b = first; b < slots; b += kNestPtile)
            ptiles.push_back(NestPtile{b, std::min<int64_t>(b + kNestPtile, slots)});
    }
    spb[S] = (int32_t)ptiles.size();
    OSK_REQUIRE(ptiles.size() < (size_t)(1 << 24), "too many parent tiles");
    OSK_HIP(v->d_nest_segs.upload(nsegs, st));
    OSK_HIP(v->d_ptiles.upload(ptiles, st));
    OSK_HIP(v->d_shard_ptile_begin.upload(spb, st));
    OSK_HIP(hipStreamSynchronize(st));   // the sources are locals
    v->nest_parents = slots;
    v->n_ptiles = (int)ptiles.size();
    v->nest_ready = true;
    return OSK_OK;
}

// The segment's bf16 hi/lo copy in MFMA fragment order (+ |x|² rows and their max).  Built once.
int32_t ensure_split(osk_seg* s, hipStream_t st) {
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->d_split.p) return OSK_OK;
    const int KS = ((s->units + 7) / 8 + kKsAlign - 1) / kKsAlign * kKsAlign;   // 32-dim K-steps (padded)
    const int64_t n_tiles = (s->n_rows + 127) / 128;        // 128-row tiles
    const int64_t n_rb = std::max<int64_t>(1, n_tiles) * 8;
    const size_t n = (size_t)std::max<int64_t>(1, s->n_rows);
    DevBuf xnorm, split, xsqrt, maxnorm2;
    const float* xn = s->d_xnorm_f.as<float>();   // the segment's row norms, or (none yet) the ones built here
    if (!xn) {
        OSK_HIP(xnorm.reserve(n * sizeof(float)));
        if (s->n_rows > 0)
            OSK_HIP(launch_row_norms_f32(s->d_rows.as<const float4>(), s->n_rows, s->units, s->cfg,
                                         xnorm.as<float>(), st));
        xn = xnorm.as<float>();
    }
    hipError_t e = split.reserve((size_t)n_rb * KS * 2 * 1024);
    if (e != hipSuccess) {
        set_error(std::string("hipMalloc of the MFMA split copy failed: ") + hipGetErrorString(e));
        return OSK_ERR_OOM;
    }
    OSK_HIP(launch_split_rows(s->d_rows.as<const float4>(), s->n_rows, s->units, KS, n_rb, split.p, st));
    OSK_HIP(xsqrt.reserve(n * sizeof(float)));
    if (s->n_rows > 0) OSK_HIP(launch_row_sqrt(xn, s->n_rows, xsqrt.as<float>(), st));
    OSK_HIP(maxnorm2.reserve(sizeof(unsigned)));
    OSK_HIP(hipMemsetAsync(maxnorm2.p, 0, sizeof(unsigned), st));
    if (s->n_rows > 0) OSK_HIP(launch_max_norm2(xn, s->n_rows, maxnorm2.as<unsigned>(), st));
    unsigned bits = 0;
    OSK_HIP(hipMemcpyAsync(&bits, maxnorm2.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    OSK_HIP(hipStreamSynchronize(st));
    if (xnorm.p) s->d_xnorm_f = std::move(xnorm);
    s->d_split = std::move(split);
    s->d_xsqrt = std::move(xsqrt);
    s->d_maxnorm2 = std::move(maxnorm2);
    std::memcpy(&s->h_maxnorm2, &bits, 4);
    s->split_KS = KS;
    return OSK_OK;
}

// MFMA work units (runs of 128-row tiles, contiguous per shard) and per-shard bounds.  Built once.
int32_t ensure_mfma(osk_view* v, hipStream_t st) {
    if (v->mfma_ready) return OSK_OK;
    const int ns = (int)v->segs.size();
    std::vector<const void*> splits(ns);
    std::vector<const float*> xsq(ns);
    std::vector<int64_t> vrow(ns);
    int64_t acc = 0, total_tiles = 0;
    for (int i = 0; i < ns; ++i) {
        int32_t rc = ensure_split(v->segs[i], st);
        if (rc) return rc;
        splits[i] = v->segs[i]->d_split.p;
        xsq[i] = v->segs[i]->d_xsqrt.as<float>();
        vrow[i] = acc;
        acc += v->segs[i]->n_rows;
        total_tiles += (v->segs[i]->n_rows + 127) / 128;
    }
    OSK_REQUIRE(acc < 0xFFFFFFFFll, "a view holds < 2^32 rows");
    {   // ensure_split may have added row norms: refresh the device segment table
        const std::vector<SegDev> sd = seg_devs(v);
        OSK_HIP(v->d_segs.upload(sd, st));
    }
    // auto: one workgroup per CU (1 per CU fits: 255 VGPRs, 143 KiB LDS) in 1 round below 16k tiles
    // (C2 b256: 0.74 → 0.65 ms, fewer pilot tiles), else 2 rounds (C3 b256: 11.6 ms against 11.7;
    // 384 units, 1.5 rounds, lose 30 %; profiles/r02q/mfma_units.txt)
    const int64_t target = g_tuning.mfma_units > 0 ? (int64_t)g_tuning.mfma_units : (total_tiles < 16384 ? 256 : 512);
    const int64_t per = std::max<int64_t>(1, (total_tiles + target - 1) / target);
    std::vector<MfmaUnit> units;
    std::vector<int32_t> shard_list_begin(v->n_shards + 1, 0);
    std::vector<float> shard_max(v->n_shards, 0.0f);
    for (int sh = 0; sh < v->n_shards; ++sh) {
        shard_list_begin[sh] = (int32_t)units.size() * 2;
        for (int i = 0; i < ns; ++i) {
            if (v->seg_shard[i] != sh) continue;
            shard_max[sh] = std::max(shard_max[sh], v->segs[i]->h_maxnorm2);
            const int64_t nt = (v->segs[i]->n_rows + 127) / 128;
            for (int64_t t = 0; t < nt; t += per)
                units.push_back(MfmaUnit{i, sh, t, std::min(nt, t + per), vrow[i]});
        }
    }
    shard_list_begin[v->n_shards] = (int32_t)units.size() * 2;
    v->n_munits = (int)units.size();
    OSK_REQUIRE(v->n_munits > 0 && v->n_munits < 65536, "bad MFMA unit count");
    v->mfma_KS = ((v->units + 7) / 8 + kKsAlign - 1) / kKsAlign * kKsAlign;
    // |Σ approx − Σ device order| ≤ c·|x||q|: bf16 split (3·2^-16) + fp32 accumulation of the
    // 3·Kpad MFMA products and of the Kpad device-order products (γ_n ≈ n·2^-24), ×1.5 margin.
    const double kpad = 32.0 * v->mfma_KS;
    v->mfma_c = 1.5 * (3.0 * std::ldexp(1.0, -16) + 4.0 * kpad * std::ldexp(1.0, -24));
    OSK_HIP(v->d_munits.upload(units, st));
    OSK_HIP(v->d_seg_split.upload(splits, st));
    OSK_HIP(v->d_seg_xsqrt.upload(xsq, st));
    OSK_HIP(v->d_shard_unit_begin.upload(shard_list_begin, st));
    OSK_HIP(v->d_shard_maxnorm2.upload(shard_max, st));
    OSK_HIP(hipStreamSynchronize(st));
    v->mfma_ready = true;
    return OSK_OK;
}

// The segment's int8 copy + per-row bound terms for the certified prefilter.  Built once.
int32_t ensure_sq8_seg(osk_seg* s, hipStream_t st) {
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->d_q8.p) return OSK_OK;
    const int u8 = (s->dim + 15) / 16;
    const size_t n = (size_t)std::max<int64_t>(1, s->n_rows);
    DevBuf q8, aux, d_oor;
    hipError_t e = q8.reserve(n * u8 * 16);
    if (e != hipSuccess) {
        set_error(std::string("hipMalloc of the int8 prefilter copy failed: ") + hipGetErrorString(e));
        return OSK_ERR_OOM;
    }
    e = aux.reserve(n * sizeof(float4));
    if (e != hipSuccess) {
        set_error(std::string("hipMalloc of the prefilter bound terms failed: ") + hipGetErrorString(e));
        return OSK_ERR_OOM;
    }
    // (the kernel also reports whether some row lies outside the certificate's range: one int, read below)
    OSK_HIP(d_oor.reserve(sizeof(int)));
    OSK_HIP(hipMemsetAsync(d_oor.p, 0, sizeof(int), st));
    OSK_HIP(launch_sq8_quantize(s->d_rows.as<const float4>(), s->n_rows, s->units, s->units, u8, q8.p,
                                aux.as<float4>(), 0, st, d_oor.as<int>()));
    // the 6-bit tier of single queries, where the dim has one and the tier is on (a node
    // that sets tune sq6 = 0 before staging never holds the copy; calibration frees it per segment)
    void* q6 = nullptr;
    float4* aux6 = nullptr;
    int oor = 0;
    // (the pool allocations have no owner until the segment takes them: the steps from the first of them to
    // the last that can fail run in a lambda, and leaving it early gives them back)
    const int32_t rc = [&]() -> int32_t {
        if (sq6_supported(s->dim) && g_tuning.sq6.load(std::memory_order_relaxed)) {
            // (stream-ordered allocations: the calibration frees them with hipFreeAsync behind the events of the
            // launches that read them, no device-wide wait — fold_probe)
            const int64_t b6 = sq6_bytes(s->n_rows, s->dim), ba = std::max<int64_t>(1, s->n_rows) * 16;
            e = hipMallocAsync(&q6, (size_t)(b6 - ba), st);
            if (e == hipSuccess) e = hipMallocAsync(reinterpret_cast<void**>(&aux6), (size_t)ba, st);
            if (e != hipSuccess) {
                set_error(std::string("hipMalloc of the 6-bit prefilter tier failed: ") + hipGetErrorString(e));
                return OSK_ERR_OOM;
            }
            OSK_HIP(launch_sq6_quantize(s->d_rows.as<const float4>(), s->n_rows, s->units, s->dim, q6, aux6, st));
        }
        OSK_HIP(hipStreamSynchronize(st));
        OSK_HIP(hipMemcpy(&oor, d_oor.p, sizeof(int), hipMemcpyDeviceToHost));
        return OSK_OK;
    }();
    if (rc) {
        if (q6) (void)hipFreeAsync(q6, st);
        if (aux6) (void)hipFreeAsync(aux6, st);
        (void)hipStreamSynchronize(st);
        return rc;
    }
    s->d_q8 = std::move(q8);
    s->d_q8aux = std::move(aux);
    s->d_q6 = q6;
    s->d_q6aux = aux6;
    s->sq8_out_of_range = oor != 0;
    s->units8 = u8;
    return OSK_OK;
}

// The segment's int8 copy in sq8_mfma's tiled layout: blocks of 16 rows, per 64-dim k-step one
// contiguous 1 KiB slab (chunk-major: 16-dim chunk c of row r at c·256 + r·16 B), so each of the scan's
// load instructions reads 1 KiB contiguous and a 32-dim tail is the slab's first 512 B.  Built once, from
// the row-major int8 copy.
int32_t ensure_sq8t_seg(osk_seg* s, hipStream_t st, bool wide) {
    std::lock_guard<std::mutex> lk(s->mu);
    const int u8 = (s->dim + 15) / 16;
    const int64_t blocks = std::max<int64_t>(1, (s->n_rows + 15) / 16);
    if (!s->d_q8t.p) {
        const int ks = sq8_mfma_ks(u8);
        DevBuf q8t;
        hipError_t e = q8t.reserve((size_t)blocks * ks * 1024);
        if (e != hipSuccess) {
            set_error(std::string("hipMalloc of the tiled int8 copy failed: ") + hipGetErrorString(e));
            return OSK_ERR_OOM;
        }
        OSK_HIP(launch_sq8_tile(s->d_q8.p, s->n_rows, u8, ks, q8t.p, st));
        OSK_HIP(hipStreamSynchronize(st));
        s->d_q8t = std::move(q8t);
    }
    // the wide kernel's own copy (osk_sq8w.hip launch_sq8w_build): codes with one scale per 16-row group,
    // tiled, and their bound terms per group (352 B per 16 rows).  Built the first time the cost model sends a
    // batch of this segment's view to the wide kernel (a node whose batches never take it does not
    // hold a second int8 copy — at 768 dims +768 B per row)
    if (wide && !s->d_q8w.p && sq8_wide_supported(u8)) {
        DevBuf q8w, auxt;
        hipError_t e = q8w.reserve((size_t)blocks * sq8_wide_ks(u8) * 1024);
        if (e == hipSuccess) e = auxt.reserve((size_t)blocks * kAuxGroupF4 * sizeof(float4));
        if (e != hipSuccess) {
            set_error(std::string("hipMalloc of the wide prefilter copy failed: ") + hipGetErrorString(e));
            return OSK_ERR_OOM;
        }
        OSK_HIP(launch_sq8w_build(s->d_rows.as<const float4>(), s->n_rows, s->units, u8,
                                  s->sim == SIM_COSINE ? s->d_xnorm_f.as<float>() : nullptr,
                                  s->sim == SIM_COSINE ? 1 : 0, q8w.p, auxt.as<float4>(), st));
        OSK_HIP(hipStreamSynchronize(st));
        s->d_q8w = std::move(q8w);
        s->d_q8auxt = std::move(auxt);
    }
    return OSK_OK;
}

int32_t ensure_sq8t(osk_view* v, hipStream_t st) {
    if (v->sq8t_ready) return OSK_OK;
    const int ns = (int)v->segs.size();
    std::vector<const void*> rows(ns);
    for (int i = 0; i < ns; ++i) {
        int32_t rc = ensure_sq8t_seg(v->segs[i], st, false);
        if (rc) return rc;
        rows[i] = v->segs[i]->d_q8t.p;
    }
    OSK_HIP(v->d_sq8_rows_t.upload(rows, st));
    OSK_HIP(hipStreamSynchronize(st));
    v->sq8t_ready = true;
    return OSK_OK;
}

// The wide kernel's inputs for a view (first batch the cost model sends to it): every segment's group-scaled
// copy and tiled bound terms, and the view's own tile table of quarters.
int32_t ensure_sq8w(osk_view* v, hipStream_t st) {
    if (v->sq8w_ready) return OSK_OK;
    int32_t rc = ensure_sq8t(v, st);
    if (rc) return rc;
    const int ns = (int)v->segs.size();
    std::vector<const void*> rows_w(ns), auxt(ns);
    for (int i = 0; i < ns; ++i) {
        rc = ensure_sq8t_seg(v->segs[i], st, true);
        if (rc) return rc;
        rows_w[i] = v->segs[i]->d_q8w.p;
        auxt[i] = v->segs[i]->d_q8auxt.p;
    }
    OSK_HIP(v->d_sq8_rows_w.upload(rows_w, st));
    OSK_HIP(v->d_sq8_auxt.upload(auxt, st));
    if (sq8_wide_supported((v->segs.empty() ? 0 : v->segs[0]->units8)) && v->n_tiles > 0) {
        // The wide kernel's own tiles: its lists are per (tile, quarter) and every quarter's lists are
        // written for all 256 queries, so quarters of the scan tiles (≈ 244 rows at C2) would make the list
        // traffic rival the corpus.  Quarters here hold ≈ R / (2·CUs) rows, 256 … 16,384 (C2 ≈ 2k, C4 16k;
        // two to a few dozen per persistent workgroup), tiles never span segments, cut at multiples of 16.
        const int cus = view_cus(v);
        double R = 0.0;
        for (const osk_seg* sg : v->segs) R += (double)sg->n_rows;
        // (≥ 512 dims: quarters of R / (8·CUs), so the first pass — one round of the persistent grid — covers
        // 1/8 of the rows, not 1/2, and the second pass's floors come early; list traffic is small beside
        // rows of ≥ 512 B)
        const int u8w = v->segs.empty() ? 1 : v->segs[0]->units8;
        const int qdiv = sq8_wide_ks(u8w) >= 8 ? 8 : 2;
        // (≤ 16,384 rows, round 5's best for the ring kernel; the rows kernel ran C4 b1024 in 16.05 ms at 32,768
        // against 16.42 (profiles/r06/tune14.jsonl) but a first-pass quarter that long can fill a queue: one C4
        // query in 256 took an exact re-scan, profiles/r06/rows_clocks_c4_b256_q32768.log)
        const int64_t qmax = 16384;
        const int64_t qr = g_tuning.sq8_wide_quarter_rows > 0
                               ? std::max<int64_t>(16, (int64_t)g_tuning.sq8_wide_quarter_rows & ~15ll)
                               : std::min<int64_t>(qmax, std::max<int64_t>(256, (int64_t)(R / ((double)qdiv * cus)) + 15 & ~15ll));
        const int64_t trows = 4 * qr;
        std::vector<TileDev> wt;
        v->wshard_tile_begin.assign(v->n_shards + 1, 0);
        for (int sh = 0; sh < v->n_shards; ++sh) {
            v->wshard_tile_begin[sh] = (int32_t)wt.size();
            for (int i = 0; i < ns; ++i) {
                if ((v->seg_shard.empty() ? 0 : v->seg_shard[i]) != sh) continue;
                const int64_t n = v->segs[i]->n_rows;
                if (n == 0) continue;
                const int64_t nt = (n + trows - 1) / trows;
                auto cut = [&](int64_t t) { return t >= nt ? n : (n * t / nt) & ~(int64_t)15; };
                for (int64_t t = 0; t < nt; ++t)
                    if (cut(t + 1) > cut(t)) wt.push_back(TileDev{i, sh, cut(t), cut(t + 1)});
            }
        }
        v->wshard_tile_begin[v->n_shards] = (int32_t)wt.size();
        v->n_wtiles = (int)wt.size();
        std::vector<int32_t> order(std::max<size_t>(1, wt.size()), 0), sqb(v->n_shards + 1);
        {   // interleaved over shards (as the scan tiles' order)
            std::vector<std::pair<double, int>> key;
            for (int sh = 0; sh < v->n_shards; ++sh) {
                const int t0 = v->wshard_tile_begin[sh], n = v->wshard_tile_begin[sh + 1] - t0;
                for (int j = 0; j < n; ++j) key.push_back({(j + 0.5) / n, t0 + j});
            }
            std::stable_sort(key.begin(), key.end(), [](auto& a, auto& b) { return a.first < b.first; });
            for (size_t i = 0; i < key.size(); ++i) order[i] = key[i].second;
        }
        for (int i = 0; i <= v->n_shards; ++i) sqb[i] = 4 * v->wshard_tile_begin[i];
        OSK_HIP(v->d_wtiles.upload(wt, st));
        OSK_HIP(v->d_wtile_order.upload(order, st));
        OSK_HIP(v->d_wshard_tile_begin.upload(v->wshard_tile_begin, st));
        OSK_HIP(v->d_shard_quarter_begin.upload(sqb, st));
        OSK_HIP(v->d_quarter_bm.reserve(sizeof(float4) * 4 * std::max<size_t>(1, wt.size())));
        OSK_HIP(launch_wide_quarter_max(v->d_wtiles.as<TileDev>(), v->n_wtiles, v->d_sq8_auxt.as<const float4*>(),
                                        v->d_quarter_bm.as<float4>(), st));
        // the quarters' descriptors, read by every workgroup's setup instead of recomputed (64 B each)
        OSK_HIP(v->d_wqtable.reserve((size_t)64 * 4 * std::max<size_t>(1, wt.size())));
        OSK_HIP(launch_wide_quarter_table(v->d_wtiles.as<TileDev>(), v->d_wtile_order.as<int32_t>(), 4 * v->n_wtiles,
                                          sq8_wide_ks(u8w), v->d_sq8_rows_w.p, v->d_sq8_auxt.p,
                                          v->d_seg_vrow.as<int64_t>(), v->d_quarter_bm.as<const float4>(),
                                          v->d_wqtable.p, st));
    }
    OSK_HIP(hipStreamSynchronize(st));
    v->sq8w_ready = true;
    return OSK_OK;
}

// Settle slices over the wave lists of a tile table (list = tile·4 + wave): kSliceLists lists each,
// never spanning shards (an empty shard gets one empty slice so its result is still written); each
// slice carries its L group (aligned chunks of kLGroupLists lists of the shard).
void settle_slices(const std::vector<int32_t>& shard_tile_begin, std::vector<int4>& sl, std::vector<int32_t>& ssb) {
    const int S = (int)shard_tile_begin.size() - 1;
    sl.clear();
    ssb.assign(S + 1, 0);
    for (int sh = 0; sh < S; ++sh) {
        ssb[sh] = (int32_t)sl.size();
        const int l0 = 4 * shard_tile_begin[sh], l1 = 4 * shard_tile_begin[sh + 1];
        if (l0 == l1) sl.push_back(make_int4(l0, l0, l0, l0));
        for (int l = l0; l < l1; l += kSliceLists) {
            const int ga = l0 + (l - l0) / kLGroupLists * kLGroupLists;
            sl.push_back(make_int4(l, std::min(l + kSliceLists, l1), ga, std::min(ga + kLGroupLists, l1)));
        }
    }
    ssb[S] = (int32_t)sl.size();
}

// Gather tiles for filtered scans over the compacted accepted ordinals (osk_filter.hip): one round of
// the chip's resident scan workgroups (CUs × 4) split over the segments by rows, at least one per
// non-empty segment, ordered by shard like the row tiles (so lists never span shards); gather tile
// j of nj of a segment covers ordinals [cnt·j/nj, cnt·(j+1)/nj) of its cnt accepted ones.  Built once.
int32_t ensure_gather(osk_view* v, hipStream_t st) {
    if (v->gather_ready) return OSK_OK;
    const int ns = (int)v->segs.size();
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, v->device) != hipSuccess || cus <= 0)
        cus = 256;
    const int64_t target = std::min<int64_t>((int64_t)cus * 4, std::max(1, v->n_tiles));
    int64_t total = 0;
    for (osk_seg* sg : v->segs) total += sg->n_rows;
    std::vector<int4> gt;
    std::vector<int32_t> gsb(v->n_shards + 1, 0);
    for (int sh = 0; sh < v->n_shards; ++sh) {
        gsb[sh] = (int32_t)gt.size();
        for (int i = 0; i < ns; ++i) {
            if (v->seg_shard[i] != sh || v->segs[i]->n_rows == 0) continue;
            const int64_t nj = std::max<int64_t>(1, (int64_t)((double)v->segs[i]->n_rows * target / std::max<int64_t>(1, total)));
            for (int64_t j = 0; j < nj; ++j) gt.push_back(make_int4(i, sh, (int)j, (int)nj));
        }
    }
    gsb[v->n_shards] = (int32_t)gt.size();
    std::vector<int4> sl;
    std::vector<int32_t> ssb;
    settle_slices(gsb, sl, ssb);
    // each segment's tile range in the row-tile table (tiles of a segment are contiguous)
    std::vector<TileDev> tiles(v->n_tiles);
    if (v->n_tiles)
        OSK_HIP(hipMemcpyAsync(tiles.data(), v->d_tiles.p, sizeof(TileDev) * v->n_tiles, hipMemcpyDeviceToHost, st));
    OSK_HIP(hipStreamSynchronize(st));
    std::vector<int2> seg_tiles(ns, make_int2(0, 0));
    for (int t = 0; t < v->n_tiles; ++t) {
        int2& r = seg_tiles[tiles[t].seg];
        if (r.x == r.y) r = make_int2(t, t + 1);
        else r.y = t + 1;
    }
    v->n_gtiles = (int)gt.size();
    v->n_gslices = (int)sl.size();
    OSK_HIP(v->ws_tcnt.reserve(sizeof(int32_t) * std::max(1, v->n_tiles)));
    OSK_HIP(v->ws_scnt.reserve(sizeof(int32_t) * ns));
    OSK_HIP(v->ws_comp.reserve(sizeof(uint32_t) * std::max<int64_t>(1, total)));
    OSK_HIP(v->d_gtiles.upload(gt, st));
    OSK_HIP(v->d_gslices.upload(sl, st));
    OSK_HIP(v->d_gshard_slice_begin.upload(ssb, st));
    OSK_HIP(v->d_seg_tiles.upload(seg_tiles, st));
    OSK_HIP(hipStreamSynchronize(st));
    v->gather_ready = true;
    return OSK_OK;
}

int32_t ensure_sq8(osk_view* v, hipStream_t st) {
    if (v->sq8_ready) return OSK_OK;
    const int ns = (int)v->segs.size();
    std::vector<const void*> rows(ns);
    std::vector<const float4*> aux(ns);
    for (int i = 0; i < ns; ++i) {
        int32_t rc = ensure_sq8_seg(v->segs[i], st);
        if (rc) return rc;
        rows[i] = v->segs[i]->d_q8.p;
        aux[i] = v->segs[i]->d_q8aux.as<float4>();
    }
    v->units8 = (v->dim + 15) / 16;
    {
        std::vector<int4> sl;
        std::vector<int32_t> ssb;
        settle_slices(v->shard_tile_begin, sl, ssb);
        v->n_slices = (int)sl.size();
        OSK_HIP(v->d_slices.upload(sl, st));
        OSK_HIP(v->d_shard_slice_begin.upload(ssb, st));
    }
    // rounding bounds of the fp32 device order over n = 4·units products: γ_n ≤ n·2^-24
    // (any summation tree); gam = γ_n/2 with a 2× margin, g2 ≥ γ_{n+2} with margin.
    const double n = 4.0 * v->units;
    v->sq8_gam = (float)((n + 8.0) * std::ldexp(1.0, -24));
    v->sq8_g2 = (float)((n + 8.0) * std::ldexp(1.0, -23));
    v->sq8_cos_slack = (float)((n + 8.0) * std::ldexp(1.0, -23) + std::ldexp(1.0, -18));
    OSK_HIP(v->d_sq8_rows.upload(rows, st));
    OSK_HIP(v->d_sq8_aux.upload(aux, st));
    // the 6-bit tier: used only when every segment has one
    std::vector<const void*> rows6(ns);
    std::vector<const float4*> aux6(ns);
    bool all6 = ns > 0;
    for (int i = 0; i < ns; ++i) {
        rows6[i] = v->segs[i]->d_q6;
        aux6[i] = v->segs[i]->d_q6aux;
        all6 = all6 && rows6[i] && aux6[i];
    }
    if (all6) {
        OSK_HIP(v->d_sq6_rows.upload(rows6, st));
        OSK_HIP(v->d_sq6_aux.upload(aux6, st));
    }
    OSK_HIP(hipStreamSynchronize(st));
    v->sq6_ready = all6;
    v->sq8_range_ok = true;
    for (const osk_seg* sg : v->segs) v->sq8_range_ok = v->sq8_range_ok && !sg->sq8_out_of_range;
    v->sq8_ready = true;
    return OSK_OK;
}

}  // namespace osk
