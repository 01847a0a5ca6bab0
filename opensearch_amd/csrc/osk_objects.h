// osk_objects.h — the host-side object model of libosknn (osk_seg, osk_view, osk_comm helpers) shared
// by the C-ABI translation units (osk_api.hip, osk_comm.hip) and the lifetime and builder code
// (osk_derived.hip).  Not part of the public ABI.
//
//   osk_seg   one segment's vector field in HBM (rows padded to 16-byte units, optional row norms,
//             optional ord→doc map, and the derived copies the fast paths read: the int8 prefilter
//             copy + bound terms, its MFMA-tiled twin, the bf16 hi/lo split).  Reference counted:
//             the reader holds one reference ([L] KnnVectorsFormat.fieldsReader … close()), every view
//             that groups it holds another, so a segment merged away under a live view stays valid
//             until the view is released (NRT refresh churn, S/index/engine/InternalEngine.java:584-589).
//   osk_view  the segments of one or more shards on one device plus the scan's tile table and a
//             workspace.  A shard's exact top-k = per-leaf exact top-k merged by (score, doc)
//             ([L] AbstractKnnVectorQuery.rewrite, driven from
//             S/search/internal/ContextIndexSearcher.java:203-218).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/osknn.h"
#include "osk_internal.h"

namespace osk {

void set_error(const std::string& msg);
void clear_error();

#define OSK_HIP(call)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            ::osk::set_error(std::string(#call) + ": " + hipGetErrorString(e_));               \
            return OSK_ERR_DEVICE;                                                             \
        }                                                                                      \
    } while (0)

#define OSK_REQUIRE(cond, msg)                                                                 \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            ::osk::set_error(msg);                                                             \
            return OSK_ERR_INVALID;                                                            \
        }                                                                                      \
    } while (0)

#define OSK_GUARD_BEGIN try {
#define OSK_GUARD_END                                                                          \
    }                                                                                          \
    catch (const std::bad_alloc&) {                                                            \
        ::osk::set_error("host allocation failed");                                            \
        return OSK_ERR_OOM;                                                                    \
    }                                                                                          \
    catch (const std::exception& ex) {                                                         \
        ::osk::set_error(ex.what());                                                           \
        return OSK_ERR_INVALID;                                                                \
    }                                                                                          \
    catch (...) {                                                                              \
        ::osk::set_error("unknown exception");                                                 \
        return OSK_ERR_INVALID;                                                                \
    }

// devices and streams
int device_count_cached();
int32_t check_device(int device);      // also makes `device` current on this thread
hipStream_t device_stream(int device);  // the library's own non-blocking stream of a device

// device buffer that grows on demand (never inside a timed/captured call once warmed)
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) {
        o.p = nullptr;
        o.cap = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p;
            cap = o.cap;
            o.p = nullptr;
            o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        reset();
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    // A host table onto the device, on `st` (at least one element is reserved).  Does not synchronise: the
    // caller waits for the stream before `h` goes away.
    template <class T> hipError_t upload(const std::vector<T>& h, hipStream_t st) {
        hipError_t e = reserve(sizeof(T) * std::max<size_t>(1, h.size()));
        if (e == hipSuccess && !h.empty())
            e = hipMemcpyAsync(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, st);
        return e;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

struct HostPinned {
    void* p = nullptr;
    size_t cap = 0;
    HostPinned() = default;
    HostPinned(const HostPinned&) = delete;
    HostPinned& operator=(const HostPinned&) = delete;
    ~HostPinned() {
        if (p) (void)hipHostFree(p);
    }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) {
            (void)hipHostFree(p);
            p = nullptr;
            cap = 0;
        }
        hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
};

inline int units_for(int dim, int enc) { return enc == ENC_FLOAT32 ? (dim + 3) / 4 : (dim + 15) / 16; }
inline int64_t elem_bytes(int enc) { return enc == ENC_FLOAT32 ? 4 : 1; }
// A device entry's stream argument: the caller's stream, or (null) the library's own stream of the device.
inline hipStream_t stream_or_default(void* stream, int device) {
    return stream ? static_cast<hipStream_t>(stream) : device_stream(device);
}

}  // namespace osk

struct osk_seg {
    int device = 0;
    int64_t n_rows = 0;
    int dim = 0, enc = 0, sim = 0, max_doc = 0;
    int units = 0, cfg = 0;
    // device memory: each buffer is reserved once, at its exact size (hbm_bytes is the sum of the capacities)
    osk::DevBuf d_rows;
    osk::DevBuf d_xnorm_f;             // float |x|² per row (cosine; added by ensure_split otherwise)
    osk::DevBuf d_xnorm_i;             // int32 |x|² per row (byte fields)
    osk::DevBuf d_ord_to_doc;          // int32 per row (sparse fields)
    // batched MFMA path (built by osk_seg_warm or on first batched search): bf16 hi/lo copy in MFMA
    // fragment order, |x|² per row (device lane order) and max |x|² of the segment
    osk::DevBuf d_split;
    int split_KS = 0;
    osk::DevBuf d_maxnorm2;            // [1] unsigned: the bits of max |x|²
    osk::DevBuf d_xsqrt;               // float |x| per row (MFMA path)
    float h_maxnorm2 = 0.0f;
    // certified int8 prefilter (built at staging for float32 segments): int8 rows + per-row bound terms
    osk::DevBuf d_q8;
    osk::DevBuf d_q8aux;               // float4 per row
    bool sq8_out_of_range = false;   // some row lies outside the certificate's range (sq8_in_range; set with d_q8)
    osk::DevBuf d_q8t;        // the int8 rows in sq8_mfma's tiled layout (osk_seg_warm / first batched prefilter)
    osk::DevBuf d_q8w;            // sq8_wide's copy: codes with one scale per 16-row group, tiled (launch_sq8w_build)
    osk::DevBuf d_q8auxt;         // ...and its float4 bound terms per 16-row group (built with d_q8w)
    void* d_q6 = nullptr;     // the 6-bit tier (dims with sq6_supported, tune sq6 on at staging): tiled codes,
    float4* d_q6aux = nullptr;   // built with the int8 copy; freed when the segment's calibration turns it off
    // The 6-bit tier's calibration, per segment: every view over the segment (a searcher's view, its
    // leased replicas, the next refresh's view) shares it.  Probe calls count, per segment, the rows they
    // re-bound from the int8 copy (read back asynchronously, osk_api.hip fold_probe); after kSq6Probes
    // probes the tier stays on, or turns off (above sq6_probe_pct % of the rows) and its copy is freed.
    std::atomic<int> sq6_state{0};     // 0 probing, 1 on, 2 off
    int sq6_probes = 0;                // (guarded by mu)
    int64_t sq6_probe_rows = 0, sq6_probe_rebound = 0;
    int units8 = 0;
    // nested k-NN (osk_seg_set_parents, once per segment): each row's parent rank among the leaf's parent
    // docs ([L] the BitSetProducer of the nested path), and their number; guarded by mu
    osk::DevBuf d_row_parent;          // int32 per row
    int64_t n_parents = 0;
    std::mutex mu;
    std::atomic<int> refs{1};          // the reader's reference + one per view that groups the segment
    osk_view* self_view = nullptr;     // single-segment view behind osk_seg_search (holds no reference)
    ~osk_seg();
    int64_t hbm_bytes() const;         // every device allocation the segment owns
};

struct osk_view {
    int device = 0, dim = 0, enc = 0, sim = 0, units = 0, cfg = 0;
    std::vector<osk_seg*> segs;
    bool holds_refs = true;            // false for a segment's own self_view
    std::vector<int32_t> seg_shard, seg_doc_base;
    int n_shards = 0;
    std::vector<int32_t> shard_index;
    std::vector<int32_t> shard_tile_begin;
    int n_tiles = 0;
    osk::DevBuf d_segs, d_tiles, d_shard_tile_begin, d_shard_index, d_tile_coff, d_tile_order;
    // workspace
    osk::DevBuf ws_cand, ws_q, ws_qnorm, ws_qin, ws_keys, ws_counts, ws_accept_ptrs, ws_accept,
        ws_out, ws_visited;
    osk::HostPinned h_stage;
    osk::HostPinned h_accept_tab;     // upload_accept's pointer table (source of an async copy)
    // batched MFMA path
    bool mfma_ready = false;
    int n_munits = 0;
    int mfma_KS = 0;
    double mfma_c = 0.0;
    osk::DevBuf d_munits, d_seg_split, d_seg_xsqrt, d_seg_vrow, d_shard_unit_begin, d_shard_maxnorm2;
    osk::DevBuf ws_qsplit, ws_cand_a, ws_akeys, ws_acounts, ws_pkeys, ws_pcounts, ws_flags, ws_fbq, ws_fbkeys,
        ws_fbcounts;
    osk::HostPinned h_flags;
    int64_t mfma_calls = 0, mfma_fallback_queries = 0;
    osk::DevBuf d_mfma_full;               // [1] tiles whose candidate epilogue took the staging path
    // certified int8 prefilter
    bool sq8_ready = false;
    bool sq8_range_ok = true;   // (with sq8_ready) no segment has a row outside the certificate's range
    int units8 = 0;
    float sq8_gam = 0.f, sq8_g2 = 0.f, sq8_cos_slack = 0.f;
    osk::DevBuf d_sq8_rows, d_sq8_aux, d_counters;   // counters: [kCtrCount] slots (osk_internal.h Ctr)
    osk::DevBuf d_sq8_rows_t;                         // per segment: tiled int8 copy (sq8_mfma)
    osk::DevBuf d_sq8_rows_w;                         // per segment: the wide kernel's group-scaled copy
    osk::DevBuf d_sq8_auxt, d_shard_quarter_begin;    // per segment: its tiled bound terms (sq8_wide); 4·shard_tile_begin
    osk::DevBuf d_quarter_bm;                         // per (wide tile, quarter): its rows' bound-term maxima
    osk::DevBuf d_wqtable;                            // per quarter in tile order: the wide kernels' descriptor
    // sq8_wide's own tiles (ensure_sq8w: quarters of ≈ R / (2·CUs) rows), their shard ranges and dispatch order
    osk::DevBuf d_wtiles, d_wtile_order, d_wshard_tile_begin;
    std::vector<int32_t> wshard_tile_begin;
    int n_wtiles = 0;
    bool sq8t_ready = false;   // sq8_mfma's tiled copy pointers (ensure_sq8t)
    bool sq8w_ready = false;   // the wide kernel's copies, pointers and tile table (ensure_sq8w)
    osk::DevBuf d_sq6_rows, d_sq6_aux;                // per segment: the 6-bit tier (every segment has one or
    bool sq6_ready = false;                           // the view does not use it)
    int64_t sq6_calls = 0;
    osk::DevBuf ws_q6, ws_qc6, ws_floor;              // its query (nibble split, bound terms), floor buckets,
    osk::DevBuf ws_cand6, ws_cnt6;                    // the streaming pass's candidates per list {row, 6-bit test}
    // the share group of the views over this segment set with this tile table (osk_api.hip Sq6Group): joined at
    // the view's first call that may share, left in the destructor; share_slot < 0: not in a group (none tried
    // yet, or no free slot).  share_held (testing build): a call stopped after its post, for the resume entry.
    std::vector<osk::TileDev> h_tiles;                // the tile table and its dispatch order (the group's key)
    std::vector<int32_t> h_tile_order;
    void* share_group = nullptr;
    int share_slot = -1;
    bool share_tried = false;
    int share_stop = 0;                               // (testing build) 1: this call stops after its post
    std::shared_ptr<void> share_held;
    // the tier's calibration (per segment, osk_seg::sq6_state): a probe call of this view counts its int8
    // re-bounds per segment into d_seg_rebound, copies them to h_seg_rebound on its stream and records
    // ev_probe; a later call folds them into the segments once the event has completed — nothing waits
    osk::DevBuf d_seg_rebound;
    osk::HostPinned h_seg_rebound;
    hipEvent_t ev_probe = nullptr;
    bool probe_pending = false;
    osk::DevBuf ws_q8, ws_qc, ws_sq8cand, ws_sq8lb, ws_lbmax, ws_trace;
    // settle slices: kSliceLists wave lists each, never spanning shards (an empty shard gets one
    // empty slice so that its result is still written)
    int n_slices = 0;
    osk::DevBuf d_slices, d_shard_slice_begin, ws_part;
    osk::DevBuf ws_pilot, ws_thr, ws_thr_counts;   // int8 MFMA prefilter: pilot keys, per-(query, shard) floors
    osk::DevBuf ws_wfloor;                          // sq8_wide: the two passes' floors [2][kWideQ][S]
    int64_t sq8_calls = 0, sq8w_calls = 0;
    int64_t sq8_lists_last = 0;            // wave lists per query of the last prefiltered search (debug copies)
    int n_cus = 0;                         // the device's CUs (cached; the wide kernel's persistent grid)   // prefiltered searches; those whose batch took sq8_wide
    // filter pushdown by compaction (osk_filter.hip): gather tiles over the compacted accepted ordinals
    // (one round of the chip, split over segments by rows), their settle slices, per-segment tile ranges
    // the select path (osk_select.hip, any k): per-row records of one query, radix state, candidates
    osk::DevBuf ws_sel_lb, ws_sel_ub, ws_sel_keys, ws_sel_state, ws_sel_hist, ws_sel_cand, ws_sel_cand2, ws_sel_cnt;
    int64_t sel_calls = 0;
    // similarity-threshold search (osk_threshold.hip): hit mask, per-wave counts and offsets of one corpus
    // pass (≤ kThrNQ queries), the thresholds, and the host entries' device outputs
    int64_t max_tile_rows = 0;             // the largest tile's rows (sizes the mask: thr_words_per_wave)
    osk::DevBuf ws_thr_mask, ws_thr_wcounts, ws_thr_offsets, ws_thr_min, ws_thr_out;
    osk::DevBuf ws_thr_maybe;              // the int8 first pass's second mask: rows to re-score exactly
    int64_t thr_calls = 0, thr_sq8_calls = 0;   // threshold searches; those that took the int8 first pass
    // ...and its top-k entries (osk_*_search_threshold_top): calls, those with k > kScanMaxK (the select path's
    // tail), and the host entries' per-(query, shard) totals; their int8 first passes count in thr_sq8_calls
    int64_t thr_top_calls = 0, thr_top_sel_calls = 0;
    osk::DevBuf ws_thr_tot;
    // nested k-NN (osk_nested.hip), built at the first nested search or by osk_view_warm (ensure_nested): each
    // segment's row→parent table and parent-slot base (a shard's parent slots are contiguous), the parent
    // tiles and their shard ranges; the per-pass best-child keys and the parent tiles' candidates
    bool nest_ready = false;
    int64_t nest_parents = 0;
    int n_ptiles = 0;
    osk::DevBuf d_nest_segs, d_ptiles, d_shard_ptile_begin, ws_nest_best, ws_nest_cand;
    // ...and of the int8 first pass (float32 views): the per-row upper-bound records and per-parent lower-bound
    // keys of one pass (≤ kNestSq8NQ queries), the parent tiles' and the shards' floor lists
    osk::DevBuf ws_nest_ub, ws_nest_lbkey, ws_nest_fcand, ws_nest_fkeys, ws_nest_fcounts;
    int64_t nest_calls = 0, nest_sq8_calls = 0;   // nested searches; those that took the int8 first pass
    bool gather_ready = false;
    int n_gtiles = 0, n_gslices = 0;
    osk::DevBuf d_gtiles, d_gslices, d_gshard_slice_begin, d_seg_tiles;
    osk::DevBuf ws_tcnt, ws_scnt, ws_comp;
    // multi-GPU exchange (osk_comm.hip): this rank's block (lists padded to the call's shards per rank,
    // header, shard indices), the gathered blocks of every rank, the host entry's reduce outputs
    osk::DevBuf ws_xkeys, ws_xgath, ws_xout, ws_xspr;
    std::mutex mu;
    // scan-kernel timing (osk_view_profile): a ring of (start, stop) event pairs, one per search call,
    // folded into scan_ms when a slot is reused (kEvRing calls later: long complete, no host wait) or
    // when the total is read — timing never blocks the host inside the timed loop
    static constexpr int kEvRing = 64;
    bool profile = false;            // the current call stamps its scan launches (osk_view_profile)
    int profile_every = 0;           // osk_view_profile(enable): 0 off, N = every N-th call is sampled
    uint64_t profile_tick = 0;
    hipEvent_t ev_start[kEvRing] = {}, ev_stop[kEvRing] = {};
    bool ev_pending[kEvRing] = {};
    int64_t ev_next = 0;                  // calls started since enabling
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // the current call's pair
    hipEvent_t ev_call[2] = {};                 // host entries' per-call device time (tune call_timing)
    double scan_ms = 0.0;
    int64_t scan_calls = 0;
    // cross-stream ordering of the workspace: the stream of the previous search, and an event recorded
    // on it when a search arrives on another stream (order_after_last)
    hipStream_t last_stream = nullptr;
    hipEvent_t xs_event = nullptr;
    // Host entries (osk_view_search, osk_seg_search) are synchronous calls from the search thread
    // pools.  Each concurrent call leases a workspace slot — slot 0 is this view, slot i > 0 a replica
    // view over the same segments (own workspace) — and the slot's own stream, so concurrent searches
    // of one shard set run concurrently on the device instead of queueing on one workspace.
    static constexpr int kMaxLeases = 8;
    std::mutex lease_mu;
    std::condition_variable lease_cv;
    std::vector<osk_view*> replicas;          // slots 1.. (created on demand)
    std::vector<hipStream_t> lease_streams;   // one per slot
    std::vector<char> lease_busy;             // per slot
    // opportunistic batching of concurrent host calls (osk_api.hip batched_call)
    struct Batcher {
        std::mutex mu;
        std::condition_variable cv;
        std::deque<void*> queue;              // waiting requests (BatchReq*)
        int leaders = 0;                      // batches in flight
        int64_t batches = 0, requests = 0;
    } batcher;
    ~osk_view();
};

namespace osk {
// Drop one reference of a segment (deletes it at zero).
void seg_unref(osk_seg* s);

// ---- lifetime and built-once structures (osk_derived.hip)
// The device view of a view's segments (pointers re-read: staging may add row norms later).
std::vector<SegDev> seg_devs(const osk_view* v);
// A new segment with its padded rows allocated (arguments checked; the device made current).
int32_t seg_alloc(int device, int64_t n_rows, int dim, int enc, int sim, int max_doc, const int32_t* ord_to_doc,
                  std::unique_ptr<osk_seg>& out);
// The rest of staging once the rows are on the device: row norms, ord→doc map, the int8 prefilter copy.
int32_t seg_finish(osk_seg* s, const int32_t* ord_to_doc, hipStream_t st);
// The segment's bf16 hi/lo copy in MFMA fragment order (+ |x|² rows and their max).  Built once.
int32_t ensure_split(osk_seg* s, hipStream_t st);
// MFMA work units (runs of 128-row tiles, contiguous per shard) and per-shard bounds.  Built once.
int32_t ensure_mfma(osk_view* v, hipStream_t st);
// The view's tables of the nested search (caller holds v->mu).  Built once.
int32_t ensure_nested(osk_view* v, hipStream_t st);
// The segment's int8 copy + per-row bound terms for the certified prefilter.  Built once.
int32_t ensure_sq8_seg(osk_seg* s, hipStream_t st);
// The segment's int8 copy in sq8_mfma's tiled layout and (wide) the wide kernel's group-scaled copy.  Built once.
int32_t ensure_sq8t_seg(osk_seg* s, hipStream_t st, bool wide);
// The view's table of its segments' tiled int8 copies.  Built once.
int32_t ensure_sq8t(osk_view* v, hipStream_t st);
// The wide kernel's inputs for a view (first batch the cost model sends to it).
int32_t ensure_sq8w(osk_view* v, hipStream_t st);
// The view's prefilter tables: int8 and 6-bit copies of its segments, settle slices, rounding bounds.  Built once.
int32_t ensure_sq8(osk_view* v, hipStream_t st);
// Settle slices over the wave lists of a tile table (list = tile·4 + wave), never spanning shards.
void settle_slices(const std::vector<int32_t>& shard_tile_begin, std::vector<int4>& sl, std::vector<int32_t>& ssb);
// Gather tiles for filtered scans over the compacted accepted ordinals (osk_filter.hip).  Built once.
int32_t ensure_gather(osk_view* v, hipStream_t st);
// the device's CUs (cached; the persistent kernels' grids and the wide tile table are sized by them)
int view_cus(osk_view* v);

// ---- the 6-bit tier's records (osk_api.hip), as the destructors need them
// A segment being destroyed leaves the in-flight records of the 6-bit launches (which have completed).
void sq6_forget_segment(const osk_seg* sg);
// A view being destroyed leaves its share group (waits for the group's scans).
void sq6_share_detach(osk_view* v);

// Order this call's use of the view's workspace after the previous call's (another stream).
int32_t order_after_last(osk_view* v, hipStream_t st);
// A leased workspace slot of a view (host entries): `v` is the view or one of its replicas, `st` the
// slot's stream.  Released (and a waiting caller woken) when the lease goes out of scope.
struct ViewLease {
    osk_view* root = nullptr;
    osk_view* v = nullptr;
    hipStream_t st = nullptr;
    int slot = -1;
    ViewLease() = default;
    ViewLease(const ViewLease&) = delete;
    ViewLease& operator=(const ViewLease&) = delete;
    ~ViewLease();
};
int32_t lease_view(osk_view* root, ViewLease& out);
// Host accept bitsets → the view's workspace, on `st` (caller holds v->mu).  `accept` is null or
// v->segs.size() host bitsets (entries may be null).  *d_accept: the device pointer table, or null when no
// leaf has a bitset = no filter (the unfiltered scan instances).
int32_t upload_accept(osk_view* v, const uint64_t* const* accept, hipStream_t st, const uint64_t* const** d_accept);
// A host search's merged result in one buffer, nq queries of `size` hits:
// scores f32 | docs i32 | shard i32 | count i32 | total i64 (8-aligned) | max f32.  The coordinator reduce
// writes it on the device, one copy brings it to a pinned stage, copy_out hands it to the caller's arrays.
struct MergedOut {
    size_t b_hits, b_cnt, b_tot, b_max;   // bytes of scores / docs / shard each, count, total, max
    size_t o_sc, o_doc, o_sh, o_cnt, o_tot, o_max, total_bytes;
    MergedOut(int nq, int size)
        : b_hits((size_t)nq * size * 4), b_cnt((size_t)nq * 4), b_tot((size_t)nq * 8), b_max((size_t)nq * 4),
          o_sc(0), o_doc(o_sc + b_hits), o_sh(o_doc + b_hits), o_cnt(o_sh + b_hits),
          o_tot((o_cnt + b_cnt + 7) / 8 * 8), o_max(o_tot + b_tot), total_bytes(o_max + b_max) {}
    struct Ptrs {   // launch_coord_reduce's outputs
        float* scores;
        int32_t *docs, *shard, *count;
        int64_t* total;
        float* max;
    };
    Ptrs at(char* base) const {
        return {reinterpret_cast<float*>(base + o_sc),    reinterpret_cast<int32_t*>(base + o_doc),
                reinterpret_cast<int32_t*>(base + o_sh),  reinterpret_cast<int32_t*>(base + o_cnt),
                reinterpret_cast<int64_t*>(base + o_tot), reinterpret_cast<float*>(base + o_max)};
    }
    void copy_out(const char* stage, float* scores, int32_t* docs, int32_t* shard, int32_t* count, int64_t* total,
                  float* max) const;
};
// Per-shard exact top-k on the device (caller holds v->mu; device current).
int32_t view_search_device(osk_view* v, const void* d_queries, int nq, int k, const uint64_t* const* d_accept,
                           uint64_t* d_shard_keys, int32_t* d_shard_counts, int64_t* d_visited, hipStream_t st);
// Per-shard similarity-threshold search on the device (caller holds v->mu; device current).
int32_t view_threshold_device(osk_view* v, const void* d_queries, int nq, const float* d_min_scores,
                              const uint64_t* const* d_accept, int cap, int32_t* d_docs, float* d_scores,
                              int32_t* d_count, int64_t* d_total, int64_t* d_visited, hipStream_t st);
// Per-shard best k of a similarity-threshold search's hits, with the exact totals (caller holds v->mu; device
// current).  Same key layout as view_search_device.
int32_t view_threshold_top_device(osk_view* v, const void* d_queries, int nq, const float* d_min_scores, int k,
                                  const uint64_t* const* d_accept, uint64_t* d_shard_keys,
                                  int32_t* d_shard_counts, int64_t* d_shard_totals, int64_t* d_visited,
                                  hipStream_t st);
// Per-shard nested k-NN on the device: the k best parents, each by its best child (caller holds v->mu;
// device current).  Same key layout as view_search_device.
int32_t view_nested_device(osk_view* v, const void* d_queries, int nq, int k, const uint64_t* const* d_accept,
                           uint64_t* d_shard_keys, int32_t* d_shard_counts, int64_t* d_visited, hipStream_t st);
}  // namespace osk
