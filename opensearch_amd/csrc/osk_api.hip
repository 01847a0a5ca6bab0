// osk_api.hip — the C-ABI of libosknn.so (declared in include/osknn.h): segments, views, the
// single-device search paths and the coordinator merge.  The object model (osk_seg, osk_view) is in
// osk_objects.h, its lifetime and the built-once structures in osk_derived.hip; the multi-GPU exchange
// (osk_comm, RCCL) in osk_comm.hip.
// Every entry point catches all C++ exceptions and returns an error code (see osknn.h).
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cerrno>
#include <cstring>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "osk_objects.h"

using namespace osk;

namespace {
std::mutex g_dev_mu;
std::vector<hipStream_t> g_streams;
int g_ndev = -1;
// Per-call device time of this thread's last synchronous host search (osk_last_call_device_ns):
// nanoseconds between the call's first and last device operation on its stream, and how many host
// requests shared that launch chain (opportunistic batching).  −1 / 0: timing off or no call yet.
thread_local int64_t t_call_ns = -1;
thread_local int32_t t_call_shared = 0;

// Call timing of a host search (tune "call_timing"): events bracket the call's work on its stream.
struct CallTimer {
    osk_view* v = nullptr;
    hipStream_t st = nullptr;
    int32_t begin(osk_view* view, hipStream_t stream) {
        t_call_ns = -1;
        t_call_shared = 0;
        if (!g_tuning.call_timing) return OSK_OK;
        for (hipEvent_t& e : view->ev_call)
            if (!e) OSK_HIP(hipEventCreate(&e));
        v = view;
        st = stream;
        OSK_HIP(hipEventRecord(v->ev_call[0], st));
        return OSK_OK;
    }
    int32_t end() {   // before the call's final stream synchronisation
        if (v) OSK_HIP(hipEventRecord(v->ev_call[1], st));
        return OSK_OK;
    }
    int32_t publish() {   // after it
        if (!v) return OSK_OK;
        float ms = 0.f;
        OSK_HIP(hipEventElapsedTime(&ms, v->ev_call[0], v->ev_call[1]));
        t_call_ns = (int64_t)((double)ms * 1e6);
        t_call_shared = 1;
        return OSK_OK;
    }
};
}  // namespace

namespace osk {

// ------------------------------------------------------------------------------------------------
// devices and streams
// ------------------------------------------------------------------------------------------------

int device_count_cached() {
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (g_ndev < 0) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        g_ndev = n;
        g_streams.assign(n, nullptr);
    }
    return g_ndev;
}

int32_t check_device(int device) {
    const int n = device_count_cached();
    if (n <= 0) {
        set_error("no HIP device visible (libosknn has no CPU fallback)");
        return OSK_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) {
        set_error("device index out of range");
        return OSK_ERR_INVALID;
    }
    static std::atomic<int> arch_ok[64];   // per device: 0 unknown, 1 gfx950, 2 another arch
    if (device >= 64 || arch_ok[device].load() == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
            set_error("hipGetDeviceProperties failed");
            return OSK_ERR_DEVICE;
        }
        const bool ok = std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
        if (device < 64) arch_ok[device].store(ok ? 1 : 2);
        if (!ok) {
            set_error(std::string("device is ") + prop.gcnArchName + ", libosknn is built for gfx950");
            return OSK_ERR_NO_DEVICE;
        }
    } else if (arch_ok[device].load() == 2) {
        set_error("device is not gfx950; libosknn is built for gfx950");
        return OSK_ERR_NO_DEVICE;
    }
    if (hipSetDevice(device) != hipSuccess) {
        set_error("hipSetDevice failed");
        return OSK_ERR_DEVICE;
    }
    return OSK_OK;
}

// No device at all: the answer of an entry whose handle cannot be real then (checked before it is read).
int32_t any_device() {
    if (device_count_cached() > 0) return OSK_OK;
    set_error("no HIP device visible (libosknn has no CPU fallback)");
    return OSK_ERR_NO_DEVICE;
}

hipStream_t device_stream(int device) {
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (!g_streams[device]) {
        hipStream_t s;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
        g_streams[device] = s;
    }
    return g_streams[device];
}

}  // namespace osk

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int32_t osk_abi_version(void) { return OSK_ABI_VERSION; }

int32_t osk_tune_set(const char* key, int64_t value) {
    OSK_GUARD_BEGIN
    OSK_REQUIRE(key != nullptr, "key is null");
    const std::string k(key);
    struct Knob { const char* name; std::atomic<int>* v; int64_t lo, hi; bool testing; };
    const Knob knobs[] = {
        {"scan_nt", &g_tuning.scan_nt, 0, 1, false},
        {"host_batching", &g_tuning.host_batching, 0, 1, false},
        {"host_batch_leaders", &g_tuning.host_batch_leaders, 1, 8, false},
        {"tiles_target", &g_tuning.tiles_target, 0, 1 << 22, false},
        {"tile_slots_per_cu", &g_tuning.tile_slots_per_cu, 1, 64, false},
        {"tile_max_rounds", &g_tuning.tile_max_rounds, 1, 1024, false},
        {"tile_large_slots", &g_tuning.tile_large_slots, 0, 1024, false},
        {"tile_large_slots_512", &g_tuning.tile_large_slots_512, 0, 1024, false},
        {"tile_min_rows", &g_tuning.tile_min_rows, 1, 1 << 24, false},
        {"mfma_min_batch", &g_tuning.mfma_min_batch, 0, 1 << 30, false},
        {"sq8_cost_pct", &g_tuning.sq8_cost_pct, 0, 100000, false},
        {"mfma_units", &g_tuning.mfma_units, 0, 32768, false},
        {"sq8", &g_tuning.sq8, 0, 1, false},
        {"sq6", &g_tuning.sq6, 0, 1, false},
        {"sq6_probe_pct", &g_tuning.sq6_probe_pct, 0, 100, false},
        {"filter_gather", &g_tuning.filter_gather, 0, 1, false},
        {"select_mid_k", &g_tuning.select_mid_k, 0, 1, false},
        {"sel_writer", &g_tuning.sel_writer, 0, 3, false},
        {"gather_min", &g_tuning.gather_min, 0, 1 << 20, false},
        {"sq8_mfma_nt", &g_tuning.sq8_mfma_nt, 0, 1, false},
        {"sq8_mfma_queries", &g_tuning.sq8_mfma_queries, 16, 32, false},
        {"sq8_mfma_min", &g_tuning.sq8_mfma_min, 0, 1 << 20, false},
        {"sq8_wide_min", &g_tuning.sq8_wide_min, 0, 1 << 20, false},
        {"sq8_wide_force", &g_tuning.sq8_wide_force, 0, 1, false},
        {"sq8_wide_phase", &g_tuning.sq8_wide_phase, 0, 1 << 16, false},
        {"sq8_wide_grid", &g_tuning.sq8_wide_grid, 0, 1 << 16, false},
        {"sq8_wide_quarter_rows", &g_tuning.sq8_wide_quarter_rows, 0, 1 << 20, false},
        {"sq8_wide_pilot_rows", &g_tuning.sq8_wide_pilot_rows, 0, 1 << 16, false},
        {"sq8_wide_defer", &g_tuning.sq8_wide_defer, 0, 1, false},
        {"sq8_wide_rows", &g_tuning.sq8_wide_rows, 0, 1, false},
        {"sq8_wide_rows_qcap", &g_tuning.sq8_wide_rows_qcap, 0, 1 << 20, false},
        {"sq8_scan_deep", &g_tuning.sq8_scan_deep, 0, 1, false},
        {"sq8_wide_rows_claim", &g_tuning.sq8_wide_rows_claim, 0, 1, false},
        {"sq6_rebound_stride", &g_tuning.sq6_rebound_stride, 0, 1, false},
        {"sq6_rebound_retest", &g_tuning.sq6_rebound_retest, 0, 1, false},
        {"sq6_rebound_wgs", &g_tuning.sq6_rebound_wgs, 0, 16, false},
        {"sq6_share", &g_tuning.sq6_share, 0, 1, false},
        {"sq6_share_min_tiles", &g_tuning.sq6_share_min_tiles, 0, 1 << 24, false},
        {"sq6_share_idle", &g_tuning.sq6_share_idle, 0, 1, false},
        {"sq6_share_limit", &g_tuning.sq6_share_limit, -1, 1 << 24, true},
        {"sq8_mfma_ring", &g_tuning.sq8_mfma_ring, -1, 8, false},
        {"i8_stream", &g_tuning.i8_stream, 0, 1, false},
        {"ham_stream", &g_tuning.ham_stream, 0, 1, false},
        {"call_timing", &g_tuning.call_timing, 0, 1, false},
        {"thr_sq8", &g_tuning.thr_sq8, 0, 1, false},
        {"thr_sq8_all_maybe", &g_tuning.thr_sq8_all_maybe, 0, 1, true},
        {"nest_sq8", &g_tuning.nest_sq8, 0, 1, false},
        {"nest_sq8_all_settle", &g_tuning.nest_sq8_all_settle, 0, 1, true},
        {"sq8_mfma_ablate", &g_tuning.sq8_mfma_ablate, 0, 1023, true},   // (also sq6_scan's: 1 no re-bound, 2 no floor,
                                                                          // 16 loads only; sq6_rebound's: 256 no list work)
        {"sq8_force_fallback", &g_tuning.sq8_force_fallback, 0, 1, true},
        {"settle_trace", &g_tuning.settle_trace, 0, 1, true},
        {"mfma_ablate", &g_tuning.mfma_ablate, 0, 255, true},
    };
    for (const Knob& kn : knobs) {
        if (k != kn.name) continue;
#ifndef OSK_TESTING
        if (kn.testing) {
            set_error("tuning key " + k + " exists only in the testing build (libosknn_testing.so)");
            return OSK_ERR_UNSUPPORTED;
        }
#endif
        OSK_REQUIRE(value >= kn.lo && value <= kn.hi, "tuning value out of range for " + k);
        if (k == "sq8_mfma_queries") OSK_REQUIRE(value == 16 || value == 32, "sq8_mfma_queries must be 16 or 32");
        kn.v->store((int)value);
        return OSK_OK;
    }
    set_error("unknown tuning key: " + k);
    return OSK_ERR_INVALID;
    OSK_GUARD_END
}

int32_t osk_testing_glds_probe(int32_t device, int64_t* out_mismatches) {
    OSK_GUARD_BEGIN
    clear_error();
#ifndef OSK_TESTING
    (void)device; (void)out_mismatches;
    set_error("osk_testing_glds_probe exists only in the testing build (libosknn_testing.so)");
    return OSK_ERR_UNSUPPORTED;
#else
    OSK_REQUIRE(out_mismatches != nullptr, "out_mismatches is null");
    int32_t rc = check_device(device);
    if (rc) return rc;
    constexpr int kSrc = 1024, kImg = 1024, kCases = 6;
    std::vector<int4> h_src(kSrc), h_out((size_t)kCases * kImg);
    for (int i = 0; i < kSrc; ++i) h_src[i] = make_int4(i, i ^ 0x5A5A, 3 * i + 1, 7);
    DevBuf d_src, d_out;
    OSK_HIP(d_src.reserve(kSrc * sizeof(int4)));
    if (d_out.reserve(h_out.size() * sizeof(int4)) != hipSuccess) {
        set_error("hipMalloc failed");
        return OSK_ERR_DEVICE;
    }
    hipError_t e = hipMemcpy(d_src.p, h_src.data(), kSrc * sizeof(int4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_glds_probe(d_src.as<int4>(), d_out.as<int4>(), nullptr);
    if (e == hipSuccess) e = hipMemcpy(h_out.data(), d_out.p, h_out.size() * sizeof(int4), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        set_error(std::string("glds probe: ") + hipGetErrorString(e));
        return OSK_ERR_DEVICE;
    }
    // the expected image of each case: DMA k's 64 lanes at 3072 + (N − 1 − k)·2048 + 512 + lane·16, all else −1
    int64_t bad = 0;
    const int ns[kCases] = {1, 2, 4, 1, 2, 4}, gs[kCases] = {1024, 1024, 1024, kAuxGroupF4 * 16, kAuxGroupF4 * 16,
                                                             kAuxGroupF4 * 16};
    for (int c = 0; c < kCases; ++c) {
        std::vector<int4> want(kImg, make_int4(-1, -1, -1, -1));
        for (int k = 0; k < ns[c]; ++k)
            for (int l = 0; l < 64; ++l) want[(3072 + (ns[c] - 1 - k) * 2048 + 512) / 16 + l] = h_src[(k * gs[c]) / 16 + l];
        for (int i = 0; i < kImg; ++i) {
            const int4 a = h_out[(size_t)c * kImg + i], b = want[i];
            bad += a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w;
        }
    }
    *out_mismatches = bad;
    return OSK_OK;
#endif
    OSK_GUARD_END
}

int32_t osk_device_count(int32_t* n) {
    OSK_GUARD_BEGIN
    OSK_REQUIRE(n != nullptr, "n is null");
    *n = device_count_cached();
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_seg_stage(int32_t device, const void* rows, int64_t n_rows, int32_t dim,
                      int32_t encoding, int32_t similarity, const int32_t* ord_to_doc,
                      int32_t max_doc, osk_seg** out) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(out != nullptr, "out is null");
    OSK_REQUIRE(rows != nullptr || n_rows == 0, "rows is null");
    std::unique_ptr<osk_seg> s;
    int32_t rc = seg_alloc(device, n_rows, dim, encoding, similarity, max_doc, ord_to_doc, s);
    if (rc) return rc;
    hipStream_t st = device_stream(device);
    const int64_t elem = elem_bytes(encoding);
    const int64_t src_pitch = (int64_t)dim * elem;
    const int64_t dst_pitch = (int64_t)s->units * 16;
    if (n_rows > 0) {
        OSK_HIP(hipMemset2DAsync(s->d_rows.p, dst_pitch, 0, dst_pitch, n_rows, st));
        OSK_HIP(hipMemcpy2DAsync(s->d_rows.p, dst_pitch, rows, src_pitch, src_pitch, n_rows,
                                 hipMemcpyHostToDevice, st));
    }
    rc = seg_finish(s.get(), ord_to_doc, st);
    if (rc) return rc;
    *out = s.release();
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_seg_stage_file(int32_t device, const char* path, int64_t data_offset, int64_t n_rows, int32_t dim,
                           int32_t encoding, int32_t similarity, const int32_t* ord_to_doc, int32_t max_doc,
                           osk_seg** out) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(out != nullptr && path != nullptr, "null argument");
    OSK_REQUIRE(data_offset >= 0, "negative data offset");
    std::unique_ptr<osk_seg> s;
    int32_t rc = seg_alloc(device, n_rows, dim, encoding, similarity, max_doc, ord_to_doc, s);
    if (rc) return rc;
    hipStream_t st = device_stream(device);
    const int64_t row_bytes = (int64_t)dim * elem_bytes(encoding);
    const int64_t bytes = n_rows * row_bytes;
    const int64_t dst_pitch = (int64_t)s->units * 16;
    if (n_rows > 0) {
        // the .vec slice: memory-mapped (as FsDirectoryFactory maps .vec under hybridfs), copied chunk by
        // chunk into one of two pinned buffers while the other one's H2D copy runs, then into the
        // segment's padded rows (zeros past dim)
        const int fd = ::open(path, O_RDONLY | O_CLOEXEC);
        if (fd < 0) {
            set_error(std::string("cannot open ") + path + ": " + std::strerror(errno));
            return OSK_ERR_INVALID;
        }
        struct stat sb;
        if (::fstat(fd, &sb) != 0 || sb.st_size < data_offset + bytes) {
            ::close(fd);
            set_error(std::string(path) + " is shorter than the field's vector data");
            return OSK_ERR_INVALID;
        }
        const int64_t page = ::sysconf(_SC_PAGESIZE);
        const int64_t map_off = data_offset / page * page;
        const size_t map_len = (size_t)(data_offset + bytes - map_off);
        void* map = ::mmap(nullptr, map_len, PROT_READ, MAP_PRIVATE, fd, map_off);
        ::close(fd);
        if (map == MAP_FAILED) {
            set_error(std::string("mmap of ") + path + " failed: " + std::strerror(errno));
            return OSK_ERR_INVALID;
        }
        (void)::madvise(map, map_len, MADV_SEQUENTIAL);
        const char* src = static_cast<const char*>(map) + (data_offset - map_off);
        constexpr int64_t kChunk = 32ll << 20;
        const int64_t rows_per = std::max<int64_t>(1, kChunk / row_bytes);
        HostPinned ring[2];
        hipEvent_t ev[2] = {nullptr, nullptr};
        bool used[2] = {false, false};
        int32_t err = OSK_OK;
        auto fail = [&](hipError_t e, const char* what) {
            set_error(std::string(what) + ": " + hipGetErrorString(e));
            err = OSK_ERR_DEVICE;
        };
        hipError_t e;
        for (int i = 0; i < 2 && !err; ++i) {
            if ((e = ring[i].reserve((size_t)std::min(n_rows, rows_per) * row_bytes)) != hipSuccess) fail(e, "pinned staging buffer");
            else if ((e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming)) != hipSuccess) fail(e, "staging event");
        }
        if (!err && (e = hipMemset2DAsync(s->d_rows.p, dst_pitch, 0, dst_pitch, n_rows, st)) != hipSuccess)
            fail(e, "hipMemset2DAsync");
        int slot = 0;
        for (int64_t r0 = 0; r0 < n_rows && !err; r0 += rows_per, slot ^= 1) {
            const int64_t cnt = std::min(rows_per, n_rows - r0);
            if (used[slot] && (e = hipEventSynchronize(ev[slot])) != hipSuccess) { fail(e, "hipEventSynchronize"); break; }
            std::memcpy(ring[slot].p, src + r0 * row_bytes, (size_t)(cnt * row_bytes));
            if ((e = hipMemcpy2DAsync(s->d_rows.as<char>() + r0 * dst_pitch, dst_pitch, ring[slot].p, row_bytes,
                                      row_bytes, cnt, hipMemcpyHostToDevice, st)) != hipSuccess) { fail(e, "hipMemcpy2DAsync"); break; }
            if ((e = hipEventRecord(ev[slot], st)) != hipSuccess) { fail(e, "hipEventRecord"); break; }
            used[slot] = true;
        }
        if ((e = hipStreamSynchronize(st)) != hipSuccess && !err) fail(e, "hipStreamSynchronize");
        for (int i = 0; i < 2; ++i)
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        ::munmap(map, map_len);
        if (err) return err;
    }
    rc = seg_finish(s.get(), ord_to_doc, st);
    if (rc) return rc;
    *out = s.release();
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_seg_stage_device(int32_t device, const void* d_rows, int64_t src_pitch_bytes,
                             int64_t n_rows, int32_t dim, int32_t encoding, int32_t similarity,
                             const int32_t* ord_to_doc, int32_t max_doc, osk_seg** out) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(out != nullptr, "out is null");
    OSK_REQUIRE(d_rows != nullptr || n_rows == 0, "d_rows is null");
    std::unique_ptr<osk_seg> s;
    int32_t rc = seg_alloc(device, n_rows, dim, encoding, similarity, max_doc, ord_to_doc, s);
    if (rc) return rc;
    hipStream_t st = device_stream(device);
    const int64_t elem = elem_bytes(encoding);
    OSK_REQUIRE(src_pitch_bytes >= (int64_t)dim * elem, "src_pitch_bytes < dim * element size");
    if (n_rows > 0)
        OSK_HIP(launch_pad_rows(d_rows, src_pitch_bytes, s->d_rows.p, (int64_t)s->units * 16, n_rows,
                                (int64_t)dim * elem, st));
    rc = seg_finish(s.get(), ord_to_doc, st);
    if (rc) return rc;
    *out = s.release();
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_seg_synth(int32_t device, int64_t n_rows, int32_t dim, int32_t encoding,
                      int32_t similarity, uint64_t seed, int32_t dist, int64_t row0,
                      osk_seg** out) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(out != nullptr, "out is null");
    OSK_REQUIRE(dist >= 0 && dist <= 4, "unknown dist");
    OSK_REQUIRE((dist == DIST_INT8) == (encoding == ENC_BYTE), "dist INT8 <=> encoding BYTE");
    OSK_REQUIRE(n_rows <= 0x7FFFFFFFll, "a Lucene segment holds < 2^31 docs");
    std::unique_ptr<osk_seg> s;
    int32_t rc = seg_alloc(device, n_rows, dim, encoding, similarity, (int32_t)n_rows, nullptr, s);
    if (rc) return rc;
    hipStream_t st = device_stream(device);
    if (n_rows > 0)
        OSK_HIP(launch_synth(s->d_rows.p, n_rows, dim, s->units, encoding, seed, dist, row0, st));
    rc = seg_finish(s.get(), nullptr, st);
    if (rc) return rc;
    *out = s.release();
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_seg_release(osk_seg* seg) {
    OSK_GUARD_BEGIN
    if (!seg) return OSK_OK;
    seg_unref(seg);   // freed when no view holds it any more
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_seg_retain(osk_seg* seg) {
    OSK_GUARD_BEGIN
    OSK_REQUIRE(seg != nullptr, "seg is null");
    seg->refs.fetch_add(1);
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_seg_footprint(const osk_seg* seg, int64_t* hbm_bytes) {
    OSK_GUARD_BEGIN
    OSK_REQUIRE(seg != nullptr && hbm_bytes != nullptr, "null argument");
    *hbm_bytes = seg->hbm_bytes();
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_seg_warm(osk_seg* seg, int32_t what) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(seg != nullptr, "seg is null");
    OSK_REQUIRE((what & ~OSK_WARM_ALL) == 0, "unknown warm flags");
    int32_t rc = check_device(seg->device);
    if (rc) return rc;
    if (seg->enc != ENC_FLOAT32) return OSK_OK;   // byte fields scan their rows directly
    hipStream_t st = device_stream(seg->device);
    if (what & (OSK_WARM_PREFILTER | OSK_WARM_PREFILTER_MFMA)) {
        rc = ensure_sq8_seg(seg, st);
        if (rc) return rc;
    }
    if ((what & OSK_WARM_PREFILTER_MFMA) && sq8_mfma_supported((seg->dim + 15) / 16)) {
        rc = ensure_sq8t_seg(seg, st, false);
        if (rc) return rc;
    }
    if (what & OSK_WARM_BATCHED) return ensure_split(seg, st);
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_seg_info(const osk_seg* seg, int64_t* n_rows, int32_t* dim, int32_t* encoding,
                     int32_t* similarity, int32_t* max_doc, int32_t* device) {
    OSK_GUARD_BEGIN
    OSK_REQUIRE(seg != nullptr, "seg is null");
    if (n_rows) *n_rows = seg->n_rows;
    if (dim) *dim = seg->dim;
    if (encoding) *encoding = seg->enc;
    if (similarity) *similarity = seg->sim;
    if (max_doc) *max_doc = seg->max_doc;
    if (device) *device = seg->device;
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_view_create(osk_seg* const* segs, int32_t n_segs, const int32_t* seg_shard,
                        const int32_t* seg_doc_base, int32_t n_shards, const int32_t* shard_index,
                        osk_view** out) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(out != nullptr && segs != nullptr, "null argument");
    OSK_REQUIRE(n_segs >= 1, "need at least one segment");
    OSK_REQUIRE(n_shards >= 1, "need at least one shard");
    const osk_seg* s0 = segs[0];
    OSK_REQUIRE(s0 != nullptr, "null segment");
    for (int i = 0; i < n_segs; ++i) {
        OSK_REQUIRE(segs[i] != nullptr, "null segment");
        OSK_REQUIRE(segs[i]->device == s0->device && segs[i]->dim == s0->dim &&
                        segs[i]->enc == s0->enc && segs[i]->sim == s0->sim,
                    "segments of a view must share device, dim, encoding and similarity");
        const int sh = seg_shard ? seg_shard[i] : 0;
        OSK_REQUIRE(sh >= 0 && sh < n_shards, "seg_shard out of range");
        OSK_REQUIRE(!seg_doc_base || seg_doc_base[i] >= 0, "negative doc base");
    }
    int32_t rc = check_device(s0->device);
    if (rc) return rc;
    auto v = std::make_unique<osk_view>();
    v->device = s0->device;
    v->dim = s0->dim;
    v->enc = s0->enc;
    v->sim = s0->sim;
    v->units = s0->units;
    v->cfg = s0->cfg;
    v->segs.assign(segs, segs + n_segs);
    v->seg_shard.resize(n_segs);
    for (int i = 0; i < n_segs; ++i) v->seg_shard[i] = seg_shard ? seg_shard[i] : 0;
    v->n_shards = n_shards;
    v->shard_index.resize(n_shards);
    for (int s = 0; s < n_shards; ++s) v->shard_index[s] = shard_index ? shard_index[s] : s;

    // tiles: a whole number of "rounds" of the chip's resident workgroup slots (CUs × tile_slots_per_cu;
    // the scan kernels run 4 waves/SIMD = 4 workgroups of 256 threads per CU), so every round is full
    // and no tail round runs with most slots idle (profiles/r01e/tiles_ab.txt: 1.25M rows, 1024 tiles
    // 0.190 ms vs 1221 tiles 0.219 ms).  Rounds grow with the view up to tile_max_rounds; a tile never
    // drops below 8 row-groups per wave nor tile_min_rows rows.
    static const int kL[9] = {4, 8, 8, 16, 16, 16, 32, 64, 64};
    const int R = 64 / kL[v->cfg];
    int64_t total = 0;
    for (int i = 0; i < n_segs; ++i) total += segs[i]->n_rows;
    int64_t min_rows = std::max<int64_t>(4LL * R * 8, (int)g_tuning.tile_min_rows);
    int64_t target = g_tuning.tiles_target;
    if (target <= 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s0->device) != hipSuccess || cus <= 0)
            cus = 256;
        const int64_t slots = (int64_t)cus * std::max(1, (int)g_tuning.tile_slots_per_cu);
        const int64_t rounds = std::min<int64_t>(std::max(1, (int)g_tuning.tile_max_rounds),
                                                 std::max<int64_t>(1, total / (slots * min_rows)));
        target = rounds * slots;
        // large views: whole rounds of BOTH scan kernels' residency.  sq8_scan holds 4 workgroups per
        // CU but sq8_mfma at 32 queries only 3 (LDS), so 4 rounds of 4 slots leave sq8_mfma a third
        // of a tail round.  cus × tile_large_slots tiles (24 = 2 · lcm(3, 4)) are 6 full sq8_scan rounds
        // and 8 full sq8_mfma rounds (profiles/r01l/tiles_ab.txt: C3 b32 2.72 -> 2.47 ms, C4 b32
        // 7.2 -> 6.5 ms, C3 b1 within 1%).
        // Rows of ≥ 512 dims (the 6-bit tier's views, C3/C5i-shaped) take half as many (12 = lcm(3, 4): 3 full
        // sq8_scan rounds, 4 sq8_mfma rounds): their tiles are heavy enough that fewer, fuller workgroups win —
        // the 6-bit tier's pilot, re-bound and settle run over fewer lists (C3 b1 +2.0 % at 4 in flight and one
        // in flight, 3 interleaved A/B pairs, profiles/r05m/), C3 b32 and C5i gained too; C4 b32 (96 dims)
        // lost 9 % with 12 (profiles/r05j/), so lighter rows keep tile_large_slots.
        const int slots_large = v->dim >= 512 ? (int)g_tuning.tile_large_slots_512 : (int)g_tuning.tile_large_slots;
        const int64_t large = (int64_t)cus * slots_large;
        if (slots_large > 0 && total >= large * min_rows) target = large;
        // views smaller than one round at tile_min_rows (C1: 100k rows): latency-bound, so spread them
        // over more of the chip with tiles down to 8 row groups per wave (≥ 256 rows): C1's scan
        // 34 -> 16 µs (profiles/r02o/tile_min_rows.txt); a full round is unaffected (C2: 1024 tiles)
        if (total < slots * min_rows) min_rows = std::max<int64_t>(4LL * R * 8, 256);
    }
    // split the target over segments in proportion to their rows (largest remainder), each segment's
    // share capped so its tiles keep ≥ min_rows rows
    std::vector<int64_t> seg_tiles(n_segs, 0);
    {
        int64_t given = 0;
        std::vector<std::pair<double, int>> rem;
        for (int i = 0; i < n_segs; ++i) {
            const int64_t n = segs[i]->n_rows;
            if (n == 0) continue;
            const double share = total > 0 ? (double)n * (double)target / (double)total : 1.0;
            const int64_t cap = std::max<int64_t>(1, (n + min_rows - 1) / min_rows);
            seg_tiles[i] = std::min<int64_t>(cap, std::max<int64_t>(1, (int64_t)share));
            given += seg_tiles[i];
            rem.push_back({share - (double)(int64_t)share, i});
        }
        std::sort(rem.begin(), rem.end(), [](auto& a, auto& b) { return a.first > b.first || (a.first == b.first && a.second < b.second); });
        for (size_t j = 0; j < rem.size() && given < target; ++j) {
            const int i = rem[j].second;
            const int64_t cap = std::max<int64_t>(1, (segs[i]->n_rows + min_rows - 1) / min_rows);
            if (seg_tiles[i] < cap) { ++seg_tiles[i]; ++given; }
        }
    }
    std::vector<TileDev> tiles;
    v->shard_tile_begin.assign(n_shards + 1, 0);
    for (int sh = 0; sh < n_shards; ++sh) {
        v->shard_tile_begin[sh] = (int32_t)tiles.size();
        for (int i = 0; i < n_segs; ++i) {
            if ((seg_shard ? seg_shard[i] : 0) != sh) continue;
            const int64_t n = segs[i]->n_rows;
            if (n == 0) continue;
            const int64_t nt = seg_tiles[i];
            // balanced split at multiples of 16 rows (sq8_mfma's row groups then start on its tiled
            // copy's 16-row blocks): tile t = rows [⌊n·t/nt⌋₁₆, ⌊n·(t+1)/nt⌋₁₆), the last one ends at n
            auto cut = [&](int64_t t) { return t >= nt ? n : (n * t / nt) & ~(int64_t)15; };
            for (int64_t t = 0; t < nt; ++t)
                if (cut(t + 1) > cut(t)) tiles.push_back(TileDev{i, sh, cut(t), cut(t + 1)});
        }
    }
    v->shard_tile_begin[n_shards] = (int32_t)tiles.size();
    v->n_tiles = (int)tiles.size();
    v->h_tiles = tiles;
    for (const TileDev& td : tiles) v->max_tile_rows = std::max(v->max_tile_rows, td.row_end - td.row_begin);
    // each tile's first row's slot in its shard's candidate region (the select path's collect)
    std::vector<int32_t> tile_coff(std::max<size_t>(1, tiles.size()), 0);
    for (int sh = 0; sh < n_shards; ++sh) {
        int64_t acc = 0;
        for (int t = v->shard_tile_begin[sh]; t < v->shard_tile_begin[sh + 1]; ++t) {
            tile_coff[t] = (int32_t)std::min<int64_t>(acc, INT32_MAX);
            acc += tiles[t].row_end - tiles[t].row_begin;
        }
    }
    OSK_REQUIRE(v->n_tiles < (1 << 24), "too many tiles");
    // dispatch order of the 6-bit scan: tiles interleaved over shards (shard s's j-th of n_s tiles at
    // ≈ (j + ½)/n_s of the grid), so every round of resident workgroups scans a slice of every shard and
    // each shard's floor rises from the first round on (osk_sq6.hip)
    std::vector<int32_t> tile_order(std::max<size_t>(1, tiles.size()), 0);
    {
        std::vector<std::pair<double, int>> key;
        for (int sh = 0; sh < n_shards; ++sh) {
            const int t0 = v->shard_tile_begin[sh], n = v->shard_tile_begin[sh + 1] - t0;
            for (int j = 0; j < n; ++j) key.push_back({(j + 0.5) / n, t0 + j});
        }
        std::stable_sort(key.begin(), key.end(), [](auto& a, auto& b) { return a.first < b.first; });
        for (size_t i = 0; i < key.size(); ++i) tile_order[i] = key[i].second;
    }
    v->h_tile_order = tile_order;

    v->seg_doc_base.resize(n_segs);
    for (int i = 0; i < n_segs; ++i) v->seg_doc_base[i] = seg_doc_base ? seg_doc_base[i] : 0;
    std::vector<int64_t> vrow(n_segs);   // view-global row of each segment's ord 0
    int64_t vacc = 0;
    for (int i = 0; i < n_segs; ++i) {
        vrow[i] = vacc;
        vacc += segs[i]->n_rows;
    }
    OSK_REQUIRE(total < 0xFFFFFFFFll, "a view holds < 2^32 rows");
    std::vector<SegDev> sd = seg_devs(v.get());
    hipStream_t st = device_stream(v->device);
    OSK_HIP(v->d_counters.reserve(sizeof(unsigned long long) * kCtrCount));
    OSK_HIP(hipMemsetAsync(v->d_counters.p, 0, sizeof(unsigned long long) * kCtrCount, st));
    OSK_HIP(v->d_seg_vrow.upload(vrow, st));
    OSK_HIP(v->d_segs.upload(sd, st));
    OSK_HIP(v->d_tiles.upload(tiles, st));
    OSK_HIP(v->d_shard_tile_begin.upload(v->shard_tile_begin, st));
    OSK_HIP(v->d_shard_index.upload(v->shard_index, st));
    OSK_HIP(v->d_tile_coff.upload(tile_coff, st));
    OSK_HIP(v->d_tile_order.upload(tile_order, st));
    OSK_HIP(hipStreamSynchronize(st));
    for (osk_seg* sg : v->segs) sg->refs.fetch_add(1);   // released by ~osk_view
    *out = v.release();
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_view_warm(osk_view* view, int32_t what) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(view != nullptr, "view is null");
    OSK_REQUIRE((what & ~OSK_WARM_ALL) == 0, "unknown warm flags");
    for (osk_seg* s : view->segs) {
        int32_t rc = osk_seg_warm(s, what);
        if (rc) return rc;
    }
    bool all_parents = true;   // the nested search's view tables, once every segment has its parents
    for (osk_seg* s : view->segs) {
        std::lock_guard<std::mutex> lk(s->mu);
        all_parents = all_parents && s->n_parents > 0;
    }
    if ((view->enc != ENC_FLOAT32 || view->n_tiles == 0) && !all_parents) return OSK_OK;
    int32_t rc = check_device(view->device);
    if (rc) return rc;
    hipStream_t st = device_stream(view->device);
    std::lock_guard<std::mutex> lk(view->mu);
    rc = order_after_last(view, st);
    if (rc) return rc;
    if (all_parents && (rc = ensure_nested(view, st)) != OSK_OK) return rc;
    if (view->enc != ENC_FLOAT32 || view->n_tiles == 0) return OSK_OK;
    if (what & (OSK_WARM_PREFILTER | OSK_WARM_PREFILTER_MFMA)) {
        rc = ensure_sq8(view, st);
        if (rc) return rc;
    }
    if ((what & OSK_WARM_PREFILTER_MFMA) && sq8_mfma_supported((view->dim + 15) / 16)) {
        rc = ensure_sq8t(view, st);
        if (rc) return rc;
    }
    if (what & OSK_WARM_BATCHED) return ensure_mfma(view, st);
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_view_release(osk_view* view) {
    OSK_GUARD_BEGIN
    if (!view) return OSK_OK;
    (void)hipSetDevice(view->device);
    delete view;
    return OSK_OK;
    OSK_GUARD_END
}

}  // extern "C"

namespace {

// Scan-kernel timing (osk_view_profile).  The streaming and prefilter scans stamp v->ev0 / v->ev1
// from their own dispatch packets (first and last launch of the call: launch_ev); the MFMA path,
// several launches, brackets them with event records (record = true).
int32_t profile_fold(osk_view* v, int slot) {
    if (!v->ev_pending[slot]) return OSK_OK;
    float ms = 0.f;
    OSK_HIP(hipEventSynchronize(v->ev_stop[slot]));
    OSK_HIP(hipEventElapsedTime(&ms, v->ev_start[slot], v->ev_stop[slot]));
    v->scan_ms += ms;
    v->scan_calls += 1;
    v->ev_pending[slot] = false;
    return OSK_OK;
}

int32_t profile_begin(osk_view* v, hipStream_t st, bool record) {
    const int slot = (int)(v->ev_next++ % osk_view::kEvRing);
    int32_t rc = profile_fold(v, slot);   // the call kEvRing calls ago
    if (rc) return rc;
    v->ev0 = v->ev_start[slot];
    v->ev1 = v->ev_stop[slot];
    v->ev_pending[slot] = false;
    if (record) OSK_HIP(hipEventRecord(v->ev0, st));
    return OSK_OK;
}

// osk_view_profile(N): every N-th call stamps its scan launches (N = 1: every call); the event stamps cost
// a few µs of stream time around the stamped launch, so a long timed loop samples instead of stamping all
int32_t profile_sample(osk_view* v, hipStream_t st, bool record) {
    v->profile = v->profile_every > 0 && v->profile_tick++ % (uint64_t)v->profile_every == 0;
    return v->profile ? profile_begin(v, st, record) : OSK_OK;
}

int32_t profile_end(osk_view* v, hipStream_t st, bool record) {
    if (!v->profile) return OSK_OK;
    if (record) OSK_HIP(hipEventRecord(v->ev1, st));
    v->ev_pending[(v->ev_next - 1) % osk_view::kEvRing] = true;
    return OSK_OK;
}

// (start, stop) events for launch q0 of a call that launches [0, nq) in chunks of `chunk` queries
inline hipEvent_t launch_ev_start(const osk_view* v, int q0) { return v->profile && q0 == 0 ? v->ev0 : nullptr; }
inline hipEvent_t launch_ev_stop(const osk_view* v, int q0, int nq, int chunk = kMaxNQ) {
    return v->profile && q0 + chunk >= nq ? v->ev1 : nullptr;
}

// Nothing staged: every shard returns zero hits.
int32_t zero_shard_hits(const osk_view* v, int nq, int k, uint64_t* d_shard_keys, int32_t* d_shard_counts,
                        int64_t* d_visited, hipStream_t st) {
    OSK_HIP(hipMemsetAsync(d_shard_keys, 0, sizeof(uint64_t) * nq * v->n_shards * k, st));
    OSK_HIP(hipMemsetAsync(d_shard_counts, 0, sizeof(int32_t) * nq * v->n_shards, st));
    if (d_visited) OSK_HIP(hipMemsetAsync(d_visited, 0, sizeof(int64_t) * v->segs.size(), st));
    return OSK_OK;
}

// Streaming exact scan of queries already in the padded unit layout (≤ 8 per launch) + per-shard merge.
int32_t stream_search(osk_view* v, const void* qpad, const void* qnorm, int nq, int k, int UP,
                      const uint64_t* const* d_accept, uint64_t* d_shard_keys, int32_t* d_shard_counts,
                      int64_t* d_visited, hipStream_t st) {
    OSK_HIP(v->ws_cand.reserve(sizeof(uint64_t) * (size_t)nq * v->n_tiles * k));
    HamParams p{};   // (a Hamming view's launches read q_units; every other launch takes the ScanParams base)
    p.q_units = UP;
    p.segs = v->d_segs.as<SegDev>();
    p.tiles = v->d_tiles.as<TileDev>();
    p.accept = d_accept;
    p.cand = v->ws_cand.as<uint64_t>();
    p.visited = reinterpret_cast<unsigned long long*>(d_visited);
    p.n_tiles = v->n_tiles;
    p.units = v->units;
    p.k = k;
    p.sim = v->sim;
    p.dim = v->dim;
    for (int q0 = 0; q0 < nq; q0 += kMaxNQ) {
        const int qc = std::min(kMaxNQ, nq - q0);
        p.q0 = q0;
        p.q_count = qc;
        p.q = static_cast<const char*>(qpad) + (size_t)q0 * UP * 16;
        p.qnorm_f = static_cast<const float*>(qnorm) + q0;
        p.qnorm_i = static_cast<const int32_t*>(qnorm) + q0;
        if (v->sim == SIM_HAMMING)   // packed bits: osk_hamming.hip's scans (no norms; their own lane configs)
            OSK_HIP(launch_scan_ham(qc, p, st, launch_ev_start(v, q0), launch_ev_stop(v, q0, nq)));
        else
            OSK_HIP(launch_scan(v->enc, v->cfg, qc, p, st, launch_ev_start(v, q0), launch_ev_stop(v, q0, nq)));
    }
    int32_t rc = profile_end(v, st, false);
    if (rc) return rc;
    OSK_HIP(launch_merge_shards(v->ws_cand.as<uint64_t>(), v->n_tiles,
                                v->d_shard_tile_begin.as<int32_t>(), v->n_shards, nq, k,
                                d_shard_keys, d_shard_counts, st));
    return OSK_OK;
}

// Batched search: MFMA candidates → per-shard approx top-k' → exact re-score + certificate →
// exact streaming scan for any query whose certificate failed.  ws_q / ws_qnorm hold the padded
// queries and their |q|² in the device lane order.
int32_t batched_search(osk_view* v, int nq, int k, int UP, const uint64_t* const* d_accept,
                       uint64_t* d_shard_keys, int32_t* d_shard_counts, int64_t* d_visited, hipStream_t st) {
    int32_t rc = ensure_mfma(v, st);
    if (rc) return rc;
    const int S = v->n_shards, KS = v->mfma_KS;
    const int n_qb = (nq + 255) / 256;
    const int nq_pad = n_qb * 256;
    OSK_HIP(v->ws_qsplit.reserve((size_t)(nq_pad / 16) * KS * 2 * 1024));
    OSK_HIP(launch_split_rows(v->ws_q.as<float4>(), nq, UP, KS, nq_pad / 16, v->ws_qsplit.p, st));
    OSK_HIP(v->ws_cand_a.reserve(sizeof(uint64_t) * (size_t)nq * v->n_munits * 2 * kKC));
    MfmaParams mp{};
    mp.segs = v->d_segs.as<SegDev>();
    mp.units = v->d_munits.as<MfmaUnit>();
    mp.seg_split = v->d_seg_split.as<const void*>();
    mp.xsqrt = v->d_seg_xsqrt.as<const float*>();
    mp.accept = d_accept;
    mp.qsplit = v->ws_qsplit.p;
    mp.qnorm = v->ws_qnorm.as<float>();
    mp.cand = v->ws_cand_a.as<uint64_t>();
    mp.visited = reinterpret_cast<unsigned long long*>(d_visited);
    mp.n_units = v->n_munits;
    mp.KS = KS;
    mp.nq = nq;
    mp.nq_pad = std::min(nq_pad, (int)(v->ws_qnorm.cap / sizeof(float)));
    mp.sim = v->sim;
    mp.ablate = g_tuning.mfma_ablate;
    if (!v->d_mfma_full.p) {
        OSK_HIP(v->d_mfma_full.reserve(sizeof(unsigned long long)));
        OSK_HIP(hipMemsetAsync(v->d_mfma_full.p, 0, sizeof(unsigned long long), st));
    }
    mp.full_tiles = v->d_mfma_full.as<unsigned long long>();
    mp.n_shards = S;
    OSK_HIP(v->ws_akeys.reserve(sizeof(uint64_t) * (size_t)nq * S * kKC));
    OSK_HIP(v->ws_acounts.reserve(sizeof(int32_t) * (size_t)nq * S));
    if (!(g_tuning.mfma_ablate & 16)) {
        // pilot: the first tile of every unit, merged per (query, shard) → k'-th approx score =
        // a threshold no row below which can reach the shard's top-k'
        OSK_HIP(v->ws_pkeys.reserve(sizeof(uint64_t) * (size_t)nq * S * kKC));
        OSK_HIP(v->ws_pcounts.reserve(sizeof(int32_t) * (size_t)nq * S));
        MfmaParams pp = mp;
        pp.visited = nullptr;
        OSK_HIP(launch_mfma_cand(pp, n_qb, true, st));
        OSK_HIP(launch_merge_shards(v->ws_cand_a.as<uint64_t>(), v->n_munits * 2, v->d_shard_unit_begin.as<int32_t>(),
                                    S, nq, kKC, v->ws_pkeys.as<uint64_t>(), v->ws_pcounts.as<int32_t>(), st));
        mp.thr_keys = v->ws_pkeys.as<uint64_t>();
        mp.thr_counts = v->ws_pcounts.as<int32_t>();
    }
    OSK_HIP(launch_mfma_cand(mp, n_qb, false, st));
    rc = profile_end(v, st, true);
    if (rc) return rc;
    OSK_HIP(launch_merge_shards(v->ws_cand_a.as<uint64_t>(), v->n_munits * 2, v->d_shard_unit_begin.as<int32_t>(),
                                S, nq, kKC, v->ws_akeys.as<uint64_t>(), v->ws_acounts.as<int32_t>(), st));
    OSK_HIP(v->ws_flags.reserve(sizeof(int) * nq));
    OSK_HIP(hipMemsetAsync(v->ws_flags.p, 0, sizeof(int) * nq, st));
    RescoreParams rp{};
    rp.segs = v->d_segs.as<SegDev>();
    rp.seg_vrow_begin = v->d_seg_vrow.as<int64_t>();
    rp.akeys = v->ws_akeys.as<uint64_t>();
    rp.q = v->ws_q.p;
    rp.qnorm_dev = v->ws_qnorm.as<float>();
    rp.qnorm_approx = v->ws_qnorm.as<float>();
    rp.shard_maxnorm2 = v->d_shard_maxnorm2.as<float>();
    rp.shard_keys = d_shard_keys;
    rp.shard_counts = d_shard_counts;
    rp.flags = v->ws_flags.as<int>();
    rp.c = v->mfma_c;
    rp.n_shards = S;
    rp.n_segs = (int)v->segs.size();
    rp.units = v->units;
    rp.k = k;
    rp.sim = v->sim;
    OSK_HIP(launch_rescore(v->cfg, nq, rp, st));
    // certificate failures → exact streaming scan of those queries (rare; needs the flags on host)
    OSK_HIP(v->h_flags.reserve(sizeof(int) * nq));
    OSK_HIP(hipMemcpyAsync(v->h_flags.p, v->ws_flags.p, sizeof(int) * nq, hipMemcpyDeviceToHost, st));
    OSK_HIP(hipStreamSynchronize(st));
    const int* fl = static_cast<const int*>(v->h_flags.p);
    std::vector<int> fail;
    for (int q = 0; q < nq; ++q)
        if (fl[q]) fail.push_back(q);
    v->mfma_calls += 1;
    v->mfma_fallback_queries += (int64_t)fail.size();
    if (fail.empty() || g_tuning.mfma_ablate) return OSK_OK;
    const int nf = (int)fail.size();
    const int nf_pad = (nf + kMaxNQ - 1) / kMaxNQ * kMaxNQ;
    OSK_HIP(v->ws_fbq.reserve((size_t)nf_pad * UP * 16 + sizeof(float) * nf_pad));
    OSK_HIP(hipMemsetAsync(v->ws_fbq.p, 0, (size_t)nf_pad * UP * 16 + sizeof(float) * nf_pad, st));
    char* fbq = v->ws_fbq.as<char>();
    float* fbn = reinterpret_cast<float*>(fbq + (size_t)nf_pad * UP * 16);
    for (int i = 0; i < nf; ++i) {
        OSK_HIP(hipMemcpyAsync(fbq + (size_t)i * UP * 16, v->ws_q.as<char>() + (size_t)fail[i] * UP * 16,
                               (size_t)UP * 16, hipMemcpyDeviceToDevice, st));
        OSK_HIP(hipMemcpyAsync(fbn + i, v->ws_qnorm.as<float>() + fail[i], sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    OSK_HIP(v->ws_fbkeys.reserve(sizeof(uint64_t) * (size_t)nf * S * k));
    OSK_HIP(v->ws_fbcounts.reserve(sizeof(int32_t) * (size_t)nf * S));
    const bool prof = v->profile;
    v->profile = false;
    rc = stream_search(v, fbq, fbn, nf, k, UP, d_accept, v->ws_fbkeys.as<uint64_t>(),
                       v->ws_fbcounts.as<int32_t>(), nullptr, st);
    v->profile = prof;
    if (rc) return rc;
    for (int i = 0; i < nf; ++i) {
        OSK_HIP(hipMemcpyAsync(d_shard_keys + (size_t)fail[i] * S * k, v->ws_fbkeys.as<uint64_t>() + (size_t)i * S * k,
                               sizeof(uint64_t) * S * k, hipMemcpyDeviceToDevice, st));
        OSK_HIP(hipMemcpyAsync(d_shard_counts + (size_t)fail[i] * S, v->ws_fbcounts.as<int32_t>() + (size_t)i * S,
                               sizeof(int32_t) * S, hipMemcpyDeviceToDevice, st));
    }
    return OSK_OK;
}

// The 6-bit tier's calibration, folded without waiting: when this view's last probe has
// landed (its event completed), its per-segment int8 re-bound counts join the segments' calibration; a
// segment with kSq6Probes probes keeps the tier, or turns it off (re-bounds above sq6_probe_pct % of the
// rows probed) and frees its 6-bit copy — stream-ordered, with no host or device-wide wait:
//  * only a probing segment (state 0) can turn off, so only launches issued while some segment of the view
//    probes register an event (sq6_track_launch); a kept segment (state 1) never frees its copy early;
//  * a search holds the shared side of g_sq6_free_mu from its state check to that registration, so once the
//    freeing call holds the exclusive side (briefly: no waiting under it) every launch that may read the
//    copy is registered, and every later search sees state 2 and leaves the tier alone;
//  * the freeing call's stream waits on the events of the registered launches still in flight over the
//    segment (other views' streams included), then hipFreeAsync releases the copy on that stream.
std::shared_mutex g_sq6_free_mu;
struct Sq6Inflight {
    int device;
    hipEvent_t ev;
    std::vector<const osk_seg*> segs;
};
std::mutex g_sq6_inflight_mu;                       // (inner to g_sq6_free_mu)
std::vector<Sq6Inflight> g_sq6_inflight;            // launches over probing segments, not yet seen complete
std::vector<std::pair<int, hipEvent_t>> g_sq6_ev_pool;

// (g_sq6_inflight_mu held) drop the entries whose launches have completed; their events go back to the pool
void sq6_prune_locked() {
    size_t j = 0;
    for (size_t i = 0; i < g_sq6_inflight.size(); ++i) {
        if (hipEventQuery(g_sq6_inflight[i].ev) == hipSuccess)
            g_sq6_ev_pool.push_back({g_sq6_inflight[i].device, g_sq6_inflight[i].ev});
        else
            g_sq6_inflight[j++] = std::move(g_sq6_inflight[i]);
    }
    g_sq6_inflight.resize(j);
}

}  // namespace

// A segment being destroyed leaves the in-flight records (its launches have completed: the destructor waits for
// the device before it calls this), so a segment later allocated at the same address never waits on them.
void osk::sq6_forget_segment(const osk_seg* sg) {
    std::lock_guard<std::mutex> lk(g_sq6_inflight_mu);
    for (Sq6Inflight& f : g_sq6_inflight) f.segs.erase(std::remove(f.segs.begin(), f.segs.end(), sg), f.segs.end());
    sq6_prune_locked();
}

namespace {

// A 6-bit launch over a view with a probing segment: record its completion (caller holds the shared side
// of g_sq6_free_mu, and the view's device is current).
int32_t sq6_track_launch(const osk_view* v, hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_sq6_inflight_mu);
    sq6_prune_locked();
    hipEvent_t ev = nullptr;
    for (size_t i = 0; i < g_sq6_ev_pool.size(); ++i)
        if (g_sq6_ev_pool[i].first == v->device) {
            ev = g_sq6_ev_pool[i].second;
            g_sq6_ev_pool.erase(g_sq6_ev_pool.begin() + (ptrdiff_t)i);
            break;
        }
    if (!ev) OSK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, st);
    if (e != hipSuccess) {
        g_sq6_ev_pool.push_back({v->device, ev});
        OSK_HIP(e);
    }
    g_sq6_inflight.push_back(Sq6Inflight{v->device, ev, std::vector<const osk_seg*>(v->segs.begin(), v->segs.end())});
    return OSK_OK;
}

int32_t fold_probe(osk_view* v, hipStream_t st) {
    if (!v->probe_pending || hipEventQuery(v->ev_probe) != hipSuccess) return OSK_OK;
    v->probe_pending = false;
    const unsigned long long* rb = static_cast<const unsigned long long*>(v->h_seg_rebound.p);
    std::vector<osk_seg*> off;
    for (size_t i = 0; i < v->segs.size(); ++i) {
        osk_seg* sg = v->segs[i];
        std::lock_guard<std::mutex> lk(sg->mu);
        if (sg->sq6_state.load() != 0) continue;
        sg->sq6_probe_rows += sg->n_rows;
        sg->sq6_probe_rebound += (int64_t)rb[i];
        if (++sg->sq6_probes < kSq6Probes) continue;
        const bool keep = (double)sg->sq6_probe_rebound * 100.0 <=
                          (double)sg->sq6_probe_rows * (double)g_tuning.sq6_probe_pct;
        sg->sq6_state.store(keep ? 1 : 2, std::memory_order_release);
        if (!keep) off.push_back(sg);
    }
    if (off.empty()) return OSK_OK;
    std::unique_lock<std::shared_mutex> ex(g_sq6_free_mu);
    std::lock_guard<std::mutex> lk(g_sq6_inflight_mu);
    sq6_prune_locked();
    for (const Sq6Inflight& f : g_sq6_inflight) {
        bool reads = false;
        for (const osk_seg* sg : off) reads = reads || std::find(f.segs.begin(), f.segs.end(), sg) != f.segs.end();
        if (reads) OSK_HIP(hipStreamWaitEvent(st, f.ev, 0));
    }
    for (osk_seg* sg : off) {
        std::lock_guard<std::mutex> sl(sg->mu);
        if (sg->d_q6) OSK_HIP(hipFreeAsync(sg->d_q6, st));
        if (sg->d_q6aux) OSK_HIP(hipFreeAsync(sg->d_q6aux, st));
        sg->d_q6 = nullptr;
        sg->d_q6aux = nullptr;
    }
    return OSK_OK;
}

// The prefilter's two int8 MFMA kernels, in µs for this view's R rows (measured end to end on MI355X,
// DESIGN.md §3c): sq8_mfma per launch of ≤ 32 queries streams R·(int8 row + 16-B bound terms) at ≈ 4.3 TB/s
// + ≈ 165 µs + 0.28 µs per dim (pilot, merge, settle, re-score); the wide kernel per launch of ≤ 256 queries
// ≈ R·KS·0.031 ns (it is issue-bound, not HBM-bound: C4 6.35 ms per 256 at b1024, C3 4.07 ms at b256, round 5
// with deferred insertions, profiles/r05d/) + ≈ 300 µs (pilot, two passes, floors, settle: C2 0.33 ms per 256).
double sq8_narrow_us(double R, int nq, int u8, int dim) {
    return (double)((nq + 31) / 32) * (R * (16.0 * u8 + 16.0) / 4.3e6 + 165.0 + 0.28 * dim);
}
double sq8_wide_us(double R, int nq, int u8) {
    return (double)((nq + kWideQ - 1) / kWideQ) * (R * sq8_wide_ks(u8) * 0.031e-3 + 300.0);
}
// the wide kernel takes an unfiltered batch of ≥ sq8_wide_min queries of ≤ 768 dims when the model has it
// cheaper than sq8_mfma (C4: from about 96 queries)
bool sq8_wide_pick(const osk_view* v, int nq, bool filtered) {
    const int u8 = (v->dim + 15) / 16;
    if (filtered || !sq8_wide_supported(u8) || g_tuning.sq8_wide_min <= 0 || nq < g_tuning.sq8_wide_min ||
        g_tuning.sq8_mfma_min <= 0 || nq < g_tuning.sq8_mfma_min)
        return false;
    double R = 0.0;
    for (const osk_seg* sg : v->segs) R += (double)sg->n_rows;
    return g_tuning.sq8_wide_force || sq8_wide_us(R, nq, u8) <= sq8_narrow_us(R, nq, u8, v->dim);
}

// The wide kernels' pilot rows per quarter (tune sq8_wide_pilot_rows; 0: 128, 256 at ≥ 512 dims, where the
// pilot's steps are 32 rows and the better floors pay: C3 b256 3.76 → 3.71 ms, C4's 96 dims 22.98 → 23.27 ms,
// profiles/r05p/tune50_*).
// At least ≈ 64k pilot rows per shard: the floor is the k-th best of the shard's quarter maxima, so a
// shard of few quarters (6.5M rows over 8 shards: 64 quarters of 12.7k rows) sampled at 128 rows a
// quarter floored the first pass at ≈ its 1,000th best row, and the rows kernel's queues overflowed for
// every query (exact re-scans of the overflowed quarters); up to 1,024 rows a quarter.
int sq8_wide_pilot_rows(const osk_view* v) {
    const int prows = g_tuning.sq8_wide_pilot_rows.load();
    if (prows > 0) return prows;
    const int pr = sq8_wide_ks(v->units8) >= 8 ? 256 : kWidePilotRowsDefault;
    const int qps = std::max(1, 4 * v->n_wtiles / std::max(1, v->n_shards));   // quarters per shard
    const int want = (kWidePilotSample + qps - 1) / qps;
    return std::max(pr, std::min(1024, (want + 127) / 128 * 128));
}
// The wide kernels' two passes: the first 1/phase of the nql quarters (tile order: every shard) under the
// pilot's floors, then the rest under floors raised by the first pass's list maxima.  Returns the first
// pass's quarters (0: one pass).
// (the first pass takes whole rounds of the persistent grid, at least one: a small view's 1/phase
// would idle the chip, and a partial round leaves a tail)
int sq8_wide_first_pass(int nql, int wgrid) {
    const int phase = g_tuning.sq8_wide_phase;
    const int rounds = std::max(1, (int)std::lround((double)nql / ((double)phase * wgrid)));
    return phase > 1 ? std::min(nql / 2, rounds * wgrid) : 0;
}

// ---- Share groups of the 6-bit tier: views over one segment set with equal tile tables (a
// searcher's add_view views, a view's leased replicas) whose single queries in flight are served by shared
// corpus passes (osk_sq6.hip sq6_scan_shared).  A group is a ref-counted registry entry keyed by the device,
// the ordered segment list, the tile table and its dispatch order; it owns kShareSlots slots on the device (the
// posted queries) and a word per (slot, tile) carrying the generation whose tile is done.  Its scans are
// chained: each waits, on its own stream, for the event of the one enqueued before it (the group mutex covers
// wait, launch and record), so no scan sees another's tile half done and nothing is cleared per call. ----
// The registry's key: two views share only if all of this compares equal.
struct Sq6ShareKey {
    int device = 0, n_shards = 0, dim = 0, sim = 0;
    std::vector<const osk_seg*> segs;
    std::vector<TileDev> tiles;
    std::vector<int32_t> order;
    bool operator==(const Sq6ShareKey& o) const {
        if (device != o.device || n_shards != o.n_shards || dim != o.dim || sim != o.sim || segs != o.segs ||
            order != o.order || tiles.size() != o.tiles.size())
            return false;
        for (size_t i = 0; i < tiles.size(); ++i)
            if (tiles[i].seg != o.tiles[i].seg || tiles[i].shard != o.tiles[i].shard ||
                tiles[i].row_begin != o.tiles[i].row_begin || tiles[i].row_end != o.tiles[i].row_end)
                return false;
        return true;
    }
};
struct Sq6Group {
    Sq6ShareKey key;
    std::mutex mu;                       // slots, generations, the event chain
    int attached = 0;
    bool used[kShareSlots] = {};
    uint32_t gen[kShareSlots] = {};      // the last generation each slot posted (kept across owners: a word of an
    unsigned long long seq = 0;          // earlier owner never equals a later generation)
    hipEvent_t last = nullptr;           // the last shared scan enqueued
    bool has_last = false;
    Sq6Slot* d_slots = nullptr;
    uint32_t* d_done = nullptr;          // [kShareSlots][n_tiles]
};
std::mutex g_sq6_groups_mu;              // the registry (outer to a group's mu)
std::vector<Sq6Group*> g_sq6_groups;

// Join the view's group (created on first use) and take a slot; a view that finds none does not share
// (caller holds v->mu; the view's device is current).
int32_t sq6_share_attach(osk_view* v) {
    Sq6ShareKey key{v->device, v->n_shards, v->dim, v->sim, {v->segs.begin(), v->segs.end()}, v->h_tiles, v->h_tile_order};
    std::lock_guard<std::mutex> reg(g_sq6_groups_mu);
    Sq6Group* grp = nullptr;
    for (Sq6Group* c : g_sq6_groups)
        if (c->key == key) grp = c;
    if (!grp) {
        auto fresh = std::make_unique<Sq6Group>();
        fresh->key = std::move(key);
        const size_t words = (size_t)kShareSlots * std::max(1, v->n_tiles);
        OSK_HIP(hipMalloc(&fresh->d_slots, sizeof(Sq6Slot) * kShareSlots));
        hipError_t e = hipMalloc(&fresh->d_done, sizeof(uint32_t) * words);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&fresh->last, hipEventDisableTiming);
        if (e == hipSuccess) e = hipMemset(fresh->d_slots, 0, sizeof(Sq6Slot) * kShareSlots);
        if (e == hipSuccess) e = hipMemset(fresh->d_done, 0, sizeof(uint32_t) * words);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);   // (the fills land before any stream posts)
        if (e != hipSuccess) {
            (void)hipFree(fresh->d_slots);
            if (fresh->d_done) (void)hipFree(fresh->d_done);
            if (fresh->last) (void)hipEventDestroy(fresh->last);
            OSK_HIP(e);
        }
        grp = fresh.release();
        g_sq6_groups.push_back(grp);
    }
    std::lock_guard<std::mutex> lk(grp->mu);
    for (int s = 0; s < kShareSlots; ++s)
        if (!grp->used[s]) {
            grp->used[s] = true;
            grp->attached += 1;
            v->share_group = grp;
            v->share_slot = s;
            break;
        }
    v->share_tried = true;   // (a failed allocation above leaves the view free to try again)
    return OSK_OK;
}

// Withdraw a slot's posted query (caller holds grp->mu, which keeps later scans out; the group's device is
// current): behind the group's last pass, which may be reading the query or writing its view's lists, the
// slot's generation word is cleared so no later pass reads the descriptor.
void sq6_share_withdraw(Sq6Group* grp, int slot) {
    if (grp->has_last) (void)hipEventSynchronize(grp->last);
    (void)hipMemset(&grp->d_slots[slot].gen, 0, sizeof(uint32_t));
    (void)hipStreamSynchronize(nullptr);
}

}  // namespace

// Leave the group: after its last scan has completed the view's query is withdrawn; the group goes with its
// last view.
void osk::sq6_share_detach(osk_view* v) {
    Sq6Group* grp = static_cast<Sq6Group*>(v->share_group);
    if (!grp) return;
    int cur = -1;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(grp->key.device);
    {
        // the group lock keeps later scans out while the last one drains and the slot is cleared; the registry
        // lock is not held over the wait, so other groups attach and detach meanwhile (the group itself stays:
        // this view is still attached)
        std::lock_guard<std::mutex> lk(grp->mu);
        sq6_share_withdraw(grp, v->share_slot);
    }
    bool last_view = false;
    {
        std::lock_guard<std::mutex> reg(g_sq6_groups_mu);
        std::lock_guard<std::mutex> lk(grp->mu);
        grp->used[v->share_slot] = false;
        last_view = --grp->attached == 0;
        if (last_view) g_sq6_groups.erase(std::remove(g_sq6_groups.begin(), g_sq6_groups.end(), grp), g_sq6_groups.end());
    }
    v->share_group = nullptr;
    v->share_slot = -1;
    if (last_view) {   // (off the registry: no view can find it any more)
        (void)hipFree(grp->d_slots);
        (void)hipFree(grp->d_done);
        (void)hipEventDestroy(grp->last);
        delete grp;
    }
    if (cur >= 0) (void)hipSetDevice(cur);
}

namespace {

// ---- Certified int8 prefilter search (float32, k ≤ kKQ): int8 scan → settle per slice of tiles (exact
// re-score of the rows the certificate cannot exclude; a tile whose list overflowed is re-scanned
// exactly inside the settle) → per-shard merge.  Nothing waits on the host.  sq8_search decides on one of
// four scans (sq8_decide), prepares the queries, runs the scan (scan_valu, scan_mfma, scan_wide, scan_sq6:
// each with its own copies, workspace and parameter block) and settles the lists the scan reports. ----
enum class Sq8Strategy { kValu, kMfma, kWide, kSq6 };
struct Sq8Plan {
    Sq8Strategy strategy;
    bool gather;    // kValu: a filtered scan over the compacted accepted ordinals
    bool probing;   // kSq6: some segment is still calibrating the tier (it may yet turn it off)
    bool probe6;    // kSq6: this call counts its int8 re-bounds per segment (one probe in flight per view)
    bool share;     // kSq6: the view's share group has another view: post the query and take the shared pass
};
// one search call's arguments
struct Sq8Call {
    osk_view* v;
    int nq, k;
    const uint64_t* const* d_accept;
    uint64_t* d_shard_keys;
    int32_t* d_shard_counts;
    int64_t* d_visited;
    hipStream_t st;
};
// What a scan reports to the settle: its wave lists (ws_sq8cand, ws_sq8lb, ws_lbmax), the rows per
// wave-iteration that split a tile among its waves, and the tile and slice tables the lists are over.
struct Sq8Lists {
    int n_lists;
    int scan_R;
    const TileDev* tiles;                    // (exact re-scan of an overflowed list)
    const int4* slices;
    const int32_t* shard_slice_begin;
    int n_slices;
    GatherSplit gather;                      // gather scans: the scan's split
    const int32_t* wide_shard_tile_begin;    // wide scans: one settle workgroup per (shard, query); else null
};

// Batches of ≥ sq8_mfma_min queries: the int8 MFMA scan, ≤ 32 queries per launch — large unfiltered batches
// of ≤ 768-dim rows on the wide kernels when the cost model picked them (wide_pick: sq8_wide_pick), one
// corpus pass per kWideQ queries (osk_sq8w.hip); else the VALU scan, ≤ 8 per launch, filtered ones over the
// compacted accepted ordinals.  A single unfiltered query scans the 6-bit tier where the view has one
// (DESIGN.md §3f): every segment's calibration probing or on.  The shared lock is taken for that check and
// keeps a segment's copy alive from it to the launches (fold_probe frees it under the exclusive one, with
// hipFreeAsync behind the events of the launches still reading it: no device wait).
Sq8Plan sq8_decide(const osk_view* v, int nq, bool filtered, bool wide_pick,
                   std::shared_lock<std::shared_mutex>& tier_lock) {
    Sq8Plan plan{Sq8Strategy::kValu, false, false, false, false};
    if (g_tuning.sq8_mfma_min > 0 && nq >= g_tuning.sq8_mfma_min && sq8_mfma_supported(v->units8)) {
        plan.strategy = !g_tuning.sq8_force_fallback && wide_pick ? Sq8Strategy::kWide : Sq8Strategy::kMfma;
        return plan;
    }
    bool use6 = nq == 1 && !filtered && v->sq6_ready && g_tuning.sq6;
    if (use6) {
        tier_lock.lock();
        for (const osk_seg* sg : v->segs) {
            const int st6 = sg->sq6_state.load(std::memory_order_acquire);
            use6 = use6 && st6 != 2 && sg->d_q6;
            plan.probing |= st6 == 0;
        }
    }
    if (use6) {
        plan.strategy = Sq8Strategy::kSq6;
        plan.probe6 = plan.probing && !v->probe_pending;
    } else {
        plan.probing = false;
        plan.gather = filtered && g_tuning.filter_gather;
    }
    return plan;
}

// The 6-bit tier's share of the prologue: a probe call's per-segment re-bound counts (zeroed), and the
// tier's query form and floor buckets for the fused prep to fill.
int32_t sq6_prep(osk_view* v, int nq_pad, bool probe6, hipStream_t st, Sq6Prep& q6) {
    const size_t ns = v->segs.size();
    if (probe6) {
        OSK_HIP(v->d_seg_rebound.reserve(sizeof(unsigned long long) * ns));
        OSK_HIP(v->h_seg_rebound.reserve(sizeof(unsigned long long) * ns));
        if (!v->ev_probe) OSK_HIP(hipEventCreateWithFlags(&v->ev_probe, hipEventDisableTiming));
        OSK_HIP(hipMemsetAsync(v->d_seg_rebound.p, 0, sizeof(unsigned long long) * ns, st));
    }
    q6.C = sq6_chunks(v->dim);
    q6.floor_n = v->n_shards * (kFloorBuckets + 1) * kFloorStride;   // buckets + the floor cell per shard
    OSK_HIP(v->ws_q6.reserve((size_t)nq_pad * 256 * q6.C));
    OSK_HIP(v->ws_qc6.reserve(sizeof(float4) * nq_pad));
    OSK_HIP(v->ws_floor.reserve(sizeof(uint32_t) * (size_t)nq_pad * q6.floor_n));
    q6.q6 = v->ws_q6.as<uint32_t>();
    q6.qc6 = v->ws_qc6.as<float4>();
    q6.floor = v->ws_floor.as<uint32_t>();
    return OSK_OK;
}

// One launch: padded fp32 queries (ws_q), |q|² (device order, ws_qnorm), int8 queries + bound terms (and the
// 6-bit tier's query form, floor buckets zeroed), flags = 0.
int32_t sq8_prep_queries(const Sq8Call& c, const void* d_queries, int UP, const Sq8Plan& plan) {
    osk_view* v = c.v;
    const int u8 = v->units8, nq_pad = (c.nq + kMaxNQ - 1) / kMaxNQ * kMaxNQ;
    Sq6Prep q6{};
    if (plan.strategy == Sq8Strategy::kSq6) {
        const int32_t rc = sq6_prep(v, nq_pad, plan.probe6, c.st, q6);
        if (rc) return rc;
    }
    OSK_HIP(v->ws_q8.reserve((size_t)nq_pad * u8 * 16));
    OSK_HIP(v->ws_qc.reserve(sizeof(float4) * nq_pad));
    OSK_HIP(v->ws_flags.reserve(sizeof(int) * c.nq));
    OSK_HIP(launch_sq8_prep(v->cfg, static_cast<const float*>(d_queries), v->dim, c.nq, nq_pad, UP, u8,
                            v->ws_q.as<float4>(), v->ws_qnorm.as<float>(), v->ws_q8.p, v->ws_qc.as<float4>(),
                            v->ws_flags.as<int>(), c.st, q6));
    return OSK_OK;
}

// The wave lists of a scan over n_tiles tiles (4 per tile and query), the fields every strategy's kernels
// share, and the report of a scan over the view's own tiles.
int32_t sq8_lists(const Sq8Call& c, int n_tiles, int scan_R, Sq8Common& p, Sq8Lists& out) {
    osk_view* v = c.v;
    const size_t nl = (size_t)c.nq * 4 * n_tiles * kKQ;
    OSK_HIP(v->ws_sq8cand.reserve(sizeof(uint64_t) * nl));
    OSK_HIP(v->ws_sq8lb.reserve(sizeof(uint32_t) * nl));
    OSK_HIP(v->ws_lbmax.reserve(sizeof(uint32_t) * (size_t)c.nq * 4 * n_tiles));
    p.segs = v->d_segs.as<SegDev>();
    p.tiles = v->d_tiles.as<TileDev>();
    p.accept = c.d_accept;
    p.rows8 = v->d_sq8_rows.as<const int4*>();
    p.aux = v->d_sq8_aux.as<const float4*>();
    p.seg_vrow = v->d_seg_vrow.as<int64_t>();
    p.cand = v->ws_sq8cand.as<uint64_t>();
    p.cand_lb = v->ws_sq8lb.as<uint32_t>();
    p.list_lbmax = v->ws_lbmax.as<uint32_t>();
    p.visited = reinterpret_cast<unsigned long long*>(c.d_visited);
    p.n_tiles = n_tiles;
    p.n_lists = 4 * n_tiles;
    v->sq8_lists_last = p.n_lists;
    p.units8 = v->units8;
    p.sim = v->sim;
    p.gam = v->sq8_gam;
    p.g2 = v->sq8_g2;
    p.cos_slack = v->sq8_cos_slack;
    p.k = c.k;
    p.n_shards = v->n_shards;
    p.counters = v->d_counters.as<unsigned long long>();
    p.ablate = g_tuning.sq8_mfma_ablate;
    out = Sq8Lists{p.n_lists, scan_R, p.tiles, v->d_slices.as<int4>(), v->d_shard_slice_begin.as<int32_t>(),
                   v->n_slices, GatherSplit{}, nullptr};
    return OSK_OK;
}
// ...and the launch's queries [q0, q0 + chunk) of nq
void sq8_chunk(const osk_view* v, Sq8Common& p, int q0, int chunk, int nq) {
    p.q0 = q0;
    p.q_count = std::min(chunk, nq - q0);
    p.q8 = v->ws_q8.as<int4>() + (size_t)q0 * v->units8;
    p.qc = v->ws_qc.as<float4>() + q0;
    p.qn_dev = v->ws_qnorm.as<float>() + q0;
}

// The VALU scan, ≤ kMaxNQ queries per launch; gather: over the accepted ordinals of every segment,
// compacted first (count, then prefix + write).
int32_t scan_valu(const Sq8Call& c, bool gather, Sq8Lists& out) {
    osk_view* v = c.v;
    int32_t rc = gather ? ensure_gather(v, c.st) : OSK_OK;
    if (rc) return rc;
    Sq8ScanParams p{};
    rc = sq8_lists(c, gather ? v->n_gtiles : v->n_tiles, 64 / sq8_lanes(v->units8), p, out);
    if (rc) return rc;
    if (gather) {
        FilterParams fp{};
        fp.segs = p.segs;
        fp.tiles = p.tiles;
        fp.accept = c.d_accept;
        fp.seg_vrow = p.seg_vrow;
        fp.seg_tiles = v->d_seg_tiles.as<int2>();
        fp.tcnt = v->ws_tcnt.as<int32_t>();
        fp.scnt = v->ws_scnt.as<int32_t>();
        fp.comp = v->ws_comp.as<uint32_t>();
        fp.n_tiles = v->n_tiles;
        fp.n_segs = (int)v->segs.size();
        OSK_HIP(launch_filter_compact(fp, c.st));
        p.gather = GatherSplit{v->d_gtiles.as<int4>(), fp.comp, fp.scnt, g_tuning.gather_min};
        out.gather = p.gather;
        out.slices = v->d_gslices.as<int4>();
        out.shard_slice_begin = v->d_gshard_slice_begin.as<int32_t>();
        out.n_slices = v->n_gslices;
    }
    for (int q0 = 0; q0 < c.nq; q0 += kMaxNQ) {
        sq8_chunk(v, p, q0, kMaxNQ, c.nq);
        OSK_HIP(launch_sq8_scan(p.q_count, p, c.st, launch_ev_start(v, q0), launch_ev_stop(v, q0, c.nq)));
    }
    return OSK_OK;
}

// sq8_mfma, sq8_mfma_queries (16 or 32) per launch.  Pilot: 16 sampled rows per wave → per (query, tile) the
// top k sampled lower bounds → per (query, shard) the top k; its k-th floors the main pass's quick
// thresholds (sq8_mfma comment).
int32_t scan_mfma(const Sq8Call& c, Sq8Lists& out) {
    osk_view* v = c.v;
    const int S = v->n_shards;
    Sq8MfmaParams p{};
    int32_t rc = sq8_lists(c, v->n_tiles, kMfmaScanR, p, out);
    if (rc || (rc = ensure_sq8t(v, c.st)) != OSK_OK) return rc;
    // pilot keys: per (query, tile) 64 sampled keys
    OSK_HIP(v->ws_pilot.reserve(sizeof(uint64_t) * kMfmaQueries * 64 * (size_t)std::max(1, v->n_tiles)));
    OSK_HIP(v->ws_thr.reserve(sizeof(uint64_t) * kMfmaQueries * S * 64));
    OSK_HIP(v->ws_thr_counts.reserve(sizeof(int32_t) * kMfmaQueries * S));
    p.rows8t = v->d_sq8_rows_t.as<const int4*>();
    p.nt = g_tuning.sq8_mfma_nt;
    p.pilot_keys = v->ws_pilot.as<uint64_t>();
    p.thr_keys = v->ws_thr.as<uint64_t>();
    p.thr_counts = v->ws_thr_counts.as<int32_t>();
    const int chunk = g_tuning.sq8_mfma_queries;
    for (int q0 = 0; q0 < c.nq; q0 += chunk) {
        sq8_chunk(v, p, q0, chunk, c.nq);
        p.ring_slots = sq8_ring_slots(p.units8, p.q_count > 16 ? 2 : 1, g_tuning.sq8_mfma_ring);
        p.pilot = 1;
        OSK_HIP(launch_sq8_mfma(p, c.st, launch_ev_start(v, q0), nullptr));
        OSK_HIP(launch_merge_shards(p.pilot_keys, v->n_tiles, v->d_shard_tile_begin.as<int32_t>(), S, p.q_count, c.k,
                                    v->ws_thr.as<uint64_t>(), v->ws_thr_counts.as<int32_t>(), c.st));
        p.pilot = 0;
        OSK_HIP(launch_sq8_mfma(p, c.st, nullptr, launch_ev_stop(v, q0, c.nq, chunk)));
    }
    return OSK_OK;
}

// The wide kernels, kWideQ queries per launch, over their own copy and tile table (ensure_sq8w).  Pilot: the
// first rows of every quarter → per (query, quarter) the best lower-bound key (and the quarter's list
// maximum zeroed) → per (query, shard) the k-th best of them floors the main passes (sq8_wide_first_pass).
int32_t scan_wide(const Sq8Call& c, Sq8Lists& out) {
    osk_view* v = c.v;
    const int S = v->n_shards;
    int32_t rc = ensure_sq8w(v, c.st);
    if (rc) return rc;
    Sq8WideParams p{};
    rc = sq8_lists(c, v->n_wtiles, kMfmaScanR, p, out);
    if (rc) return rc;
    out.tiles = v->d_wtiles.as<TileDev>();
    out.wide_shard_tile_begin = v->d_wshard_tile_begin.as<int32_t>();
    // pilot keys: per (query, quarter) of the kernels' own table (4 per wide tile, qi·4·n_wtiles + list)
    OSK_HIP(v->ws_pilot.reserve(sizeof(uint64_t) * kWideQ * 4 * (size_t)std::max(1, v->n_wtiles)));
    OSK_HIP(v->ws_wfloor.reserve(sizeof(uint32_t) * 2 * kWideQ * S));
    // persistent workgroups: one per CU (sq8_wide_grid overrides it: the tests' LDS-cap grid doubling)
    p.wide_grid = g_tuning.sq8_wide_grid > 0 ? (int)g_tuning.sq8_wide_grid : view_cus(v);
    p.rows8w = v->d_sq8_rows_w.as<const int4*>();
    p.auxt = v->d_sq8_auxt.as<const float4*>();
    p.wtiles = v->d_wtiles.as<TileDev>();
    p.tile_order = v->d_wtile_order.as<int32_t>();
    p.pilot_rows = sq8_wide_pilot_rows(v);
    p.wide_defer = g_tuning.sq8_wide_defer;
    p.pilot_keys = v->ws_pilot.as<uint64_t>();
    p.quarter_bm = v->d_quarter_bm.as<const float4>();
    p.wide_qtable = v->d_wqtable.p;
    p.wide_claim = g_tuning.sq8_wide_rows_claim;
    // ≤ 128 dims: the pilot and the main passes without a step barrier (sq8_wide_rows, osk_sq8w.hip)
    const bool rows = g_tuning.sq8_wide_rows && sq8_wide_rows_supported(p.units8);
    p.wide_qcap = rows ? (int)g_tuning.sq8_wide_rows_qcap : 0;
    auto launch = [&](hipEvent_t e0, hipEvent_t e1) {
        return rows ? launch_sq8_wide_rows(p, c.st, e0, e1) : launch_sq8_wide(p, c.st, e0, e1);
    };
    const int nql = p.n_lists;
    const int n_a = sq8_wide_first_pass(nql, p.wide_grid);
    const int32_t* sqb = v->d_shard_quarter_begin.as<int32_t>();
    uint32_t* floor_a = v->ws_wfloor.as<uint32_t>();
    uint32_t* floor_b = floor_a + (size_t)kWideQ * S;
    for (int q0 = 0; q0 < c.nq; q0 += kWideQ) {
        sq8_chunk(v, p, q0, kWideQ, c.nq);
        p.pilot = 1;
        p.quarter_begin = 0;
        p.quarter_end = 0;
        p.floors = nullptr;
        OSK_HIP(launch(launch_ev_start(v, q0), nullptr));
        OSK_HIP(launch_wide_floor(nullptr, p.pilot_keys, nql, sqb, S, p.q_count, c.k, nullptr, floor_a, c.st));
        p.pilot = 0;
        p.floors = floor_a;
        if (n_a > 0) {   // (the pilot zeroed every list maximum: the second pass's read as empty until it writes them)
            p.quarter_end = n_a;
            OSK_HIP(launch(nullptr, nullptr));
            OSK_HIP(launch_wide_floor(p.list_lbmax + (size_t)q0 * nql, nullptr, nql, sqb, S, p.q_count, c.k, floor_a,
                                      floor_b, c.st));
            p.quarter_begin = n_a;
            p.quarter_end = 0;
            p.floors = floor_b;
        }
        OSK_HIP(launch(nullptr, launch_ev_stop(v, q0, c.nq, kWideQ)));
    }
    return OSK_OK;
}

// The 6-bit tier, one query: pilot → streaming pass over the 6-bit codes → int8 re-bound of the rows that
// passed; sq6_prep reserved and the fused prep filled its query form.  A call whose view is in a share group
// with another view (plan.share) posts its query after the pilot and takes the group's shared pass, chained
// behind the group's previous one; every other call launches today's three kernels (launch_sq6_scan).
int32_t sq6_params(const Sq8Call& c, const Sq8Plan& plan, Sq6Params& p, Sq8Lists& out) {
    osk_view* v = c.v;
    int32_t rc = sq8_lists(c, v->n_tiles, kSq6ScanR, p, out);
    if (rc) return rc;
    OSK_HIP(v->ws_cand6.reserve(sizeof(uint2) * (size_t)p.n_lists * kSq6Cap));
    OSK_HIP(v->ws_cnt6.reserve(sizeof(int32_t) * (size_t)c.nq * p.n_lists));
    p.rows6 = v->d_sq6_rows.as<const void*>();
    p.aux6 = v->d_sq6_aux.as<const float4*>();
    p.q6 = v->ws_q6.as<int4>();
    p.qc6 = v->ws_qc6.as<float4>();
    p.floor = v->ws_floor.as<uint32_t>();
    p.tile_order = v->d_tile_order.as<int32_t>();
    p.rb_cus = view_cus(v);   // (the persistent re-bound's grid: 4 workgroups per CU)
    p.n_segs = (int)v->segs.size();
    p.rb_stride = g_tuning.sq6_rebound_stride;
    p.rb_retest = g_tuning.sq6_rebound_retest;
    p.rb_wg_per_cu = g_tuning.sq6_rebound_wgs;
    p.cand6 = v->ws_cand6.as<uint2>();
    p.cnt6 = v->ws_cnt6.as<int32_t>();
    p.cap6 = kSq6Cap;
    p.seg_rebound = plan.probe6 ? v->d_seg_rebound.as<unsigned long long>() : nullptr;
    sq8_chunk(v, p, 0, 1, c.nq);
    return OSK_OK;
}

// Steps 1 and 2 of a sharing call: the pilot, then the post of the view's slot with the group's next generation
int32_t sq6_share_post(const Sq8Call& c, Sq6Params& p) {
    osk_view* v = c.v;
    Sq6Group* grp = static_cast<Sq6Group*>(v->share_group);
    OSK_HIP(launch_sq6_pilot(p, v->dim, c.st));
    Sq6Slot d{};
    {
        std::lock_guard<std::mutex> lk(grp->mu);
        uint32_t& g = grp->gen[v->share_slot];
        g = g + 1u ? g + 1u : 1u;   // (never 0: an empty slot)
        d.gen = g;
        d.seq = ++grp->seq;
    }
    d.k = p.k;
    d.q6 = p.q6;
    d.qc6 = p.qc6;
    d.qn_dev = p.qn_dev;
    d.floor = p.floor;
    d.cand6 = p.cand6;
    d.cnt6 = p.cnt6;
    OSK_HIP(launch_sq6_post(grp->d_slots + v->share_slot, d, c.st));
    p.sh_slots = grp->d_slots;
    p.sh_done = grp->d_done;
    p.sh_slot = v->share_slot;
    p.sh_gen = d.gen;
    const int limit = g_tuning.sq6_share_limit;
    p.sh_limit = limit < 0 ? INT32_MAX : limit;
    p.sh_idle = g_tuning.sq6_share_idle;
    return OSK_OK;
}

// Steps 3 and 4: the shared pass behind the group's previous one, then this view's own re-bound
int32_t sq6_share_scan(const Sq8Call& c, const Sq6Params& p) {
    osk_view* v = c.v;
    Sq6Group* grp = static_cast<Sq6Group*>(v->share_group);
    {
        std::lock_guard<std::mutex> lk(grp->mu);
        hipError_t e = grp->has_last ? hipStreamWaitEvent(c.st, grp->last, 0) : hipSuccess;
        if (e == hipSuccess) e = launch_sq6_scan_shared(p, v->dim, c.st, launch_ev_start(v, 0), launch_ev_stop(v, 0, c.nq));
        if (e == hipSuccess) e = hipEventRecord(grp->last, c.st);
        if (e != hipSuccess) {
            // the query is posted but its pass is not coming: withdraw it, so no later pass writes this view's
            // lists while another call of the view uses them
            sq6_share_withdraw(grp, v->share_slot);
            OSK_HIP(e);
        }
        grp->has_last = true;
    }
    OSK_HIP(launch_sq6_rebound(p, v->dim, c.st));
    return OSK_OK;
}

int32_t scan_sq6(const Sq8Call& c, const Sq8Plan& plan, Sq8Lists& out) {
    osk_view* v = c.v;
    Sq6Params p{};
    int32_t rc = sq6_params(c, plan, p, out);
    if (rc) return rc;
    if (plan.share) {
        if ((rc = sq6_share_post(c, p)) != OSK_OK) return rc;
        return sq6_share_scan(c, p);
    }
    OSK_HIP(launch_sq6_scan(p, v->dim, c.st, launch_ev_start(v, 0), launch_ev_stop(v, 0, c.nq)));
    // a segment may still turn the tier off: its free waits for this launch
    return plan.probing ? sq6_track_launch(v, c.st) : OSK_OK;
}

// Settle the lists a scan reported: per slice of kSliceLists lists (sq8_settle → sq8_settle_merge), or per
// (shard, query) for the wide scans (sq8_settle_wide).
int32_t sq8_settle_lists(const Sq8Call& c, const Sq8Lists& lists) {
    osk_view* v = c.v;
    OSK_HIP(v->ws_part.reserve(sizeof(uint64_t) * (size_t)c.nq * lists.n_slices * c.k));
    SettleParams sp{};
    sp.slices = lists.slices;
    sp.shard_slice_begin = lists.shard_slice_begin;
    sp.tiles = lists.tiles;
    sp.gather = lists.gather;   // the scan's split, exactly
    sp.accept = c.d_accept;
    sp.part = v->ws_part.as<uint64_t>();
    sp.n_slices = lists.n_slices;
    sp.segs = v->d_segs.as<SegDev>();
    sp.seg_vrow = v->d_seg_vrow.as<int64_t>();
    sp.cand = v->ws_sq8cand.as<uint64_t>();
    sp.cand_lb = v->ws_sq8lb.as<uint32_t>();
    sp.list_lbmax = v->ws_lbmax.as<uint32_t>();
    sp.q = v->ws_q.p;
    sp.qnorm = v->ws_qnorm.as<float>();
    sp.shard_keys = c.d_shard_keys;
    sp.shard_counts = c.d_shard_counts;
    sp.flags = v->ws_flags.as<int>();
    sp.counters = v->d_counters.as<unsigned long long>();
    sp.n_lists = lists.n_lists;
    sp.scan_R = lists.scan_R;
    sp.n_shards = v->n_shards;
    sp.n_segs = (int)v->segs.size();
    sp.units = v->units;
    sp.k = c.k;
    sp.sim = v->sim;
    sp.force_fail = g_tuning.sq8_force_fallback;
    if (g_tuning.settle_trace) {
        OSK_HIP(v->ws_trace.reserve(sizeof(unsigned long long) * 8 * (size_t)c.nq * lists.n_slices));
        sp.trace = v->ws_trace.as<unsigned long long>();
    }
    sp.shard_tile_begin = lists.wide_shard_tile_begin;
    if (lists.wide_shard_tile_begin)
        OSK_HIP(launch_sq8_settle_wide(v->cfg, c.nq, sp, c.st));
    else
        OSK_HIP(launch_sq8_settle(v->cfg, c.nq, sp, c.st));
    return OSK_OK;
}

// What follows a scan: the settle of its lists, the call counts, a probe call's read-back.
int32_t sq8_finish(const Sq8Call& c, const Sq8Plan& plan, const Sq8Lists& lists) {
    osk_view* v = c.v;
    int32_t rc = profile_end(v, c.st, false);
    if (rc || (rc = sq8_settle_lists(c, lists)) != OSK_OK) return rc;
    v->sq8_calls += 1;
    v->sq8w_calls += plan.strategy == Sq8Strategy::kWide ? 1 : 0;
    v->sq6_calls += plan.strategy == Sq8Strategy::kSq6 ? 1 : 0;
    if (plan.probe6) {   // read back asynchronously: a later call folds it (fold_probe), nothing waits here
        OSK_HIP(hipMemcpyAsync(v->h_seg_rebound.p, v->d_seg_rebound.p, sizeof(unsigned long long) * v->segs.size(),
                               hipMemcpyDeviceToHost, c.st));
        OSK_HIP(hipEventRecord(v->ev_probe, c.st));
        v->probe_pending = true;
    }
    return OSK_OK;
}

#ifdef OSK_TESTING
// A sharing call stopped after its post (osk_testing_sq6_post), for osk_testing_sq6_resume
struct Sq6Held {
    Sq8Call c;
    Sq8Plan plan;
    Sq6Params p;
    Sq8Lists lists;
};
#endif

// ws_q / ws_qnorm are reserved by the caller; wide_pick: sq8_wide_pick for this call.
int32_t sq8_search(osk_view* v, const void* d_queries, int nq, int k, int UP, const uint64_t* const* d_accept,
                   uint64_t* d_shard_keys, int32_t* d_shard_counts, int64_t* d_visited, hipStream_t st,
                   bool wide_pick) {
    const Sq8Call c{v, nq, k, d_accept, d_shard_keys, d_shard_counts, d_visited, st};
    int32_t rc = ensure_sq8(v, st);
    if (rc || (rc = fold_probe(v, st)) != OSK_OK) return rc;
    std::shared_lock<std::shared_mutex> tier_lock(g_sq6_free_mu, std::defer_lock);
    Sq8Plan plan = sq8_decide(v, nq, d_accept != nullptr, wide_pick, tier_lock);
    // the 6-bit tier with every segment calibrated and kept (a kept segment never frees its copy): share the
    // pass when another view is in the view's group (tune sq6_share, read once per call)
    if (plan.strategy == Sq8Strategy::kSq6 && !plan.probing && g_tuning.sq6_share) {
        if (!v->share_tried && (rc = sq6_share_attach(v)) != OSK_OK) return rc;
        if (Sq6Group* grp = static_cast<Sq6Group*>(v->share_group)) {
            std::lock_guard<std::mutex> lk(grp->mu);
            // ...and the pass runs more than one round of resident workgroups: the tiles of a single round all
            // start together, before a neighbour's post can land, so nothing would be shared and the chained
            // passes would only lose the overlap of their tails (one shard of the headline: −7 %)
            const int min_tiles = g_tuning.sq6_share_min_tiles;
            const int rounds_over = view_cus(v) * std::max(1, (int)g_tuning.tile_slots_per_cu);
            plan.share = grp->attached > 1 && v->n_tiles > (min_tiles > 0 ? min_tiles - 1 : rounds_over);
        }
    }
    if ((rc = sq8_prep_queries(c, d_queries, UP, plan)) != OSK_OK) return rc;
    Sq8Lists lists{};
#ifdef OSK_TESTING
    if (v->share_stop == 1) {
        OSK_REQUIRE(plan.share, "the call does not share its 6-bit pass");
        auto held = std::make_shared<Sq6Held>(Sq6Held{c, plan, Sq6Params{}, Sq8Lists{}});
        if ((rc = sq6_params(c, plan, held->p, held->lists)) != OSK_OK || (rc = sq6_share_post(c, held->p)) != OSK_OK)
            return rc;
        v->share_held = held;
        return OSK_OK;
    }
#endif
    switch (plan.strategy) {
        case Sq8Strategy::kValu: rc = scan_valu(c, plan.gather, lists); break;
        case Sq8Strategy::kMfma: rc = scan_mfma(c, lists); break;
        case Sq8Strategy::kWide: rc = scan_wide(c, lists); break;
        case Sq8Strategy::kSq6: rc = scan_sq6(c, plan, lists); break;
    }
    return rc ? rc : sq8_finish(c, plan, lists);
}

// The select path's workspaces and the parameters every query of a call shares: the per-row records (bounds:
// LB / UB; exact: keys), the radix state and histograms, and a candidate region of a whole shard.  *rows =
// the view's rows (the records' length).
int32_t select_workspace(osk_view* v, int k, const uint64_t* const* d_accept, bool bounds, SelParams& p,
                         int64_t* rows) {
    const int S = v->n_shards;
    int64_t total = 0;
    std::vector<int64_t> shard_rows(S, 0);
    for (size_t i = 0; i < v->segs.size(); ++i) {
        total += v->segs[i]->n_rows;
        shard_rows[v->seg_shard[i]] += v->segs[i]->n_rows;
    }
    const int64_t cap = std::max<int64_t>(1, *std::max_element(shard_rows.begin(), shard_rows.end()));
    OSK_REQUIRE(cap < (1ll << 31), "a shard holds < 2^31 rows");
    if (bounds) {
        OSK_HIP(v->ws_sel_lb.reserve(sizeof(uint32_t) * std::max<int64_t>(1, total)));
        OSK_HIP(v->ws_sel_ub.reserve(sizeof(uint32_t) * std::max<int64_t>(1, total)));
    } else {
        OSK_HIP(v->ws_sel_keys.reserve(sizeof(uint64_t) * std::max<int64_t>(1, total)));
    }
    OSK_HIP(v->ws_sel_state.reserve(sizeof(RadixState) * S));
    OSK_HIP(v->ws_sel_hist.reserve(sizeof(uint32_t) * kSelBins * kSelRep * S));
    OSK_HIP(v->ws_sel_cand.reserve(sizeof(uint64_t) * (size_t)cap * S));
    if (cap > kSelCap) OSK_HIP(v->ws_sel_cand2.reserve(sizeof(uint64_t) * (size_t)cap * S));
    OSK_HIP(v->ws_sel_cnt.reserve(sizeof(int32_t) * std::max(1, v->n_tiles)));
    p.segs = v->d_segs.as<SegDev>();
    p.tiles = v->d_tiles.as<TileDev>();
    p.seg_vrow = v->d_seg_vrow.as<int64_t>();
    p.shard_tile_begin = v->d_shard_tile_begin.as<int32_t>();
    p.tile_coff = v->d_tile_coff.as<int32_t>();
    p.accept = d_accept;
    p.n_tiles = v->n_tiles;
    p.n_shards = S;
    p.n_segs = (int)v->segs.size();
    p.k = k;
    p.sim = v->sim;
    p.dim = v->dim;
    p.units = v->units;
    p.enc = v->enc;
    p.exact = bounds ? 0 : 1;
    p.lb = v->ws_sel_lb.as<uint32_t>();
    p.ub = v->ws_sel_ub.as<uint32_t>();
    p.keys = v->ws_sel_keys.as<uint64_t>();
    p.state = v->ws_sel_state.as<RadixState>();
    p.hist = v->ws_sel_hist.as<uint32_t>();
    p.cand = v->ws_sel_cand.as<uint64_t>();
    p.cand2 = v->ws_sel_cand2.as<uint64_t>();
    p.tile_count = v->ws_sel_cnt.as<int32_t>();
    p.cap = (int)cap;
    if (rows) *rows = total;
    return OSK_OK;
}

// The select path (osk_select.hip): exact top-k for any k ≤ OSK_MAX_K, one query at a time.
//   bounds = true: float32 fields through the int8 prefilter copy (bounds → threshold → candidates →
//   exact re-score → top k); bounds = false: exact mode (exact keys → threshold → top k; float32 with the
//   prefilter off, byte vectors).  The candidate buffer holds a whole shard, so nothing overflows and
//   nothing waits on the host.  ws_q / ws_qnorm hold the padded queries (exact mode: the caller's
//   launch_prep_queries; bounds mode: sq8_prep here).
int32_t select_search(osk_view* v, const void* d_queries, int nq, int k, int UP, const uint64_t* const* d_accept,
                      uint64_t* d_shard_keys, int32_t* d_shard_counts, int64_t* d_visited, hipStream_t st,
                      bool bounds) {
    const int S = v->n_shards;
    const int nq_pad = (nq + kMaxNQ - 1) / kMaxNQ * kMaxNQ;
    int u8 = 0;
    if (bounds) {
        int32_t rc = ensure_sq8(v, st);
        if (rc) return rc;
        u8 = v->units8;
        OSK_HIP(v->ws_q8.reserve((size_t)nq_pad * u8 * 16));
        OSK_HIP(v->ws_qc.reserve(sizeof(float4) * nq_pad));
        OSK_HIP(v->ws_flags.reserve(sizeof(int) * nq));
        OSK_HIP(launch_sq8_prep(v->cfg, static_cast<const float*>(d_queries), v->dim, nq, nq_pad, UP, u8,
                                v->ws_q.as<float4>(), v->ws_qnorm.as<float>(), v->ws_q8.p, v->ws_qc.as<float4>(),
                                v->ws_flags.as<int>(), st));
    } else {
        if (v->enc == ENC_FLOAT32 && v->sim == SIM_COSINE)
            OSK_HIP(launch_row_norms_f32(v->ws_q.as<float4>(), nq, UP, v->cfg, v->ws_qnorm.as<float>(), st));
    }
    SelParams p{};
    const int32_t rc_ws = select_workspace(v, k, d_accept, bounds, p, nullptr);
    if (rc_ws) return rc_ws;
    p.units8 = u8;
    p.writer = g_tuning.sel_writer.load(std::memory_order_relaxed);
    p.rows8 = v->d_sq8_rows.as<const int4*>();
    p.aux = v->d_sq8_aux.as<const float4*>();
    p.gam = v->sq8_gam;
    p.g2 = v->sq8_g2;
    for (int q = 0; q < nq; ++q) {
        p.q = v->ws_q.as<char>() + (size_t)q * UP * 16;
        p.qnorm = v->ws_qnorm.as<float>() + q;
        p.q8 = v->ws_q8.as<int4>() + (size_t)q * u8;
        p.qc = v->ws_qc.as<float4>() + q;
        p.qflags = bounds ? v->ws_flags.as<int>() + q : nullptr;
        p.out_keys = d_shard_keys + (size_t)q * S * k;
        p.out_counts = d_shard_counts + (size_t)q * S;
        p.visited = q == 0 ? reinterpret_cast<unsigned long long*>(d_visited) : nullptr;
        OSK_HIP(launch_select_one(p, v->cfg, st, launch_ev_start(v, q), launch_ev_stop(v, q, nq, 1)));
    }
    v->sel_calls += 1;
    return OSK_OK;
}

}  // namespace

namespace osk {

// Lease a workspace slot of `root` for one synchronous host call: a free slot if there is one, else a
// new replica (up to kMaxLeases slots), else wait for a slot to come free.
int32_t lease_view(osk_view* root, ViewLease& out) {
    std::unique_lock<std::mutex> lk(root->lease_mu);
    for (;;) {
        int slot = -1;
        for (size_t i = 0; i < root->lease_busy.size(); ++i)
            if (!root->lease_busy[i]) {
                slot = (int)i;
                break;
            }
        if (slot < 0 && (int)root->lease_busy.size() < osk_view::kMaxLeases) {
            hipStream_t st = nullptr;
            OSK_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            if (!root->lease_busy.empty()) {   // slots 1..: a replica over the same segments
                std::vector<osk_seg*> segs = root->segs;
                osk_view* v = nullptr;
                int32_t rc = osk_view_create(segs.data(), (int32_t)segs.size(), root->seg_shard.data(),
                                             root->seg_doc_base.data(), root->n_shards, root->shard_index.data(), &v);
                if (rc) {
                    (void)hipStreamDestroy(st);
                    return rc;
                }
                if (!root->holds_refs) {   // a segment's self view: its replicas must not keep it alive
                    v->holds_refs = false;
                    for (osk_seg* sg : segs) sg->refs.fetch_sub(1);
                }
                root->replicas.push_back(v);
            }
            root->lease_streams.push_back(st);
            root->lease_busy.push_back(0);
            slot = (int)root->lease_busy.size() - 1;
        }
        if (slot >= 0) {
            root->lease_busy[slot] = 1;
            out.root = root;
            out.slot = slot;
            out.v = slot == 0 ? root : root->replicas[slot - 1];
            out.st = root->lease_streams[slot];
            return OSK_OK;
        }
        root->lease_cv.wait(lk);
    }
}

ViewLease::~ViewLease() {
    if (!root) return;
    {
        std::lock_guard<std::mutex> lk(root->lease_mu);
        root->lease_busy[slot] = 0;
    }
    root->lease_cv.notify_one();
}

// Every search on a view reuses its workspace.  Calls are serialised by the view mutex on the host,
// but a call on stream B could still overtake a call on stream A on the device, so a search whose
// stream differs from the previous one first waits for everything enqueued on that stream so far
// (an event recorded there now).  Same-stream calls — the common case — pay nothing.  A caller stream
// must therefore stay valid until the next search on the view has been issued (osknn.h).
int32_t order_after_last(osk_view* v, hipStream_t st) {
    if (v->last_stream != nullptr && v->last_stream != st) {
        if (!v->xs_event) OSK_HIP(hipEventCreateWithFlags(&v->xs_event, hipEventDisableTiming));
        OSK_HIP(hipEventRecord(v->xs_event, v->last_stream));
        OSK_HIP(hipStreamWaitEvent(st, v->xs_event, 0));
    }
    v->last_stream = st;
    return OSK_OK;
}

int32_t upload_accept(osk_view* v, const uint64_t* const* accept, hipStream_t st, const uint64_t* const** d_accept) {
    *d_accept = nullptr;
    const int ns = (int)v->segs.size();
    size_t words = 0;
    bool any_bits = false;
    for (int i = 0; accept && i < ns; ++i)
        if (accept[i]) {
            any_bits = true;
            words += (size_t)(v->segs[i]->max_doc + 63) / 64;
        }
    if (!any_bits) return OSK_OK;
    OSK_HIP(v->ws_accept.reserve(std::max<size_t>(8, words * 8)));
    OSK_HIP(v->ws_accept_ptrs.reserve(sizeof(void*) * ns));
    // the pointer table is staged in the view's pinned buffer: it is the source of an async copy and
    // must outlive it (the stream is synchronised only at the end of the call)
    OSK_HIP(v->h_accept_tab.reserve(sizeof(void*) * ns));
    const uint64_t** ptrs = static_cast<const uint64_t**>(v->h_accept_tab.p);
    size_t off = 0;
    for (int i = 0; i < ns; ++i) {
        ptrs[i] = nullptr;
        if (!accept[i]) continue;
        const size_t w = (size_t)(v->segs[i]->max_doc + 63) / 64;
        ptrs[i] = v->ws_accept.as<uint64_t>() + off;
        if (w) OSK_HIP(hipMemcpyAsync(const_cast<uint64_t*>(ptrs[i]), accept[i], w * 8, hipMemcpyHostToDevice, st));
        off += w;
    }
    OSK_HIP(hipMemcpyAsync(v->ws_accept_ptrs.p, ptrs, sizeof(void*) * ns, hipMemcpyHostToDevice, st));
    *d_accept = v->ws_accept_ptrs.as<const uint64_t*>();
    return OSK_OK;
}

void MergedOut::copy_out(const char* stage, float* scores, int32_t* docs, int32_t* shard, int32_t* count,
                         int64_t* total, float* max) const {
    std::memcpy(scores, stage + o_sc, b_hits);
    std::memcpy(docs, stage + o_doc, b_hits);
    std::memcpy(shard, stage + o_sh, b_hits);
    std::memcpy(count, stage + o_cnt, b_cnt);
    std::memcpy(total, stage + o_tot, b_tot);
    std::memcpy(max, stage + o_max, b_max);
}

// Core of osk_view_search_device (caller holds the view mutex; device already set).
int32_t view_search_device(osk_view* v, const void* d_queries, int nq, int k,
                           const uint64_t* const* d_accept, uint64_t* d_shard_keys,
                           int32_t* d_shard_counts, int64_t* d_visited, hipStream_t st) {
    OSK_REQUIRE(nq >= 1, "n_queries must be >= 1");
    OSK_REQUIRE(k >= 1 && k <= OSK_MAX_K, "k must be in [1, OSK_MAX_K]");
    OSK_REQUIRE(d_queries && d_shard_keys && d_shard_counts, "null device buffer");
    int32_t rc0 = order_after_last(v, st);
    if (rc0) return rc0;
    const int UP = cfg_padded_units(v->cfg);
    const int nq_pad = (nq + kMaxNQ - 1) / kMaxNQ * kMaxNQ;

    if (v->n_tiles == 0) return zero_shard_hits(v, nq, k, d_shard_keys, d_shard_counts, d_visited, st);
    OSK_HIP(v->ws_q.reserve((size_t)nq_pad * UP * 16));
    OSK_HIP(v->ws_qnorm.reserve(sizeof(float) * nq_pad));
    // Path cost model, measured end to end on MI355X, in µs for this view's rows R:
    //   int8 prefilter: the cheaper of its kernels (sq8_narrow_us, sq8_wide_us);
    //   bf16×3, per block of ≤ 256 queries: R·(0.153 + 0.00119·dim) ns + ≈ 325 µs (C3 11.0, C4 27.1, C2 0.63 ms;
    //     fitted to those three, profiles/r02q/c2_batches_*.jsonl, c3_batches_*.jsonl).
    // 96-dim rows stay on the prefilter at any batch, 768-dim rows move to bf16×3 blocks from about 160
    // queries, and small views (C2) from about 128.  sq8_cost_pct scales the prefilter's side (100 = the model).
    // A view holding a row outside the certificate's range (osk_sq8.hip sq8_in_range; known once the int8
    // copy is built) is served by the exact paths, as if the prefilter were off.
    bool sq8_on = v->enc == ENC_FLOAT32 && g_tuning.sq8 && !(v->sq8_ready && !v->sq8_range_ok);
    double R = 0.0;
    for (const osk_seg* sg : v->segs) R += (double)sg->n_rows;
    const int u8v = (v->dim + 15) / 16;
    const bool wide_pick = sq8_wide_pick(v, nq, d_accept != nullptr);
    const double sq8_us = wide_pick ? sq8_wide_us(R, nq, u8v) : sq8_narrow_us(R, nq, u8v, v->dim);
    const double bf_us = (double)((nq + 255) / 256) * (R * (0.153 + 0.00119 * v->dim) * 1e-3 + 325.0);
    const bool blocks_cheaper = bf_us * 100.0 <= sq8_us * (double)g_tuning.sq8_cost_pct &&
                                !(g_tuning.sq8_wide_force && wide_pick);
    bool batched = false, prefilter = false, select = false;
    auto choose = [&]() {
        const bool sq8_ok = sq8_on && k <= kKQ - 4;
        batched = v->enc == ENC_FLOAT32 && g_tuning.mfma_min_batch > 0 && nq >= g_tuning.mfma_min_batch &&
                  k <= kKC - 4 && (!sq8_ok || blocks_cheaper);
        // k ≤ kKQ − 4: a tile list holds 4 more rows than k, so it rarely overflows past the certificate
        prefilter = !batched && sq8_ok;
        // the select path: k beyond the streaming scans' 64-lane lists, or float32 k beyond the prefilter's
        // lists (its int8 bounds pass reads ¼ of the fp32 scan's bytes)
        select = !batched && !prefilter && (k > kScanMaxK || (sq8_on && k > kKQ - 4 && g_tuning.select_mid_k));
    };
    choose();
    if (prefilter || (select && sq8_on)) {   // one-time build of the int8 copy
        const int32_t rc8 = ensure_sq8(v, st);
        if (rc8) return rc8;
        if (!v->sq8_range_ok) {
            sq8_on = false;
            choose();
        }
    }
    // queries → padded unit layout (zeros past dim and for the dummy queries of the last launch); the
    // prefilter path does this inside its own fused prep launch (so does the select path's bounds mode)
    if (!prefilter && !(select && sq8_on))
        OSK_HIP(launch_prep_queries(d_queries, v->dim * elem_bytes(v->enc), nq, v->ws_q.p, UP, nq_pad, st));

    if (d_visited) OSK_HIP(hipMemsetAsync(d_visited, 0, sizeof(int64_t) * v->segs.size(), st));

    int32_t rc = profile_sample(v, st, batched);
    if (rc) return rc;
    if (select) {
        rc = select_search(v, d_queries, nq, k, UP, d_accept, d_shard_keys, d_shard_counts, d_visited, st, sq8_on);
        if (rc == OSK_OK) rc = profile_end(v, st, false);
    } else if (prefilter) {
        rc = sq8_search(v, d_queries, nq, k, UP, d_accept, d_shard_keys, d_shard_counts, d_visited, st, wide_pick);
    } else if (batched) {
        // |q|² in the device lane layout: approx transforms, the re-score (COSINE) and the bound
        OSK_HIP(launch_row_norms_f32(v->ws_q.as<float4>(), nq, UP, v->cfg, v->ws_qnorm.as<float>(), st));
        rc = batched_search(v, nq, k, UP, d_accept, d_shard_keys, d_shard_counts, d_visited, st);
    } else {
        rc = stream_search(v, v->ws_q.p, v->ws_qnorm.p, nq, k, UP, d_accept, d_shard_keys, d_shard_counts,
                           d_visited, st);
    }
    if (rc) return rc;
    return OSK_OK;
}

// What the two threshold cores (every hit by position; the best k by score) share: the query prep, the mask /
// maybe / counts / offsets workspaces, the parameters of a pass and its first-pass launches.  The cores
// differ only in what follows thr_offsets.
namespace {
struct ThrCall {
    ThrParams p{};
    bool use8 = false;   // the certified int8 first pass (thr_scan_sq8 + thr_settle_f32)
    int UP = 0;
    size_t waves = 0;    // per query of a pass
};

// The prep of a call of nq queries; c.p is complete but for the outputs and the per-pass fields.
int32_t thr_begin(osk_view* v, const void* d_queries, int nq, const uint64_t* const* d_accept, int64_t* d_visited,
                  hipStream_t st, ThrCall& c) {
    int32_t rc = order_after_last(v, st);
    if (rc) return rc;
    const int UP = cfg_padded_units(v->cfg);
    const int nq_pad = (nq + kThrNQ - 1) / kThrNQ * kThrNQ;
    const int wpw = thr_words_per_wave(v->cfg, v->max_tile_rows);
    const size_t waves = (size_t)std::max(1, v->n_tiles) * 4;   // per query of a pass
    OSK_HIP(v->ws_q.reserve((size_t)nq_pad * UP * 16));
    OSK_HIP(v->ws_thr_mask.reserve(sizeof(uint64_t) * kThrNQ * waves * wpw));
    OSK_HIP(v->ws_thr_wcounts.reserve(sizeof(int32_t) * kThrNQ * waves));
    OSK_HIP(v->ws_thr_offsets.reserve(sizeof(int64_t) * kThrNQ * waves));
    // float32 views whose int8 copy certifies (no row outside the certificate's range) take the int8 first
    // pass: thr_scan_sq8 settles every row whose interval clears min_score on ¼ of the bytes, thr_settle_f32
    // re-scores the rest exactly.  Every other view, and every byte field, keeps the fp32 / byte scan.
    bool use8 = v->enc == ENC_FLOAT32 && v->n_tiles > 0 && g_tuning.thr_sq8.load(std::memory_order_relaxed) &&
                g_tuning.sq8 && !(v->sq8_ready && !v->sq8_range_ok);
    if (use8) {
        if ((rc = ensure_sq8(v, st)) != OSK_OK) return rc;
        use8 = v->sq8_range_ok;
    }
    if (use8) {   // the select path's fused prep: padded fp32 queries, |q|², int8 codes, bound terms, flags
        const int u8 = v->units8;
        OSK_HIP(v->ws_thr_maybe.reserve(sizeof(uint64_t) * kThrNQ * waves * wpw));
        OSK_HIP(v->ws_qnorm.reserve(sizeof(float) * nq_pad));
        OSK_HIP(v->ws_q8.reserve((size_t)nq_pad * u8 * 16));
        OSK_HIP(v->ws_qc.reserve(sizeof(float4) * nq_pad));
        OSK_HIP(v->ws_flags.reserve(sizeof(int) * nq_pad));
        OSK_HIP(launch_sq8_prep(v->cfg, static_cast<const float*>(d_queries), v->dim, nq, nq_pad, UP, u8,
                                v->ws_q.as<float4>(), v->ws_qnorm.as<float>(), v->ws_q8.p, v->ws_qc.as<float4>(),
                                v->ws_flags.as<int>(), st));
    } else {
        OSK_HIP(launch_prep_queries(d_queries, v->dim * elem_bytes(v->enc), nq, v->ws_q.p, UP, nq_pad, st));
    }
    if (d_visited) OSK_HIP(hipMemsetAsync(d_visited, 0, sizeof(int64_t) * v->segs.size(), st));
    if ((rc = profile_sample(v, st, false)) != OSK_OK) return rc;

    c.use8 = use8;
    c.UP = UP;
    c.waves = waves;
    ThrParams& p = c.p;
    if (use8) {
        p.maybe = v->ws_thr_maybe.as<uint64_t>();
        p.rows8 = v->d_sq8_rows.as<const int4*>();
        p.aux = v->d_sq8_aux.as<const float4*>();
        p.settled = v->d_counters.as<unsigned long long>() + kCtrThrSettledRows;
        p.gam = v->sq8_gam;
        p.g2 = v->sq8_g2;
        p.units8 = v->units8;
        p.wave_R = 64 / kCfgLV[v->cfg][0];
        p.all_maybe = g_tuning.thr_sq8_all_maybe.load(std::memory_order_relaxed);
    }
    p.segs = v->d_segs.as<SegDev>();
    p.tiles = v->d_tiles.as<TileDev>();
    p.accept = d_accept;
    p.mask = v->ws_thr_mask.as<uint64_t>();
    p.counts = v->ws_thr_wcounts.as<int32_t>();
    p.offsets = v->ws_thr_offsets.as<int64_t>();
    p.visited = reinterpret_cast<unsigned long long*>(d_visited);
    p.shard_tile_begin = v->d_shard_tile_begin.as<int32_t>();
    p.n_tiles = v->n_tiles;
    p.n_shards = v->n_shards;
    p.wpw = wpw;
    p.units = v->units;
    p.sim = v->sim;
    p.dim = v->dim;
    return OSK_OK;
}

// The pass of the call's queries [q0, q0 + kThrNQ): its fields of c.p, and (with tiles) the cleared mask and the
// corpus read that fills it and the counts.  What follows — thr_offsets and the emit or the collector — is the
// caller's.
int32_t thr_first_pass(osk_view* v, ThrCall& c, int q0, int nq, const float* d_min_scores, hipStream_t st) {
    ThrParams& p = c.p;
    p.q0 = q0;
    p.q_count = std::min(kThrNQ, nq - q0);
    p.q = v->ws_q.as<char>() + (size_t)q0 * c.UP * 16;
    p.min_score = d_min_scores + q0;
    if (v->n_tiles <= 0) return OSK_OK;   // (nothing staged: thr_offsets alone writes zero hits for every shard)
    OSK_HIP(hipMemsetAsync(p.mask, 0, sizeof(uint64_t) * p.q_count * c.waves * p.wpw, st));
    hipEvent_t ev_stop = v->profile && q0 + kThrNQ >= nq ? v->ev1 : nullptr;
    if (c.use8) {
        OSK_HIP(hipMemsetAsync(p.maybe, 0, sizeof(uint64_t) * p.q_count * c.waves * p.wpw, st));
        p.q8 = v->ws_q8.as<int4>() + (size_t)q0 * v->units8;
        p.qc = v->ws_qc.as<float4>() + q0;
        p.qnorm = v->ws_qnorm.as<float>() + q0;
        p.qflags = v->ws_flags.as<int>() + q0;
        OSK_HIP(launch_thr_scan_sq8(v->cfg, p, st, launch_ev_start(v, q0), ev_stop));
        OSK_HIP(launch_thr_settle(v->cfg, p, st));
    } else {
        OSK_HIP(launch_thr_scan(v->enc, v->cfg, p, st, launch_ev_start(v, q0), ev_stop));
    }
    return OSK_OK;
}
}  // namespace

// Core of osk_view_search_threshold_device (caller holds the view mutex; device already set): passes of up
// to kThrNQ queries, each one corpus read (thr_scan), a prefix sum (thr_offsets) and an in-order emit.
int32_t view_threshold_device(osk_view* v, const void* d_queries, int nq, const float* d_min_scores,
                              const uint64_t* const* d_accept, int cap, int32_t* d_docs, float* d_scores,
                              int32_t* d_count, int64_t* d_total, int64_t* d_visited, hipStream_t st) {
    OSK_REQUIRE(nq >= 1, "n_queries must be >= 1");
    OSK_REQUIRE(cap >= 1, "cap must be >= 1");
    OSK_REQUIRE(d_queries && d_min_scores && d_docs && d_scores && d_count && d_total, "null device buffer");
    ThrCall c;
    int32_t rc = thr_begin(v, d_queries, nq, d_accept, d_visited, st, c);
    if (rc) return rc;
    ThrParams& p = c.p;
    p.out_docs = d_docs;
    p.out_scores = d_scores;
    p.out_count = d_count;
    p.out_total = d_total;
    p.cap = cap;
    for (int q0 = 0; q0 < nq; q0 += kThrNQ) {
        if ((rc = thr_first_pass(v, c, q0, nq, d_min_scores, st)) != OSK_OK) return rc;
        OSK_HIP(launch_thr_offsets(p, st));
        if (v->n_tiles > 0) OSK_HIP(launch_thr_emit(v->enc, v->cfg, p, st));
    }
    if (v->n_tiles > 0 && (rc = profile_end(v, st, false)) != OSK_OK) return rc;
    v->thr_calls += 1;
    v->thr_sq8_calls += c.use8 ? 1 : 0;
    return OSK_OK;
}

// Core of osk_view_search_threshold_top_device (caller holds the view mutex; device already set): the same
// passes up to thr_offsets, which here writes the exact totals alone; then the pass's masked rows are
// re-scored into keys instead of positions.  k ≤ kScanMaxK: thr_top_* leaves a best-first list per (query,
// tile) and one merge_shards after the last pass makes the shard lists.  Larger k: per query, thr_keys_*
// stores the hit keys by view row into the select path's zeroed records and launch_select_one (keys_written)
// selects, collects and sorts them.  At most k candidates reach sel_sort — the shard's non-zero keys when
// they are ≤ k, else exactly the k largest (keys are distinct) — so they fit its LDS (k ≤ OSK_MAX_K < kSelCap),
// cand2 is never read, and cand stays sized for a whole shard as the k-NN select path leaves it.
int32_t view_threshold_top_device(osk_view* v, const void* d_queries, int nq, const float* d_min_scores, int k,
                                  const uint64_t* const* d_accept, uint64_t* d_shard_keys,
                                  int32_t* d_shard_counts, int64_t* d_shard_totals, int64_t* d_visited,
                                  hipStream_t st) {
    OSK_REQUIRE(nq >= 1, "n_queries must be >= 1");
    OSK_REQUIRE(k >= 1 && k <= OSK_MAX_K, "k must be in [1, OSK_MAX_K]");
    OSK_REQUIRE(d_queries && d_min_scores && d_shard_keys && d_shard_counts && d_shard_totals,
                "null device buffer");
    static_assert(OSK_MAX_K <= kSelCap, "the collector's candidates are sorted in LDS");
    ThrCall c;
    int32_t rc = thr_begin(v, d_queries, nq, d_accept, d_visited, st, c);
    if (rc) return rc;
    const bool select = k > kScanMaxK;
    ThrParams& p = c.p;
    p.out_total = d_shard_totals;
    p.top_k = k;
    SelParams sp{};
    int64_t rows = 0;
    if (v->n_tiles > 0 && select) {
        if ((rc = select_workspace(v, k, nullptr, false, sp, &rows)) != OSK_OK) return rc;
        sp.keys_written = 1;
        p.top_keys = sp.keys;
        p.seg_vrow = sp.seg_vrow;
    } else if (v->n_tiles > 0) {
        OSK_HIP(v->ws_cand.reserve(sizeof(uint64_t) * (size_t)nq * v->n_tiles * k));
        p.top_cand = v->ws_cand.as<uint64_t>();
    }
    for (int q0 = 0; q0 < nq; q0 += kThrNQ) {
        if ((rc = thr_first_pass(v, c, q0, nq, d_min_scores, st)) != OSK_OK) return rc;
        OSK_HIP(launch_thr_offsets(p, st));
        if (v->n_tiles <= 0) continue;
        if (!select) {
            OSK_HIP(launch_thr_top(v->enc, v->cfg, p, st));
            continue;
        }
        for (int b = 0; b < p.q_count; ++b) {
            OSK_HIP(hipMemsetAsync(sp.keys, 0, sizeof(uint64_t) * (size_t)rows, st));
            p.key_b = b;
            OSK_HIP(launch_thr_keys(v->enc, v->cfg, p, st));
            sp.out_keys = d_shard_keys + (size_t)(q0 + b) * v->n_shards * k;
            sp.out_counts = d_shard_counts + (size_t)(q0 + b) * v->n_shards;
            OSK_HIP(launch_select_one(sp, v->cfg, st));
        }
    }
    if (v->n_tiles <= 0) {
        if ((rc = zero_shard_hits(v, nq, k, d_shard_keys, d_shard_counts, d_visited, st)) != OSK_OK) return rc;
    } else {
        if (!select)
            OSK_HIP(launch_merge_shards(p.top_cand, v->n_tiles, p.shard_tile_begin, v->n_shards, nq, k, d_shard_keys,
                                        d_shard_counts, st));
        if ((rc = profile_end(v, st, false)) != OSK_OK) return rc;
    }
    v->thr_top_calls += 1;
    v->thr_top_sel_calls += select ? 1 : 0;
    v->thr_sq8_calls += c.use8 ? 1 : 0;
    return OSK_OK;
}

// Core of osk_view_search_nested_device (caller holds the view mutex; device already set): passes of up to
// kMaxNQ queries, each a clear of the pass's best-child keys, one corpus read (nest_scan) and the parent
// tiles' top k (nest_topk); then merge_shards over the parent tiles, as over scan tiles.  On the int8 route a
// pass is up to kNestSq8NQ queries and its corpus read is nest_scan_sq8, followed by the floor (nest_topk +
// merge_shards over the lower-bound keys) and the exact settle into the same best-child keys.
int32_t view_nested_device(osk_view* v, const void* d_queries, int nq, int k, const uint64_t* const* d_accept,
                           uint64_t* d_shard_keys, int32_t* d_shard_counts, int64_t* d_visited, hipStream_t st) {
    OSK_REQUIRE(nq >= 1, "n_queries must be >= 1");
    OSK_REQUIRE(k >= 1, "k must be >= 1");
    OSK_REQUIRE(d_queries && d_shard_keys && d_shard_counts, "null device buffer");
    if (k > kScanMaxK) {
        set_error("nested search supports k <= 64 (the streaming scan's lists); larger k is not implemented");
        return OSK_ERR_UNSUPPORTED;
    }
    int32_t rc = order_after_last(v, st);
    if (rc) return rc;
    if ((rc = ensure_nested(v, st)) != OSK_OK) return rc;
    if (v->n_tiles == 0) {
        v->nest_calls += 1;
        return zero_shard_hits(v, nq, k, d_shard_keys, d_shard_counts, d_visited, st);
    }
    const int UP = cfg_padded_units(v->cfg);
    const int nq_pad = (nq + kMaxNQ - 1) / kMaxNQ * kMaxNQ;   // (a multiple of kNestSq8NQ too)
    const size_t P = (size_t)v->nest_parents;
    // float32 views whose int8 copy certifies take the int8 first pass (view_threshold_device's rule): the
    // corpus is read once from the int8 copy, the rows that can still be the best child of a top-k family are
    // re-scored exactly.  Every other view, and every byte field, keeps the fp32 / byte scan.
    bool use8 = v->enc == ENC_FLOAT32 && v->n_tiles > 0 && g_tuning.nest_sq8.load(std::memory_order_relaxed) &&
                g_tuning.sq8 && !(v->sq8_ready && !v->sq8_range_ok);
    if (use8) {
        if ((rc = ensure_sq8(v, st)) != OSK_OK) return rc;
        use8 = v->sq8_range_ok;
    }
    const int pass = use8 ? kNestSq8NQ : kMaxNQ;
    int64_t n_rows = 0;
    for (const osk_seg* sg : v->segs) n_rows += sg->n_rows;
    OSK_HIP(v->ws_q.reserve((size_t)nq_pad * UP * 16));
    OSK_HIP(v->ws_nest_best.reserve(sizeof(uint64_t) * (size_t)std::min(nq, kMaxNQ) * P));
    OSK_HIP(v->ws_nest_cand.reserve(sizeof(uint64_t) * (size_t)nq * v->n_ptiles * k));
    if (use8) {   // the select path's fused prep: padded fp32 queries, |q|², int8 codes, bound terms, flags
        const int u8 = v->units8;
        OSK_HIP(v->ws_nest_ub.reserve(sizeof(uint32_t) * kNestSq8NQ * (size_t)n_rows));
        OSK_HIP(v->ws_nest_lbkey.reserve(sizeof(uint64_t) * kNestSq8NQ * P));
        OSK_HIP(v->ws_nest_fcand.reserve(sizeof(uint64_t) * kNestSq8NQ * (size_t)v->n_ptiles * k));
        OSK_HIP(v->ws_nest_fkeys.reserve(sizeof(uint64_t) * kNestSq8NQ * (size_t)v->n_shards * k));
        OSK_HIP(v->ws_nest_fcounts.reserve(sizeof(int32_t) * kNestSq8NQ * (size_t)v->n_shards));
        OSK_HIP(v->ws_qnorm.reserve(sizeof(float) * nq_pad));
        OSK_HIP(v->ws_q8.reserve((size_t)nq_pad * u8 * 16));
        OSK_HIP(v->ws_qc.reserve(sizeof(float4) * nq_pad));
        OSK_HIP(v->ws_flags.reserve(sizeof(int) * nq_pad));
        OSK_HIP(launch_sq8_prep(v->cfg, static_cast<const float*>(d_queries), v->dim, nq, nq_pad, UP, u8,
                                v->ws_q.as<float4>(), v->ws_qnorm.as<float>(), v->ws_q8.p, v->ws_qc.as<float4>(),
                                v->ws_flags.as<int>(), st));
    } else {
        OSK_HIP(launch_prep_queries(d_queries, v->dim * elem_bytes(v->enc), nq, v->ws_q.p, UP, nq_pad, st));
    }
    if (d_visited) OSK_HIP(hipMemsetAsync(d_visited, 0, sizeof(int64_t) * v->segs.size(), st));
    if ((rc = profile_sample(v, st, false)) != OSK_OK) return rc;

    NestParams p{};
    if (use8) {
        p.ub = v->ws_nest_ub.as<uint32_t>();
        p.lbkey = v->ws_nest_lbkey.as<unsigned long long>();
        p.floor_keys = v->ws_nest_fkeys.as<uint64_t>();
        p.floor_counts = v->ws_nest_fcounts.as<int32_t>();
        p.seg_vrow = v->d_seg_vrow.as<int64_t>();
        p.rows8 = v->d_sq8_rows.as<const int4*>();
        p.aux = v->d_sq8_aux.as<const float4*>();
        p.settled = v->d_counters.as<unsigned long long>() + kCtrNestSettledRows;
        p.n_rows = n_rows;
        p.gam = v->sq8_gam;
        p.g2 = v->sq8_g2;
        p.units8 = v->units8;
        p.n_shards = v->n_shards;
        p.all_settle = g_tuning.nest_sq8_all_settle.load(std::memory_order_relaxed);
    }
    p.segs = v->d_segs.as<SegDev>();
    p.tiles = v->d_tiles.as<TileDev>();
    p.nsegs = v->d_nest_segs.as<NestSeg>();
    p.accept = d_accept;
    p.best = v->ws_nest_best.as<unsigned long long>();
    p.visited = reinterpret_cast<unsigned long long*>(d_visited);
    p.ptiles = v->d_ptiles.as<NestPtile>();
    p.cand = v->ws_nest_cand.as<uint64_t>();
    p.n_parents = v->nest_parents;
    p.n_tiles = v->n_tiles;
    p.n_ptiles = v->n_ptiles;
    p.units = v->units;
    p.k = k;
    p.sim = v->sim;
    p.dim = v->dim;
    for (int q0 = 0; q0 < nq; q0 += pass) {
        p.q0 = q0;
        p.q_count = std::min(pass, nq - q0);
        p.q = v->ws_q.as<char>() + (size_t)q0 * UP * 16;
        OSK_HIP(hipMemsetAsync(p.best, 0, sizeof(uint64_t) * (size_t)p.q_count * P, st));
        if (use8) {
            OSK_HIP(hipMemsetAsync(p.lbkey, 0, sizeof(uint64_t) * (size_t)p.q_count * P, st));
            // a filtered scan stores the records of the steps that hold an accepted row only: a row that is not
            // accepted must have none
            if (d_accept) OSK_HIP(hipMemsetAsync(p.ub, 0, sizeof(uint32_t) * (size_t)p.q_count * (size_t)n_rows, st));
            p.q8 = v->ws_q8.as<int4>() + (size_t)q0 * v->units8;
            p.qc = v->ws_qc.as<float4>() + q0;
            p.qnorm = v->ws_qnorm.as<float>() + q0;
            p.qflags = v->ws_flags.as<int>() + q0;
            OSK_HIP(launch_nest_scan_sq8(v->cfg, p, st, launch_ev_start(v, q0), launch_ev_stop(v, q0, nq, pass)));
            // the floor: the k best LBp keys of each shard, by the kernels that rank the best-child keys
            NestParams f = p;
            f.best = p.lbkey;
            f.cand = v->ws_nest_fcand.as<uint64_t>();
            f.q0 = 0;
            OSK_HIP(launch_nest_topk(f, st));
            OSK_HIP(launch_merge_shards(f.cand, v->n_ptiles, v->d_shard_ptile_begin.as<int32_t>(), v->n_shards,
                                        p.q_count, k, v->ws_nest_fkeys.as<uint64_t>(),
                                        v->ws_nest_fcounts.as<int32_t>(), st));
            OSK_HIP(launch_nest_settle(v->cfg, p, st));
        } else {
            OSK_HIP(launch_nest_scan(v->enc, v->cfg, p, st, launch_ev_start(v, q0), launch_ev_stop(v, q0, nq)));
        }
        OSK_HIP(launch_nest_topk(p, st));
    }
    if ((rc = profile_end(v, st, false)) != OSK_OK) return rc;
    OSK_HIP(launch_merge_shards(v->ws_nest_cand.as<uint64_t>(), v->n_ptiles, v->d_shard_ptile_begin.as<int32_t>(),
                                v->n_shards, nq, k, d_shard_keys, d_shard_counts, st));
    v->nest_calls += 1;
    v->nest_sq8_calls += use8 ? 1 : 0;
    return OSK_OK;
}

}  // namespace osk

namespace {

// The single-segment view behind the segment entries, created on first use.  seg->mu guards only the
// creation: it is never held across a search.
int32_t seg_self_view(osk_seg* seg, osk_view** out) {
    std::lock_guard<std::mutex> lk(seg->mu);
    if (!seg->self_view) {
        osk_seg* one[1] = {seg};
        int32_t rc = osk_view_create(one, 1, nullptr, nullptr, 1, nullptr, &seg->self_view);
        if (rc) return rc;
        // owned by the segment: it must not keep the segment alive
        seg->self_view->holds_refs = false;
        seg->refs.fetch_sub(1);
    }
    *out = seg->self_view;
    return OSK_OK;
}

// One synchronous host call on a view: a leased workspace slot (the view or a replica) and its stream, the
// slot's mutex, the workspace ordered after the slot's previous call, the call timer.  Members are
// destroyed in reverse order: the slot's mutex is released before the lease.
struct HostCall {
    ViewLease lease;
    std::unique_lock<std::mutex> lock;
    CallTimer timer;
    osk_view* v = nullptr;
    hipStream_t st = nullptr;
    int32_t begin(osk_view* root) {
        int32_t rc = lease_view(root, lease);
        if (rc) return rc;
        v = lease.v;
        st = lease.st;
        lock = std::unique_lock<std::mutex>(v->mu);
        if ((rc = order_after_last(v, st)) != OSK_OK) return rc;
        return timer.begin(v, st);
    }
    int32_t finish() {   // after the call's last enqueue: the results are in the pinned stage on return
        int32_t rc = timer.end();
        if (rc) return rc;
        OSK_HIP(hipStreamSynchronize(st));
        return timer.publish();
    }
};

// The device core behind a host k-NN entry: view_search_device or view_nested_device.
using ShardTopK = int32_t (*)(osk_view*, const void*, int, int, const uint64_t* const*, uint64_t*, int32_t*, int64_t*,
                              hipStream_t);

}  // namespace

extern "C" {

int32_t osk_view_search_device(osk_view* view, const void* d_queries, int32_t n_queries, int32_t k,
                               const uint64_t* const* d_accept, uint64_t* d_shard_keys,
                               int32_t* d_shard_counts, int64_t* d_visited, void* stream) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(view != nullptr, "view is null");
    int32_t rc = check_device(view->device);
    if (rc) return rc;
    hipStream_t st = stream_or_default(stream, view->device);
    std::lock_guard<std::mutex> lk(view->mu);
    return view_search_device(view, d_queries, n_queries, k, d_accept, d_shard_keys, d_shard_counts,
                              d_visited, st);
    OSK_GUARD_END
}

#ifdef OSK_TESTING
// Testing build only: a sharing single-query call split at its shared pass.  osk_testing_sq6_post runs the
// prep, the pilot and the post of the view's slot on `stream` and stops; osk_testing_sq6_resume takes up the
// held call from the wait for the group's previous pass (the pass, the re-bound, the settle) on that stream.
int32_t osk_testing_sq6_post(osk_view* view, const void* d_queries, int32_t k, uint64_t* d_shard_keys,
                             int32_t* d_shard_counts, int64_t* d_visited, void* stream) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(view != nullptr, "view is null");
    int32_t rc = check_device(view->device);
    if (rc) return rc;
    hipStream_t st = stream_or_default(stream, view->device);
    std::lock_guard<std::mutex> lk(view->mu);
    OSK_REQUIRE(!view->share_held, "a posted call of this view has not been resumed");
    view->share_stop = 1;
    rc = view_search_device(view, d_queries, 1, k, nullptr, d_shard_keys, d_shard_counts, d_visited, st);
    view->share_stop = 0;
    if (rc == OSK_OK && !view->share_held) {
        set_error("the call did not take the 6-bit tier's shared pass");
        return OSK_ERR_INVALID;
    }
    return rc;
    OSK_GUARD_END
}

// ...and the share groups' key on the host alone: two views, each given as {device, n_shards, dim, sim}, its
// segment handles in order, its tiles as {seg, shard, row_begin, row_end} rows and their dispatch order.
int32_t osk_testing_sq6_share_key_equal(const int32_t* hdr_a, const uint64_t* segs_a, int32_t n_segs_a,
                                        const int64_t* tiles_a, const int32_t* order_a, int32_t n_tiles_a,
                                        const int32_t* hdr_b, const uint64_t* segs_b, int32_t n_segs_b,
                                        const int64_t* tiles_b, const int32_t* order_b, int32_t n_tiles_b,
                                        int32_t* out_equal) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(hdr_a && hdr_b && segs_a && segs_b && tiles_a && tiles_b && order_a && order_b && out_equal,
                "null argument");
    OSK_REQUIRE(n_segs_a >= 0 && n_segs_b >= 0 && n_tiles_a >= 0 && n_tiles_b >= 0, "negative count");
    auto key = [](const int32_t* h, const uint64_t* sg, int ns, const int64_t* t, const int32_t* ord, int nt) {
        Sq6ShareKey k{h[0], h[1], h[2], h[3], {}, {}, std::vector<int32_t>(ord, ord + nt)};
        for (int i = 0; i < ns; ++i) k.segs.push_back(reinterpret_cast<const osk_seg*>((uintptr_t)sg[i]));
        for (int i = 0; i < nt; ++i)
            k.tiles.push_back(TileDev{(int32_t)t[4 * i], (int32_t)t[4 * i + 1], t[4 * i + 2], t[4 * i + 3]});
        return k;
    };
    *out_equal = key(hdr_a, segs_a, n_segs_a, tiles_a, order_a, n_tiles_a) ==
                         key(hdr_b, segs_b, n_segs_b, tiles_b, order_b, n_tiles_b)
                     ? 1
                     : 0;
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_testing_sq6_resume(osk_view* view) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(view != nullptr, "view is null");
    int32_t rc = check_device(view->device);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(view->mu);
    OSK_REQUIRE(view->share_held != nullptr, "no posted call to resume");
    const std::shared_ptr<Sq6Held> held = std::static_pointer_cast<Sq6Held>(view->share_held);
    view->share_held.reset();
    rc = sq6_share_scan(held->c, held->p);
    return rc ? rc : sq8_finish(held->c, held->plan, held->lists);
    OSK_GUARD_END
}
#endif

// Packed-bit fields (osknn.h OSK_HAMMING) are served by the k-NN entries only: every threshold and nested entry
// refuses them here, before the device is touched (radial and nested Hamming search are not built).
static int32_t refuse_hamming(int sim, const char* what) {
    if (sim != SIM_HAMMING) return OSK_OK;
    set_error(std::string(what) + " is not served for Hamming (OSK_HAMMING) fields");
    return OSK_ERR_UNSUPPORTED;
}

int32_t osk_view_search_threshold_device(osk_view* view, const void* d_queries, int32_t n_queries,
                                         const float* d_min_scores, const uint64_t* const* d_accept, int32_t cap,
                                         int32_t* d_docs, float* d_scores, int32_t* d_count, int64_t* d_total,
                                         int64_t* d_visited, void* stream) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(view != nullptr, "view is null");
    OSK_REQUIRE(d_queries && d_min_scores && d_docs && d_scores && d_count && d_total, "null device buffer");
    OSK_REQUIRE(n_queries >= 1, "n_queries must be >= 1");
    OSK_REQUIRE(cap >= 1, "cap must be >= 1");
    int32_t rc = refuse_hamming(view->sim, "similarity-threshold search");
    if (rc) return rc;
    rc = any_device();
    if (rc) return rc;
    rc = check_device(view->device);
    if (rc) return rc;
    hipStream_t st = stream_or_default(stream, view->device);
    std::lock_guard<std::mutex> lk(view->mu);
    return view_threshold_device(view, d_queries, n_queries, d_min_scores, d_accept, cap, d_docs, d_scores, d_count,
                                 d_total, d_visited, st);
    OSK_GUARD_END
}

// The argument rules every threshold top-k entry checks before the device is touched.
static int32_t threshold_top_args(int32_t n_queries, int32_t k) {
    OSK_REQUIRE(n_queries >= 1, "n_queries must be >= 1");
    OSK_REQUIRE(k >= 1 && k <= OSK_MAX_K, "k must be in [1, OSK_MAX_K]");
    return OSK_OK;
}

int32_t osk_view_search_threshold_top_device(osk_view* view, const void* d_queries, int32_t n_queries,
                                             const float* d_min_scores, int32_t k, const uint64_t* const* d_accept,
                                             uint64_t* d_shard_keys, int32_t* d_shard_counts,
                                             int64_t* d_shard_totals, int64_t* d_visited, void* stream) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(view != nullptr, "view is null");
    OSK_REQUIRE(d_queries && d_min_scores && d_shard_keys && d_shard_counts && d_shard_totals,
                "null device buffer");
    int32_t rc = threshold_top_args(n_queries, k);
    if (rc) return rc;
    if ((rc = refuse_hamming(view->sim, "similarity-threshold search")) != OSK_OK) return rc;
    rc = any_device();
    if (rc) return rc;
    rc = check_device(view->device);
    if (rc) return rc;
    hipStream_t st = stream_or_default(stream, view->device);
    std::lock_guard<std::mutex> lk(view->mu);
    return view_threshold_top_device(view, d_queries, n_queries, d_min_scores, k, d_accept, d_shard_keys,
                                     d_shard_counts, d_shard_totals, d_visited, st);
    OSK_GUARD_END
}

// The argument rules every nested entry checks before the device is touched (k ≤ kScanMaxK: the lists of
// the streaming scan; larger k through the select path is not implemented).
static int32_t nested_args(int32_t n_queries, int32_t k) {
    OSK_REQUIRE(n_queries >= 1, "n_queries must be >= 1");
    OSK_REQUIRE(k >= 1, "k must be >= 1");
    if (k > kScanMaxK) {
        set_error("nested search supports k <= 64 (the streaming scan's lists); larger k is not implemented");
        return OSK_ERR_UNSUPPORTED;
    }
    return OSK_OK;
}

int32_t osk_view_search_nested_device(osk_view* view, const void* d_queries, int32_t n_queries, int32_t k,
                                      const uint64_t* const* d_accept, uint64_t* d_shard_keys,
                                      int32_t* d_shard_counts, int64_t* d_visited, void* stream) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(view != nullptr, "view is null");
    OSK_REQUIRE(d_queries && d_shard_keys && d_shard_counts, "null device buffer");
    int32_t rc = nested_args(n_queries, k);
    if (rc) return rc;
    if ((rc = refuse_hamming(view->sim, "nested search")) != OSK_OK) return rc;
    rc = any_device();
    if (rc) return rc;
    rc = check_device(view->device);
    if (rc) return rc;
    hipStream_t st = stream_or_default(stream, view->device);
    std::lock_guard<std::mutex> lk(view->mu);
    return view_nested_device(view, d_queries, n_queries, k, d_accept, d_shard_keys, d_shard_counts, d_visited, st);
    OSK_GUARD_END
}

int32_t osk_seg_set_parents(osk_seg* seg, const uint64_t* parent_bits) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(seg != nullptr && parent_bits != nullptr, "null argument");
    int32_t rc = any_device();
    if (rc) return rc;
    rc = check_device(seg->device);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(seg->mu);
    OSK_REQUIRE(seg->n_parents == 0, "the segment's parents are already registered");
    const int64_t n_words = ((int64_t)seg->max_doc + 63) / 64;
    // word_rank[w] = parent bits in words [0, w); bits at or past max_doc do not count
    std::vector<uint64_t> bits(std::max<int64_t>(1, n_words), 0ull);
    std::vector<int32_t> rank(std::max<int64_t>(1, n_words), 0);
    int64_t total = 0, last = -1;
    for (int64_t w = 0; w < n_words; ++w) {
        uint64_t m = parent_bits[w];
        const int64_t left = (int64_t)seg->max_doc - w * 64;
        if (left < 64) m &= (1ull << left) - 1ull;
        bits[w] = m;
        rank[w] = (int32_t)total;
        total += __builtin_popcountll(m);
        if (m) last = w * 64 + 63 - __builtin_clzll(m);
    }
    OSK_REQUIRE(total > 0, "the parent bitset is empty");
    hipStream_t st = device_stream(seg->device);
    int32_t last_doc = -1;   // the last vector's doc
    if (seg->n_rows > 0) {
        if (seg->d_ord_to_doc.p)
            OSK_HIP(hipMemcpy(&last_doc, seg->d_ord_to_doc.as<int32_t>() + (seg->n_rows - 1), sizeof(int32_t),
                              hipMemcpyDeviceToHost));
        else
            last_doc = (int32_t)(seg->n_rows - 1);
    }
    OSK_REQUIRE((int64_t)last_doc <= last, "a vector's doc lies after the last parent doc");
    DevBuf rp;
    OSK_HIP(rp.reserve(std::max<int64_t>(1, seg->n_rows) * sizeof(int32_t)));
    if (seg->n_rows > 0) {
        DevBuf d_bits, d_rank;
        hipError_t e = d_bits.upload(bits, st);
        if (e == hipSuccess) e = d_rank.upload(rank, st);
        if (e == hipSuccess)
            e = launch_nest_parents(d_bits.as<uint64_t>(), d_rank.as<int32_t>(), n_words,
                                    seg->d_ord_to_doc.as<int32_t>(), seg->n_rows, rp.as<int32_t>(), st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);   // (the temporaries are freed on return)
        if (e != hipSuccess) {
            set_error(std::string("osk_seg_set_parents: ") + hipGetErrorString(e));
            return OSK_ERR_DEVICE;
        }
    }
    seg->d_row_parent = std::move(rp);
    seg->n_parents = total;
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_seg_parents(const osk_seg* seg, int64_t* n_parents) {
    OSK_GUARD_BEGIN
    OSK_REQUIRE(seg != nullptr && n_parents != nullptr, "null argument");
    std::lock_guard<std::mutex> lk(const_cast<osk_seg*>(seg)->mu);
    *n_parents = seg->n_parents;
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_merge_device(int32_t device, const uint64_t* d_shard_keys, const int32_t* d_shard_counts,
                         const int32_t* d_shard_index, int32_t n_queries, int32_t n_shards, int32_t k,
                         int32_t from, int32_t size, float* d_scores, int32_t* d_docs,
                         int32_t* d_shard_out, int32_t* d_count, int64_t* d_total_hits,
                         float* d_max_score, void* stream) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(n_queries >= 1 && n_shards >= 1, "n_queries and n_shards must be >= 1");
    OSK_REQUIRE(k >= 1 && k <= OSK_MAX_K, "k must be in [1, OSK_MAX_K]");
    OSK_REQUIRE(from >= 0 && size >= 1 && (int64_t)from + size <= 100000, "bad from/size");
    OSK_REQUIRE(d_shard_keys && d_shard_counts && d_shard_index && d_scores && d_docs && d_shard_out &&
                    d_count && d_total_hits && d_max_score,
                "null device buffer");
    int32_t rc = check_device(device);
    if (rc) return rc;
    hipStream_t st = stream_or_default(stream, device);
    OSK_HIP(launch_coord_reduce(d_shard_keys, d_shard_counts, d_shard_index, n_queries, 1, n_shards, k,
                               from, size, d_scores, d_docs, d_shard_out, d_count, d_total_hits,
                               d_max_score, st));
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_merge_device_ranked(int32_t device, const uint64_t* d_keys, int32_t n_ranks,
                                int32_t shards_per_rank, const int32_t* d_shard_index, int32_t n_queries,
                                int32_t k, int32_t from, int32_t size, float* d_scores, int32_t* d_docs,
                                int32_t* d_shard_out, int32_t* d_count, int64_t* d_total_hits,
                                float* d_max_score, void* stream) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(n_queries >= 1 && n_ranks >= 1 && shards_per_rank >= 1,
                "n_queries, n_ranks and shards_per_rank must be >= 1");
    OSK_REQUIRE(k >= 1 && k <= OSK_MAX_K, "k must be in [1, OSK_MAX_K]");
    OSK_REQUIRE(from >= 0 && size >= 1 && (int64_t)from + size <= 100000, "bad from/size");
    OSK_REQUIRE(d_keys && d_shard_index && d_scores && d_docs && d_shard_out && d_count && d_total_hits &&
                    d_max_score,
                "null device buffer");
    int32_t rc = check_device(device);
    if (rc) return rc;
    hipStream_t st = stream_or_default(stream, device);
    OSK_HIP(launch_coord_reduce(d_keys, nullptr, d_shard_index, n_queries, n_ranks, shards_per_rank, k, from,
                               size, d_scores, d_docs, d_shard_out, d_count, d_total_hits, d_max_score, st));
    return OSK_OK;
    OSK_GUARD_END
}

// Scan-kernel timing for bench.py: enable, then read the mean duration of the scan launches of
// each search call (all query chunks of one call together) since enabling.
int32_t osk_view_profile(osk_view* v, int32_t enable) {
    OSK_GUARD_BEGIN
    OSK_REQUIRE(v != nullptr, "view is null");
    int32_t rc = check_device(v->device);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(v->mu);
    if (enable && !v->ev_start[0]) {
        for (int i = 0; i < osk_view::kEvRing; ++i) {
            OSK_HIP(hipEventCreate(&v->ev_start[i]));
            OSK_HIP(hipEventCreate(&v->ev_stop[i]));
        }
    }
    OSK_REQUIRE(enable >= 0, "enable must be >= 0");
    for (int i = 0; i < osk_view::kEvRing; ++i) v->ev_pending[i] = false;
    v->profile = false;
    v->profile_every = enable;
    v->profile_tick = 0;
    v->scan_ms = 0.0;
    v->scan_calls = 0;
    v->ev_next = 0;
    return OSK_OK;
    OSK_GUARD_END
}

// Test/debug only: copy an internal workspace buffer of the last search to host memory.
int32_t osk_view_debug_copy(osk_view* v, const char* name, void* host, int64_t bytes) {
    OSK_GUARD_BEGIN
#ifndef OSK_TESTING
    (void)v; (void)name; (void)host; (void)bytes;
    set_error("osk_view_debug_copy exists only in the testing build (libosknn_testing.so)");
    return OSK_ERR_UNSUPPORTED;
#else
    OSK_REQUIRE(v && name && host && bytes >= 0, "null argument");
    int32_t rc = check_device(v->device);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(v->mu);
    const std::string n(name);
    if (n == "sq8_lists") {   // (a host value: the [queries][lists][kKQ] shape of "sq8cand" / "sq8lb")
        OSK_REQUIRE(bytes == (int64_t)sizeof(int64_t), "sq8_lists is one int64");
        *static_cast<int64_t*>(host) = v->sq8_lists_last;
        return OSK_OK;
    }
    if (n == "sq6_tiles") {   // (a host copy: the view's tile table, TileDev {i32 seg, i32 shard, i64 row_begin, i64 row_end})
        OSK_REQUIRE((size_t)bytes <= sizeof(TileDev) * v->h_tiles.size(), "bytes exceed the tile table");
        std::memcpy(host, v->h_tiles.data(), (size_t)bytes);
        return OSK_OK;
    }
    if (n == "mfma_ks" || n == "mfma_c") {   // (host values of the bf16×3 path, set by its first search on the view)
        OSK_REQUIRE(v->mfma_ready, "the view has not taken the bf16x3 path yet");
        if (n == "mfma_ks") {
            OSK_REQUIRE(bytes == (int64_t)sizeof(int64_t), "mfma_ks is one int64");
            *static_cast<int64_t*>(host) = v->mfma_KS;
        } else {
            OSK_REQUIRE(bytes == (int64_t)sizeof(double), "mfma_c is one double");
            *static_cast<double*>(host) = v->mfma_c;
        }
        return OSK_OK;
    }
    static const struct {
        const char* name;
        DevBuf osk_view::*buf;
    } kBuffers[] = {
        {"acounts", &osk_view::ws_acounts}, {"pkeys", &osk_view::ws_pkeys},         {"pcounts", &osk_view::ws_pcounts},
        {"mfma_maxnorm2", &osk_view::d_shard_maxnorm2},
        {"akeys", &osk_view::ws_akeys},     {"cand_a", &osk_view::ws_cand_a},       {"flags", &osk_view::ws_flags},
        {"qsplit", &osk_view::ws_qsplit},   {"qnorm", &osk_view::ws_qnorm},         {"sq8cand", &osk_view::ws_sq8cand},
        {"sq8lb", &osk_view::ws_sq8lb},     {"qc", &osk_view::ws_qc},               {"settle_trace", &osk_view::ws_trace},
        {"sel_lb", &osk_view::ws_sel_lb},   {"sel_ub", &osk_view::ws_sel_ub},       {"nest_ub", &osk_view::ws_nest_ub},
        {"nest_lbkey", &osk_view::ws_nest_lbkey}, {"sq6cand", &osk_view::ws_cand6},   {"sq6cnt", &osk_view::ws_cnt6},
        {"sq6floor", &osk_view::ws_floor},
    };
    const DevBuf* b = nullptr;
    for (const auto& e : kBuffers)
        if (n == e.name) b = &(v->*e.buf);
    OSK_REQUIRE(b != nullptr, "unknown buffer");
    OSK_REQUIRE((size_t)bytes <= b->cap, "bytes exceed the buffer");
    OSK_HIP(hipDeviceSynchronize());   // the last search may be on any stream
    OSK_HIP(hipMemcpy(host, b->p, bytes, hipMemcpyDeviceToHost));
    return OSK_OK;
#endif
    OSK_GUARD_END
}

// The view and every replica its host entries leased (slots): counters are summed over them.
static std::vector<osk_view*> slot_views(osk_view* v) {
    std::lock_guard<std::mutex> lk(v->lease_mu);
    std::vector<osk_view*> out{v};
    out.insert(out.end(), v->replicas.begin(), v->replicas.end());
    return out;
}

int32_t osk_view_stats(osk_view* v, int64_t* batched_calls, int64_t* fallback_queries) {
    OSK_GUARD_BEGIN
    OSK_REQUIRE(v != nullptr && batched_calls && fallback_queries, "null argument");
    *batched_calls = *fallback_queries = 0;
    for (osk_view* s : slot_views(v)) {
        std::lock_guard<std::mutex> lk(s->mu);
        *batched_calls += s->mfma_calls;
        *fallback_queries += s->mfma_fallback_queries;
    }
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_view_counter(osk_view* v, const char* name, int64_t* value) {
    OSK_GUARD_BEGIN
    OSK_REQUIRE(v != nullptr && name != nullptr && value != nullptr, "null argument");
    int32_t rc = check_device(v->device);
    if (rc) return rc;
    const std::string n(name);
    if (n == "host_slots") {   // workspace slots the host entries have leased so far (1 + replicas)
        std::lock_guard<std::mutex> lk(v->lease_mu);
        *value = (int64_t)v->lease_busy.size();
        return OSK_OK;
    }
    if (n == "host_batches" || n == "host_batched_requests") {   // opportunistic batching of host calls
        std::lock_guard<std::mutex> lk(v->batcher.mu);
        *value = n == "host_batches" ? v->batcher.batches : v->batcher.requests;
        return OSK_OK;
    }
    if (n == "sq8_slices") {
        std::lock_guard<std::mutex> lk(v->mu);
        *value = v->n_slices;
        return OSK_OK;
    }
    if (n == "scan_tiles") {   // the view's scan tiles (the grid of its scan kernels)
        *value = v->n_tiles;
        return OSK_OK;
    }
    if (n == "seg_refs") {   // the references held on the view's segments, summed (readers, views, replicas)
        int64_t refs = 0;
        for (const osk_seg* sg : v->segs) refs += sg->refs.load();
        *value = refs;
        return OSK_OK;
    }
    if (n == "mfma_full_tiles") {   // (root view only)
        std::lock_guard<std::mutex> lk(v->mu);
        unsigned long long c = 0;
        if (v->d_mfma_full.p) {
            OSK_HIP(hipDeviceSynchronize());
            OSK_HIP(hipMemcpy(&c, v->d_mfma_full.p, sizeof(c), hipMemcpyDeviceToHost));
        }
        *value = (int64_t)c;
        return OSK_OK;
    }
    // every other counter: a device slot (Ctr) or a host member of the view, summed over the view and the
    // replicas its host entries leased
    static const struct {
        const char* name;
        int slot;                        // device slot, or -1:
        int64_t osk_view::*host;         // the host member
    } kCounters[] = {
        {"mfma_calls", -1, &osk_view::mfma_calls},
        {"mfma_fallback_queries", -1, &osk_view::mfma_fallback_queries},
        {"sq8_calls", -1, &osk_view::sq8_calls},
        {"sq6_calls", -1, &osk_view::sq6_calls},
        {"select_calls", -1, &osk_view::sel_calls},
        {"sq8_wide_calls", -1, &osk_view::sq8w_calls},
        {"threshold_calls", -1, &osk_view::thr_calls},
        {"threshold_sq8_calls", -1, &osk_view::thr_sq8_calls},
        {"threshold_top_calls", -1, &osk_view::thr_top_calls},
        {"threshold_top_select_calls", -1, &osk_view::thr_top_sel_calls},
        {"nested_calls", -1, &osk_view::nest_calls},
        {"nested_sq8_calls", -1, &osk_view::nest_sq8_calls},
        {"sq8_fallback_queries", kCtrFallbackQueries, nullptr},
        {"sq8_rescored_rows", kCtrRescoredRows, nullptr},
        {"sq8_exact_tiles", kCtrExactLists, nullptr},
        {"sq6_rebound_rows", kCtrSq6ReboundRows, nullptr},
        {"sq6_rebound_gathered_rows", kCtrSq6GatheredRows, nullptr},
        {"sq6_rebound_passes", kCtrSq6ReboundPasses, nullptr},
        {"sq6_rebound_max_wg_cycles", kCtrSq6MaxWgCycles, nullptr},
        {"sq6_tiles_own", kCtrSq6TilesOwn, nullptr},
        {"sq6_tiles_by_others", kCtrSq6TilesByOthers, nullptr},
        {"sq6_tiles_helped", kCtrSq6TilesHelped, nullptr},
        {"sq8_wide_events", kCtrWideEvents, nullptr},
        {"sq8_wide_pairs", kCtrWidePairs, nullptr},
        {"sq8_wide_wait_cycles", kCtrWideWaitCycles, nullptr},
        {"sq8_wide_slow_steps", kCtrWideSlowSteps, nullptr},
        {"sq8_wide_loop_cycles", kCtrWideLoopCycles, nullptr},
        {"sq8_wide_slow_cycles", kCtrWideSlowCycles, nullptr},
        {"sq8_wide_drain_cycles", kCtrWideDrainCycles, nullptr},
        {"sq8_rows_total_cycles", kCtrRowsTotalCycles, nullptr},
        {"sq8_rows_setup_cycles", kCtrRowsSetupCycles, nullptr},
        {"sq8_rows_quarter_end_cycles", kCtrRowsQuarterEndCycles, nullptr},
        {"sq8_rows_first_wait_cycles", kCtrRowsFirstWaitCycles, nullptr},
        {"sq8_rows_setup_barrier_cycles", kCtrRowsSetupBarrierCycles, nullptr},
        {"sq8_rows_setup_fragment_cycles", kCtrRowsSetupFragmentCycles, nullptr},
        {"threshold_sq8_settled_rows", kCtrThrSettledRows, nullptr},
        {"nested_sq8_settled_rows", kCtrNestSettledRows, nullptr},
    };
    const auto* ctr = std::find_if(std::begin(kCounters), std::end(kCounters), [&](const auto& e) { return n == e.name; });
    OSK_REQUIRE(ctr != std::end(kCounters), "unknown counter: " + n);
    int64_t sum = 0;
    for (osk_view* s : slot_views(v)) {
        std::lock_guard<std::mutex> lk(s->mu);
        if (ctr->host) {
            sum += s->*ctr->host;
        } else if (s->d_counters.p) {
            unsigned long long c = 0;
            OSK_HIP(hipDeviceSynchronize());   // the last search may be on any stream
            OSK_HIP(hipMemcpy(&c, s->d_counters.as<unsigned long long>() + ctr->slot, sizeof(c), hipMemcpyDeviceToHost));
            sum += (int64_t)c;
        }
    }
    *value = sum;
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_view_scan_time(osk_view* v, double* total_ms, int64_t* calls) {
    OSK_GUARD_BEGIN
    OSK_REQUIRE(v != nullptr && total_ms && calls, "null argument");
    int32_t rc = check_device(v->device);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(v->mu);
    for (int i = 0; i < osk_view::kEvRing; ++i) {
        rc = profile_fold(v, i);
        if (rc) return rc;
    }
    *total_ms = v->scan_ms;
    *calls = v->scan_calls;
    return OSK_OK;
    OSK_GUARD_END
}

// Host-buffer search + coordinator merge on one device (synchronous).
static int32_t view_search_host(osk_view* v, const void* queries, int32_t n_queries, int32_t k, int32_t from,
                                int32_t size, const uint64_t* const* accept, float* out_scores,
                                int32_t* out_docs, int32_t* out_shard_index, int32_t* out_count,
                                int64_t* out_total_hits, float* out_max_score, ShardTopK core) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(v != nullptr && queries != nullptr, "null argument");
    OSK_REQUIRE(out_scores && out_docs && out_shard_index && out_count && out_total_hits && out_max_score,
                "null output");
    OSK_REQUIRE(n_queries >= 1, "n_queries must be >= 1");
    OSK_REQUIRE(from >= 0 && size >= 1, "bad from/size");
    int32_t rc = check_device(v->device);
    if (rc) return rc;
    HostCall call;
    if ((rc = call.begin(v)) != OSK_OK) return rc;
    v = call.v;
    hipStream_t st = call.st;
    const int nq = n_queries, S = v->n_shards;
    const size_t qbytes = (size_t)nq * v->dim * elem_bytes(v->enc);
    const uint64_t* const* d_acc = nullptr;
    if ((rc = upload_accept(v, accept, st, &d_acc)) != OSK_OK) return rc;
    OSK_HIP(v->ws_qin.reserve(std::max<size_t>(16, qbytes)));
    OSK_HIP(hipMemcpyAsync(v->ws_qin.p, queries, qbytes, hipMemcpyHostToDevice, st));
    OSK_HIP(v->ws_keys.reserve(sizeof(uint64_t) * (size_t)nq * S * k));
    OSK_HIP(v->ws_counts.reserve(sizeof(int32_t) * (size_t)nq * S));
    rc = core(v, v->ws_qin.p, nq, k, d_acc, v->ws_keys.as<uint64_t>(), v->ws_counts.as<int32_t>(), nullptr, st);
    if (rc) return rc;
    const MergedOut out(nq, size);
    OSK_HIP(v->ws_out.reserve(out.total_bytes));
    const MergedOut::Ptrs o = out.at(v->ws_out.as<char>());
    OSK_HIP(launch_coord_reduce(v->ws_keys.as<uint64_t>(), v->ws_counts.as<int32_t>(),
                               v->d_shard_index.as<int32_t>(), nq, 1, S, k, from, size, o.scores, o.docs, o.shard,
                               o.count, o.total, o.max, st));
    OSK_HIP(v->h_stage.reserve(out.total_bytes));
    OSK_HIP(hipMemcpyAsync(v->h_stage.p, v->ws_out.p, out.total_bytes, hipMemcpyDeviceToHost, st));
    if ((rc = call.finish()) != OSK_OK) return rc;
    out.copy_out(static_cast<const char*>(v->h_stage.p), out_scores, out_docs, out_shard_index, out_count,
                 out_total_hits, out_max_score);
    return OSK_OK;
    OSK_GUARD_END
}

static int32_t seg_search_host(osk_seg* seg, const void* queries, int32_t n_queries, int32_t k,
                               const uint64_t* accept_bits, float* out_scores, int32_t* out_docs,
                               int32_t* out_count, int64_t* out_visited, ShardTopK core) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(seg != nullptr && queries != nullptr, "null argument");
    OSK_REQUIRE(out_scores && out_docs && out_count, "null output");
    OSK_REQUIRE(n_queries >= 1, "n_queries must be >= 1");
    OSK_REQUIRE(k >= 1 && k <= OSK_MAX_K, "k must be in [1, OSK_MAX_K]");
    int32_t rc = check_device(seg->device);
    if (rc) return rc;
    osk_view* v;
    if ((rc = seg_self_view(seg, &v)) != OSK_OK) return rc;
    (void)hipSetDevice(seg->device);
    HostCall call;
    if ((rc = call.begin(v)) != OSK_OK) return rc;
    v = call.v;
    hipStream_t st = call.st;
    const int nq = n_queries;
    const size_t qbytes = (size_t)nq * seg->dim * elem_bytes(seg->enc);
    const uint64_t* const acc[1] = {accept_bits};
    const uint64_t* const* d_acc = nullptr;
    if ((rc = upload_accept(v, acc, st, &d_acc)) != OSK_OK) return rc;
    OSK_HIP(v->ws_qin.reserve(std::max<size_t>(16, qbytes)));
    OSK_HIP(hipMemcpyAsync(v->ws_qin.p, queries, qbytes, hipMemcpyHostToDevice, st));
    OSK_HIP(v->ws_keys.reserve(sizeof(uint64_t) * (size_t)nq * k));
    OSK_HIP(v->ws_counts.reserve(sizeof(int32_t) * (size_t)nq));
    OSK_HIP(v->ws_visited.reserve(sizeof(int64_t)));
    rc = core(v, v->ws_qin.p, nq, k, d_acc, v->ws_keys.as<uint64_t>(), v->ws_counts.as<int32_t>(),
              v->ws_visited.as<int64_t>(), st);
    if (rc) return rc;
    const size_t kb = sizeof(uint64_t) * (size_t)nq * k, cb = sizeof(int32_t) * nq;
    OSK_HIP(v->h_stage.reserve(kb + cb + 8));
    char* hb = static_cast<char*>(v->h_stage.p);
    OSK_HIP(hipMemcpyAsync(hb, v->ws_keys.p, kb, hipMemcpyDeviceToHost, st));
    OSK_HIP(hipMemcpyAsync(hb + kb, v->ws_counts.p, cb, hipMemcpyDeviceToHost, st));
    OSK_HIP(hipMemcpyAsync(hb + kb + cb, v->ws_visited.p, 8, hipMemcpyDeviceToHost, st));
    if ((rc = call.finish()) != OSK_OK) return rc;
    const uint64_t* keys = reinterpret_cast<const uint64_t*>(hb);
    const int32_t* cnt = reinterpret_cast<const int32_t*>(hb + kb);
    int64_t visited;
    std::memcpy(&visited, hb + kb + cb, 8);
    for (int q = 0; q < nq; ++q) {
        out_count[q] = cnt[q];
        for (int i = 0; i < k; ++i) {
            const uint64_t key = keys[(size_t)q * k + i];
            const size_t o = (size_t)q * k + i;
            if (i < cnt[q]) {
                out_scores[o] = key_score(key);
                out_docs[o] = key_doc(key);
            } else {
                out_scores[o] = -__builtin_inff();
                out_docs[o] = 0x7FFFFFFF;
            }
        }
        if (out_visited) out_visited[q] = visited;
    }
    return OSK_OK;
    OSK_GUARD_END
}

// Opportunistic batching of concurrent host calls ("batches concurrent single-query
// calls opportunistically").  A call queues its request on the view; while fewer than host_batch_leaders
// batches are in flight, a waiting caller becomes a leader, takes the compatible requests queued so far
// (FIFO, same k / from / size, no filter, ≤ 32 queries) and runs them as ONE batched search (the int8
// MFMA prefilter reads the corpus once for all of them), then hands every request its rows (at most
// host_batch_leaders batches in flight per view).  No
// artificial delay: requests batch up only while the device is busy with earlier ones.  Results are
// identical to unbatched calls (every path is exact).
}  // extern "C"

namespace {

constexpr int kBatchMaxQueries = 32;

struct BatchReq {
    const void* queries;
    int nq, k, from, size;
    float* sc;
    int32_t* docs;
    int32_t* shard;
    int32_t* cnt;
    int64_t* tot;
    float* mx;
    int64_t* visited;
    int32_t rc = OSK_OK;
    std::string err;
    bool done = false;
    int64_t device_ns = -1;   // the serving launch chain's device time (call_timing) ...
    int32_t shared = 0;       // ... and how many requests it served
};

// run `fn(batch, total_queries)` as a leader whenever possible until `me` is done
template <class Fn>
int32_t batched_call(osk_view* root, BatchReq& me, Fn&& fn) {
    auto& B = root->batcher;
    std::unique_lock<std::mutex> lk(B.mu);
    B.queue.push_back(&me);
    while (!me.done) {
        if (!B.queue.empty() && B.leaders < (int)g_tuning.host_batch_leaders) {
            std::vector<BatchReq*> batch;
            int total = 0;
            const BatchReq* f = static_cast<const BatchReq*>(B.queue.front());
            for (auto it = B.queue.begin(); it != B.queue.end();) {
                BatchReq* r = static_cast<BatchReq*>(*it);
                if (r->k == f->k && r->from == f->from && r->size == f->size && total + r->nq <= kBatchMaxQueries) {
                    batch.push_back(r);
                    total += r->nq;
                    it = B.queue.erase(it);
                } else {
                    ++it;
                }
            }
            ++B.leaders;
            lk.unlock();
            int32_t rc;
            t_call_ns = -1;
            try {   // the batch's requests must always be completed, whatever happens
                rc = fn(batch, total);
            } catch (const std::bad_alloc&) {
                set_error("host allocation failed");
                rc = OSK_ERR_OOM;
            } catch (...) {
                set_error("batched search failed");
                rc = OSK_ERR_INVALID;
            }
            const std::string err = rc ? std::string(osk_last_error()) : std::string();
            lk.lock();
            for (BatchReq* r : batch) {
                r->rc = rc;
                r->err = err;
                r->device_ns = t_call_ns;
                r->shared = t_call_ns >= 0 ? (int32_t)batch.size() : 0;
                r->done = true;
            }
            --B.leaders;
            B.batches += 1;
            B.requests += (int64_t)batch.size();
            B.cv.notify_all();
        } else {
            B.cv.wait(lk);
        }
    }
    t_call_ns = me.device_ns;
    t_call_shared = me.shared;
    if (me.rc) set_error("batched search: " + me.err);
    return me.rc;
}

}  // namespace

extern "C" {

int32_t osk_view_search(osk_view* v, const void* queries, int32_t n_queries, int32_t k, int32_t from,
                        int32_t size, const uint64_t* const* accept, float* out_scores,
                        int32_t* out_docs, int32_t* out_shard_index, int32_t* out_count,
                        int64_t* out_total_hits, float* out_max_score) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(v != nullptr && queries != nullptr, "null argument");
    bool any_bits = false;
    for (int i = 0; accept && i < (int)v->segs.size(); ++i) any_bits |= accept[i] != nullptr;
    if (any_bits || !g_tuning.host_batching || n_queries < 1 || n_queries > kBatchMaxQueries)
        return view_search_host(v, queries, n_queries, k, from, size, accept, out_scores, out_docs, out_shard_index,
                                out_count, out_total_hits, out_max_score, view_search_device);
    BatchReq me{queries, n_queries, k, from, size, out_scores, out_docs, out_shard_index, out_count,
                out_total_hits, out_max_score, nullptr};
    const size_t qrow = (size_t)v->dim * elem_bytes(v->enc);
    return batched_call(v, me, [&](const std::vector<BatchReq*>& batch, int total) -> int32_t {
        if (batch.size() == 1) {
            BatchReq* r = batch[0];
            return view_search_host(v, r->queries, r->nq, r->k, r->from, r->size, nullptr, r->sc, r->docs, r->shard,
                                    r->cnt, r->tot, r->mx, view_search_device);
        }
        const int sz = batch[0]->size;
        std::vector<char> q((size_t)total * qrow);
        std::vector<float> sc((size_t)total * sz), mx(total);
        std::vector<int32_t> dc((size_t)total * sz), sh((size_t)total * sz), cnt(total);
        std::vector<int64_t> tot(total);
        int off = 0;
        for (BatchReq* r : batch) {
            std::memcpy(q.data() + (size_t)off * qrow, r->queries, (size_t)r->nq * qrow);
            off += r->nq;
        }
        const int32_t rc = view_search_host(v, q.data(), total, batch[0]->k, batch[0]->from, sz, nullptr, sc.data(),
                                            dc.data(), sh.data(), cnt.data(), tot.data(), mx.data(),
                                            view_search_device);
        if (rc) return rc;
        off = 0;
        for (BatchReq* r : batch) {
            const size_t o = (size_t)off * sz, n = (size_t)r->nq * sz;
            std::memcpy(r->sc, sc.data() + o, n * 4);
            std::memcpy(r->docs, dc.data() + o, n * 4);
            std::memcpy(r->shard, sh.data() + o, n * 4);
            std::memcpy(r->cnt, cnt.data() + off, (size_t)r->nq * 4);
            std::memcpy(r->tot, tot.data() + off, (size_t)r->nq * 8);
            std::memcpy(r->mx, mx.data() + off, (size_t)r->nq * 4);
            off += r->nq;
        }
        return OSK_OK;
    });
    OSK_GUARD_END
}

// [L] KnnVectorsReader.search on one segment (host buffers, synchronous).
int32_t osk_seg_search(osk_seg* seg, const void* queries, int32_t n_queries, int32_t k,
                       const uint64_t* accept_bits, float* out_scores, int32_t* out_docs,
                       int32_t* out_count, int64_t* out_visited) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(seg != nullptr && queries != nullptr, "null argument");
    if (accept_bits || !g_tuning.host_batching || n_queries < 1 || n_queries > kBatchMaxQueries)
        return seg_search_host(seg, queries, n_queries, k, accept_bits, out_scores, out_docs, out_count, out_visited,
                               view_search_device);
    osk_view* root;
    const int32_t rc_view = seg_self_view(seg, &root);
    if (rc_view) return rc_view;
    BatchReq me{queries, n_queries, k, 0, k, out_scores, out_docs, nullptr, out_count, nullptr, nullptr, out_visited};
    const size_t qrow = (size_t)seg->dim * elem_bytes(seg->enc);
    return batched_call(root, me, [&](const std::vector<BatchReq*>& batch, int total) -> int32_t {
        if (batch.size() == 1) {
            BatchReq* r = batch[0];
            return seg_search_host(seg, r->queries, r->nq, r->k, nullptr, r->sc, r->docs, r->cnt, r->visited,
                                   view_search_device);
        }
        const int kk = batch[0]->k;
        std::vector<char> q((size_t)total * qrow);
        std::vector<float> sc((size_t)total * kk);
        std::vector<int32_t> dc((size_t)total * kk), cnt(total);
        std::vector<int64_t> vis(total);
        int off = 0;
        for (BatchReq* r : batch) {
            std::memcpy(q.data() + (size_t)off * qrow, r->queries, (size_t)r->nq * qrow);
            off += r->nq;
        }
        const int32_t rc = seg_search_host(seg, q.data(), total, kk, nullptr, sc.data(), dc.data(), cnt.data(),
                                           vis.data(), view_search_device);
        if (rc) return rc;
        off = 0;
        for (BatchReq* r : batch) {
            const size_t o = (size_t)off * kk, n = (size_t)r->nq * kk;
            std::memcpy(r->sc, sc.data() + o, n * 4);
            std::memcpy(r->docs, dc.data() + o, n * 4);
            std::memcpy(r->cnt, cnt.data() + off, (size_t)r->nq * 4);
            if (r->visited) std::memcpy(r->visited, vis.data() + off, (size_t)r->nq * 8);
            off += r->nq;
        }
        return OSK_OK;
    });
    OSK_GUARD_END
}

// Host-buffer threshold search over a view (synchronous): leases a workspace slot and its stream like
// view_search_host; never joins the opportunistic batching.  accept: null or n_segs host bitsets;
// out_visited: null or n_segs.
static int32_t threshold_host(osk_view* v, const void* queries, int32_t n_queries, const float* min_scores,
                              const uint64_t* const* accept, int32_t cap, int32_t* out_docs, float* out_scores,
                              int32_t* out_count, int64_t* out_total, int64_t* out_visited) {
    HostCall call;
    int32_t rc = call.begin(v);
    if (rc) return rc;
    v = call.v;
    hipStream_t st = call.st;
    const int nq = n_queries, S = v->n_shards, ns = (int)v->segs.size();
    const size_t qbytes = (size_t)nq * v->dim * elem_bytes(v->enc);
    const uint64_t* const* d_acc = nullptr;
    if ((rc = upload_accept(v, accept, st, &d_acc)) != OSK_OK) return rc;
    OSK_HIP(v->ws_qin.reserve(std::max<size_t>(16, qbytes)));
    OSK_HIP(hipMemcpyAsync(v->ws_qin.p, queries, qbytes, hipMemcpyHostToDevice, st));
    OSK_HIP(v->ws_thr_min.reserve(sizeof(float) * nq));
    OSK_HIP(hipMemcpyAsync(v->ws_thr_min.p, min_scores, sizeof(float) * nq, hipMemcpyHostToDevice, st));
    // outputs: docs i32 | scores f32 | count i32 | total i64 | visited i64
    const size_t n_out = (size_t)nq * S * cap, n_qs = (size_t)nq * S;
    const size_t o_doc = 0, o_sc = o_doc + n_out * 4, o_cnt = o_sc + n_out * 4, o_tot = (o_cnt + n_qs * 4 + 7) / 8 * 8,
                 o_vis = o_tot + n_qs * 8, total_b = o_vis + (size_t)ns * 8;
    OSK_HIP(v->ws_thr_out.reserve(total_b));
    char* ob = v->ws_thr_out.as<char>();
    rc = view_threshold_device(v, v->ws_qin.p, nq, v->ws_thr_min.as<float>(), d_acc, cap,
                               reinterpret_cast<int32_t*>(ob + o_doc), reinterpret_cast<float*>(ob + o_sc),
                               reinterpret_cast<int32_t*>(ob + o_cnt), reinterpret_cast<int64_t*>(ob + o_tot),
                               reinterpret_cast<int64_t*>(ob + o_vis), st);
    if (rc) return rc;
    OSK_HIP(v->h_stage.reserve(total_b));
    OSK_HIP(hipMemcpyAsync(v->h_stage.p, ob, total_b, hipMemcpyDeviceToHost, st));
    if ((rc = call.finish()) != OSK_OK) return rc;
    const char* hb = static_cast<const char*>(v->h_stage.p);
    std::memcpy(out_docs, hb + o_doc, n_out * 4);
    std::memcpy(out_scores, hb + o_sc, n_out * 4);
    std::memcpy(out_count, hb + o_cnt, n_qs * 4);
    std::memcpy(out_total, hb + o_tot, n_qs * 8);
    if (out_visited) std::memcpy(out_visited, hb + o_vis, (size_t)ns * 8);
    return OSK_OK;
}

int32_t osk_view_search_threshold(osk_view* view, const void* queries, int32_t n_queries, const float* min_scores,
                                  const uint64_t* const* accept, int32_t cap, int32_t* out_docs, float* out_scores,
                                  int32_t* out_count, int64_t* out_total) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(view != nullptr && queries != nullptr && min_scores != nullptr, "null argument");
    OSK_REQUIRE(out_docs && out_scores && out_count && out_total, "null output");
    OSK_REQUIRE(n_queries >= 1, "n_queries must be >= 1");
    OSK_REQUIRE(cap >= 1, "cap must be >= 1");
    int32_t rc = refuse_hamming(view->sim, "similarity-threshold search");
    if (rc) return rc;
    rc = any_device();
    if (rc) return rc;
    rc = check_device(view->device);
    if (rc) return rc;
    return threshold_host(view, queries, n_queries, min_scores, accept, cap, out_docs, out_scores, out_count,
                          out_total, nullptr);
    OSK_GUARD_END
}

int32_t osk_seg_search_threshold(osk_seg* seg, const void* queries, int32_t n_queries, const float* min_scores,
                                 const uint64_t* accept_bits, int32_t cap, int32_t* out_docs, float* out_scores,
                                 int32_t* out_count, int64_t* out_total, int64_t* out_visited) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(seg != nullptr && queries != nullptr && min_scores != nullptr, "null argument");
    OSK_REQUIRE(out_docs && out_scores && out_count && out_total, "null output");
    OSK_REQUIRE(n_queries >= 1, "n_queries must be >= 1");
    OSK_REQUIRE(cap >= 1, "cap must be >= 1");
    int32_t rc = refuse_hamming(seg->sim, "similarity-threshold search");
    if (rc) return rc;
    rc = any_device();
    if (rc) return rc;
    rc = check_device(seg->device);
    if (rc) return rc;
    osk_view* v;
    if ((rc = seg_self_view(seg, &v)) != OSK_OK) return rc;
    (void)hipSetDevice(seg->device);
    const uint64_t* const acc[1] = {accept_bits};
    int64_t visited = 0;
    rc = threshold_host(v, queries, n_queries, min_scores, acc, cap, out_docs, out_scores, out_count, out_total,
                        &visited);
    if (rc) return rc;
    for (int q = 0; out_visited && q < n_queries; ++q) out_visited[q] = visited;
    return OSK_OK;
    OSK_GUARD_END
}

// The device part of both host top-k threshold entries, on the leased slot `v` and its stream: queries, thresholds
// and bitsets uploaded, then the core.  Leaves the shard lists in ws_keys / ws_counts, the exact totals in
// ws_thr_tot [nq][S] and, when asked, the visited counts in ws_visited [n_segs].
static int32_t threshold_top_shards(osk_view* v, hipStream_t st, const void* queries, int nq, const float* min_scores,
                                    int k, const uint64_t* const* accept, bool want_visited) {
    const int S = v->n_shards;
    const size_t qbytes = (size_t)nq * v->dim * elem_bytes(v->enc);
    const uint64_t* const* d_acc = nullptr;
    int32_t rc = upload_accept(v, accept, st, &d_acc);
    if (rc) return rc;
    OSK_HIP(v->ws_qin.reserve(std::max<size_t>(16, qbytes)));
    OSK_HIP(hipMemcpyAsync(v->ws_qin.p, queries, qbytes, hipMemcpyHostToDevice, st));
    OSK_HIP(v->ws_thr_min.reserve(sizeof(float) * nq));
    OSK_HIP(hipMemcpyAsync(v->ws_thr_min.p, min_scores, sizeof(float) * nq, hipMemcpyHostToDevice, st));
    OSK_HIP(v->ws_keys.reserve(sizeof(uint64_t) * (size_t)nq * S * k));
    OSK_HIP(v->ws_counts.reserve(sizeof(int32_t) * (size_t)nq * S));
    OSK_HIP(v->ws_thr_tot.reserve(sizeof(int64_t) * (size_t)nq * S));
    if (want_visited) OSK_HIP(v->ws_visited.reserve(sizeof(int64_t) * v->segs.size()));
    return view_threshold_top_device(v, v->ws_qin.p, nq, v->ws_thr_min.as<float>(), k, d_acc, v->ws_keys.as<uint64_t>(),
                                     v->ws_counts.as<int32_t>(), v->ws_thr_tot.as<int64_t>(),
                                     want_visited ? v->ws_visited.as<int64_t>() : nullptr, st);
}

int32_t osk_view_search_threshold_top(osk_view* view, const void* queries, int32_t n_queries, const float* min_scores,
                                      int32_t k, int32_t from, int32_t size, const uint64_t* const* accept,
                                      float* out_scores, int32_t* out_docs, int32_t* out_shard_index,
                                      int32_t* out_count, int64_t* out_total_hits, float* out_max_score) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(view != nullptr && queries != nullptr && min_scores != nullptr, "null argument");
    OSK_REQUIRE(out_scores && out_docs && out_shard_index && out_count && out_total_hits && out_max_score,
                "null output");
    int32_t rc = threshold_top_args(n_queries, k);
    if (rc) return rc;
    OSK_REQUIRE(from >= 0 && size >= 1, "bad from/size");
    if ((rc = refuse_hamming(view->sim, "similarity-threshold search")) != OSK_OK) return rc;
    rc = any_device();
    if (rc) return rc;
    rc = check_device(view->device);
    if (rc) return rc;
    HostCall call;
    if ((rc = call.begin(view)) != OSK_OK) return rc;
    osk_view* v = call.v;
    hipStream_t st = call.st;
    const int nq = n_queries, S = v->n_shards;
    if ((rc = threshold_top_shards(v, st, queries, nq, min_scores, k, accept, false)) != OSK_OK) return rc;
    // the coordinator reduce over the shard lists, as osk_view_search; its total counts the keys the lists
    // hold, so the exact totals come back beside it and are summed here
    const MergedOut out(nq, size);
    OSK_HIP(v->ws_out.reserve(out.total_bytes));
    const MergedOut::Ptrs o = out.at(v->ws_out.as<char>());
    OSK_HIP(launch_coord_reduce(v->ws_keys.as<uint64_t>(), v->ws_counts.as<int32_t>(),
                               v->d_shard_index.as<int32_t>(), nq, 1, S, k, from, size, o.scores, o.docs, o.shard,
                               o.count, o.total, o.max, st));
    const size_t o_tot = (out.total_bytes + 7) / 8 * 8, b_tot = sizeof(int64_t) * (size_t)nq * S;
    OSK_HIP(v->h_stage.reserve(o_tot + b_tot));
    char* hb = static_cast<char*>(v->h_stage.p);
    OSK_HIP(hipMemcpyAsync(hb, v->ws_out.p, out.total_bytes, hipMemcpyDeviceToHost, st));
    OSK_HIP(hipMemcpyAsync(hb + o_tot, v->ws_thr_tot.p, b_tot, hipMemcpyDeviceToHost, st));
    if ((rc = call.finish()) != OSK_OK) return rc;
    out.copy_out(hb, out_scores, out_docs, out_shard_index, out_count, out_total_hits, out_max_score);
    const int64_t* tot = reinterpret_cast<const int64_t*>(hb + o_tot);
    for (int q = 0; q < nq; ++q) {
        int64_t sum = 0;
        for (int s = 0; s < S; ++s) sum += tot[(size_t)q * S + s];
        out_total_hits[q] = sum;
    }
    return OSK_OK;
    OSK_GUARD_END
}

int32_t osk_seg_search_threshold_top(osk_seg* seg, const void* queries, int32_t n_queries, const float* min_scores,
                                     int32_t k, const uint64_t* accept_bits, float* out_scores, int32_t* out_docs,
                                     int32_t* out_count, int64_t* out_total, int64_t* out_visited) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(seg != nullptr && queries != nullptr && min_scores != nullptr, "null argument");
    OSK_REQUIRE(out_scores && out_docs && out_count && out_total, "null output");
    int32_t rc = threshold_top_args(n_queries, k);
    if (rc) return rc;
    if ((rc = refuse_hamming(seg->sim, "similarity-threshold search")) != OSK_OK) return rc;
    rc = any_device();
    if (rc) return rc;
    rc = check_device(seg->device);
    if (rc) return rc;
    osk_view* root;
    if ((rc = seg_self_view(seg, &root)) != OSK_OK) return rc;
    (void)hipSetDevice(seg->device);
    HostCall call;
    if ((rc = call.begin(root)) != OSK_OK) return rc;
    osk_view* v = call.v;
    hipStream_t st = call.st;
    const int nq = n_queries;
    const uint64_t* const acc[1] = {accept_bits};
    if ((rc = threshold_top_shards(v, st, queries, nq, min_scores, k, acc, true)) != OSK_OK) return rc;
    // keys u64 | totals i64 | visited i64 | counts i32
    const size_t kb = sizeof(uint64_t) * (size_t)nq * k, tb = sizeof(int64_t) * (size_t)nq, cb = sizeof(int32_t) * nq;
    OSK_HIP(v->h_stage.reserve(kb + tb + 8 + cb));
    char* hb = static_cast<char*>(v->h_stage.p);
    OSK_HIP(hipMemcpyAsync(hb, v->ws_keys.p, kb, hipMemcpyDeviceToHost, st));
    OSK_HIP(hipMemcpyAsync(hb + kb, v->ws_thr_tot.p, tb, hipMemcpyDeviceToHost, st));
    OSK_HIP(hipMemcpyAsync(hb + kb + tb, v->ws_visited.p, 8, hipMemcpyDeviceToHost, st));
    OSK_HIP(hipMemcpyAsync(hb + kb + tb + 8, v->ws_counts.p, cb, hipMemcpyDeviceToHost, st));
    if ((rc = call.finish()) != OSK_OK) return rc;
    const uint64_t* keys = reinterpret_cast<const uint64_t*>(hb);
    const int64_t* tot = reinterpret_cast<const int64_t*>(hb + kb);
    const int32_t* cnt = reinterpret_cast<const int32_t*>(hb + kb + tb + 8);
    int64_t visited;
    std::memcpy(&visited, hb + kb + tb, 8);
    for (int q = 0; q < nq; ++q) {
        out_count[q] = cnt[q];
        out_total[q] = tot[q];
        for (int i = 0; i < k; ++i) {
            const uint64_t key = keys[(size_t)q * k + i];
            const size_t o = (size_t)q * k + i;
            out_scores[o] = i < cnt[q] ? key_score(key) : -__builtin_inff();
            out_docs[o] = i < cnt[q] ? key_doc(key) : 0x7FFFFFFF;
        }
        if (out_visited) out_visited[q] = visited;
    }
    return OSK_OK;
    OSK_GUARD_END
}

// Nested k-NN over a view / one segment, host buffers (synchronous): the host k-NN entries' route — a leased
// workspace slot, the coordinator reduce — with the per-shard top k taken over parents; never batched with
// other callers.
int32_t osk_view_search_nested(osk_view* view, const void* queries, int32_t n_queries, int32_t k, int32_t from,
                               int32_t size, const uint64_t* const* accept, float* out_scores, int32_t* out_docs,
                               int32_t* out_shard_index, int32_t* out_count, int64_t* out_total_hits,
                               float* out_max_score) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(view != nullptr && queries != nullptr, "null argument");
    OSK_REQUIRE(out_scores && out_docs && out_shard_index && out_count && out_total_hits && out_max_score,
                "null output");
    OSK_REQUIRE(from >= 0 && size >= 1, "bad from/size");
    int32_t rc = nested_args(n_queries, k);
    if (rc) return rc;
    if ((rc = refuse_hamming(view->sim, "nested search")) != OSK_OK) return rc;
    rc = any_device();
    if (rc) return rc;
    return view_search_host(view, queries, n_queries, k, from, size, accept, out_scores, out_docs, out_shard_index,
                            out_count, out_total_hits, out_max_score, view_nested_device);
    OSK_GUARD_END
}

int32_t osk_seg_search_nested(osk_seg* seg, const void* queries, int32_t n_queries, int32_t k,
                              const uint64_t* accept_bits, float* out_scores, int32_t* out_docs, int32_t* out_count,
                              int64_t* out_visited) {
    OSK_GUARD_BEGIN
    clear_error();
    OSK_REQUIRE(seg != nullptr && queries != nullptr, "null argument");
    OSK_REQUIRE(out_scores && out_docs && out_count, "null output");
    int32_t rc = nested_args(n_queries, k);
    if (rc) return rc;
    if ((rc = refuse_hamming(seg->sim, "nested search")) != OSK_OK) return rc;
    rc = any_device();
    if (rc) return rc;
    return seg_search_host(seg, queries, n_queries, k, accept_bits, out_scores, out_docs, out_count, out_visited,
                           view_nested_device);
    OSK_GUARD_END
}

int32_t osk_last_call_device_ns(int64_t* device_ns, int32_t* shared_by) {
    OSK_GUARD_BEGIN
    OSK_REQUIRE(device_ns != nullptr, "null argument");
    *device_ns = t_call_ns;
    if (shared_by) *shared_by = t_call_shared;
    return OSK_OK;
    OSK_GUARD_END
}

}  // extern "C"
