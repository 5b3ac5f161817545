// pimemb_engine.cpp -- host side of libpimemb.so: the `emb_*` C ABI declared in include/pimemb.h.
//
// Replaces the host runtime of the reference, upmem/include/emb_host.h:
//   populate_mram (:136-183)  -> emb_alloc_table / emb_load_table / emb_load_table_column
//   lookup        (:234-404)  -> emb_lookup / emb_lookup_batched / emb_plan_*
//   post_process  (:186-222)  -> gone (conversion and [bag][col] layout are fused in the kernel)
// There is NO CPU compute path in this file: every lookup is a HIP kernel launch; if the GPU or
// the runtime is unavailable the call fails with EMB_ERR_DEVICE.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <unordered_map>
#include <vector>

#include "pimemb_hostcopy.h"
#include "pimemb_hot_rows.h"
#include "pimemb_internal.h"
#include "pimemb_xcd_map.h"

namespace pimemb {
hipError_t launch_store_word(volatile unsigned long long *dst, unsigned long long value, hipStream_t stream);   // pimemb_kernels.hip
}
using pimemb::DevDesc;
using pimemb::KernelKind;
using pimemb::LaunchGeom;

namespace {

thread_local std::string g_last_error;
using pimemb::fail;

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return fail(_e == hipErrorOutOfMemory ? EMB_ERR_NOMEM : EMB_ERR_DEVICE,         \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,    \
                        __LINE__);                                                          \
    } while (0)
#define EMB_TRY(expr)                  \
    do {                               \
        int _rc = (expr);              \
        if (_rc != EMB_OK) return _rc; \
    } while (0)

double now_us() {
    using namespace std::chrono;
    return duration<double, std::micro>(steady_clock::now().time_since_epoch()).count();
}

size_t row_stride(int dtype, uint32_t dim) { return (size_t)pimemb::row_stride_bytes(dtype, dim); }   // bytes from one row to the next
size_t index_size(emb_index_type t) { return t == EMB_IDX_I64 ? 8 : 4; }

struct Table {
    void *rows = nullptr;
    uint64_t nr_rows = 0;
    uint32_t dim = 0;
    int dtype = EMB_F32;            // (an emb_dtype value, held as int: pimemb_internal.h, dtype_value)
    LaunchGeom geom{};
    size_t bytes = 0;
    uint64_t generation = 0;  // bumped whenever `rows` is (re)allocated: prepared plans check it
    // optional hot-row set (emb_set_hot_rows): compact copy of the rows + row id -> slot hash, in HBM,
    // staged into LDS by bag_sum_hot_kernel
    void *hot_rows = nullptr;
    uint64_t *hot_hash = nullptr;
    uint32_t n_hot = 0, hot_log2 = 0;
    size_t hot_lds = 0;
};

// Launch images (descriptors + any uncached XCD map) of transient calls live in a ring of pinned,
// device-visible segments.  Calls bump-allocate inside the current segment; ONE event per segment
// (recorded when it fills up or the caller switches streams) tells when its images may be overwritten,
// so a call costs no event record of its own -- an event between two kernels of a stream also costs
// ~4 us of GPU time.
struct DescSlot {
    char *h = nullptr;
    char *d = nullptr;       // HBM twin (PIMEMB_DESC_MODE=copy only)
    size_t cap = 0;          // bytes
    size_t used = 0;
    hipStream_t stream = nullptr;   // stream of the launches whose images sit in this segment
    hipEvent_t done = nullptr;
    bool pending = false;
};
constexpr int kSlots = 4;
constexpr size_t kSlotBytes = 256u << 10;
constexpr int kRingPool = 8;
inline int ring_of_thread() {
    static const bool one = getenv("PIMEMB_RING_POOL") && atoi(getenv("PIMEMB_RING_POOL")) == 1;   // A/B: every thread on ring 0 = one lock, as in round 3
    return one ? 0 : (int)(std::hash<std::thread::id>()(std::this_thread::get_id()) % (size_t)kRingPool);
}
struct ImageRing {              // the engine has one (under its mutex); a request queue has its own (under the queue's lock)
    DescSlot slots[kSlots];
    int next_slot = 0;
    int desc_mode = 1;          // 1: kernels read descriptors from the pinned segment; 0: copied into HBM per call
    unsigned slot_flags = 0;    // hipHostMalloc flags of the segments
    void release() {
        for (DescSlot &sl : slots) {
            if (sl.h) (void)hipHostFree(sl.h);
            if (sl.d) (void)hipFree(sl.d);
            if (sl.done) (void)hipEventDestroy(sl.done);
            sl = DescSlot{};
        }
    }
};

// XCD-aware workgroup maps of transient (plan-less) launches, kept in HBM and found again by launch
// shape: the map depends on the tile counts and table sizes only, never on the buffers of a call.
struct XmapCacheEntry {
    std::vector<uint64_t> key;   // kernel kind, bags per tile, then (tiles, table bytes) per descriptor
    uint32_t *d_map = nullptr;
    uint32_t xgrid = 0;
    bool direct = false;
    uint64_t last_use = 0;
    size_t bytes = 0;
    // the streams whose launches have read this map (a handful at most: a caller's stream, a queue's): an evicted map may be
    // freed once an event recorded on each of them AT EVICTION has fired -- no device-wide wait
    hipStream_t streams[4] = {};
    uint32_t n_streams = 0;
    bool many_streams = false;   // more than four: only a device-wide wait can vouch for it
};
// an evicted map on its way out
struct XmapGrave {
    uint32_t *d_map = nullptr;
    size_t bytes = 0;
    hipEvent_t ev[4] = {};
    uint32_t n_ev = 0;
    bool needs_device_wait = false;
};
// 32 shapes in HBM; a shape earns its place on its SECOND sighting (the first one carries its map in the launch image), and an
// evicted map is freed later, never between two launches.  Round 5 found the old policy -- 8 entries, allocate + blocking copy on
// every miss, hipDeviceSynchronize + hipFree on every eviction -- to be a cliff for launches whose shapes do NOT recur: the routed
// sharded step of two ranks went from 76 to 129 us per step as soon as its pieces stopped cycling through 8 sizes, i.e. with any
// real index stream (profiles/r05/README.md "launch shapes that do not recur").
constexpr size_t kXmapCacheEntries = 32;
constexpr size_t kXmapSeenEntries = 256;       // hashes of shapes seen once (a ring: the oldest is forgotten)
constexpr size_t kXmapGraveBytes = 64u << 20;  // evicted maps not yet known to be unread: beyond this many bytes the oldest ones are waited for

}  // namespace

struct emb_engine {
    int device = 0;
    std::vector<Table> tables;
    std::mutex mu;       // guards tables, staging buffers, the launch-image ring and the map cache;
                         // emb_plan_launch does not take it
    std::mutex host_mu;  // serialises host-pointer calls (they share one staging buffer) -- held for the whole call
    pimemb::HostCopier copier;   // packs inputs / unpacks results of host-pointer calls (used under host_mu)
    hipEvent_t pipe_ev[4] = {};  // pipelined zero-copy calls: "tables of part k are done"
    hipStream_t host_s2 = nullptr;      // big host-pointer calls (under host_mu): the second half's copy-in + kernel run here, next to the first half's copy-out
    hipEvent_t split_ev[2] = {};
    // Launch images of transient calls: a small POOL of rings, each under its own lock, picked by the calling thread -- a
    // launch holds its ring's lock across image copy + enqueue, so threads of a serving process no longer queue up behind ONE
    // engine-wide mutex (round 3: launch_resolved held `mu`); `mu` is left with the tables, the map cache and the staging
    ImageRing ring[kRingPool];
    std::mutex ring_mu[kRingPool];
    std::vector<XmapCacheEntry> xmap_cache;
    uint64_t xmap_clock = 0;
    std::vector<uint64_t> xmap_seen;       // hashes of launch shapes sighted once
    size_t xmap_seen_at = 0;
    std::vector<XmapGrave> xmap_graveyard;
    size_t xmap_grave_bytes = 0;
    // staging for EMB_MEM_HOST calls
    char *h_stage = nullptr;
    size_t h_stage_cap = 0;
    char *d_stage = nullptr;
    size_t d_stage_cap = 0;
    // input validation (checked_launch, under mu): 16 bytes of HBM the validation kernels count in, and what the host
    // remembers of them -- tickets drawn and offending values found by all earlier calls, and a sequence number
    // A checked call takes SLOT seq % kValSlots of these: its own counters in HBM (which its validation kernel leaves zeroed) and
    // its own pinned verdict word.  Per-call counters (round 6; one running pair before) make a call's finding its own whatever
    // else is in flight, so a verdict need not be waited for inside the call (EMB_FLAG_DEFER_CHECK): it is read -- in order -- by
    // a later call, or by emb_check_report.
    static constexpr uint32_t kValSlots = 64;
    pimemb::ValidateCtl *d_val = nullptr;                           // [kValSlots]
    unsigned long long val_seq = 0;
    struct PendingVerdict {
        unsigned long long seq;
        hipStream_t stream;
        uint32_t n_groups;
        KernelKind kinds[8];
        bool launched;
    };
    std::deque<PendingVerdict> val_pending;                         // deferred verdicts not read yet, oldest first (under val_mu)
    bool defer_check = false;                                       // EMB_FLAG_DEFER_CHECK
    unsigned long long val_owed_bad = 0, val_owed_first = 0;        // findings of deferred calls read but not yet handed to a caller (under val_mu)
    std::mutex val_mu;          // checked calls take turns (their findings are read as deltas of one device counter); `mu` is
                                // held only while such a call enqueues, not while it waits for its result
    volatile unsigned long long *val_result = nullptr;   // [kValSlots] pinned, device-visible words the validation kernels report into (validate_word)
    volatile unsigned long long *host_done = nullptr;    // host-pointer calls (under host_mu): "the kernel of call host_seq is done"
    unsigned long long host_seq = 0;
    // stats
    std::atomic<uint64_t> n_lookup_calls{0}, n_kernel_launches{0}, n_bags{0}, n_indices{0};
    std::atomic<uint64_t> n_by_kind[5] = {};
    uint64_t table_bytes = 0;
    double us_copy_in_indices = 0, us_copy_in_lengths = 0, us_launch = 0, us_copy_out = 0,
           us_sync = 0;
    bool stage_timing = false;  // wait + clock after every stage of a host-pointer call
    bool check_inputs = false;  // EMB_FLAG_CHECK_INPUTS: emb_lookup / emb_lookup_batched validate before they launch
    std::atomic<uint32_t> live_plans{0};
    uint64_t next_generation = 1;
    // stage trace (host-pointer path)
    std::deque<emb_trace_event> trace;
    uint32_t trace_cap = 0;
    uint32_t host_call_id = 0;
    void record(uint32_t stage, double a, double b) {
        if (!trace_cap) return;
        if (trace.size() >= trace_cap) trace.pop_front();
        trace.push_back(emb_trace_event{stage, host_call_id, a, b});
    }
};

struct PlanGroup {
    DevDesc *d_descs = nullptr;
    uint32_t n = 0;
    uint32_t max_tiles = 0;
    int dtype = EMB_F32;            // (an emb_dtype value, held as int: pimemb_internal.h, dtype_value)
    LaunchGeom geom{};
    KernelKind kind = pimemb::KERNEL_WAVEBATCH;
    uint32_t *d_xmap = nullptr;      // XCD-aware workgroup map, or null (2-D grid)
    uint32_t xgrid = 0;
    bool xdirect = false;            // map expanded to one {descriptor, tile} entry per workgroup
    uint32_t hot_wgs = 0;            // KERNEL_HOT: persistent workgroups per descriptor
    uint32_t hot_lds = 0;            // KERNEL_HOT: dynamic LDS bytes (largest hot set of the group)
    uint32_t *cached_xmap = nullptr; // transient launches: map owned by the engine's cache (not in the image)
    bool ranged = false;             // descriptors serve a row range each (emb_lookup_ranged / emb_plan_create_ranged)
    uint32_t pool = 0;               // 0: plain sum (bag_sum_*); else 1 + EMB_POOL_* of a pooled launch (bag_pool_*)
    uint32_t n_weighted = 0, n_padding = 0;   // pooled launch: descriptors with per-sample weights / a padding_idx
    bool out_half = false;           // EMB_POOL_OUT_TABLE_DTYPE: pooled rows leave in the table's 2-byte dtype (half-output twins)
    bool strided = false;            // emb_lookup_strided: every descriptor carries its output's row stride (the bag_strided_* twins)
    size_t desc_off = 0, xmap_off = 0;  // byte offsets of this group's pieces in the launch image
    std::vector<uint32_t> xmap_words;
};

struct emb_plan {
    emb_engine *e = nullptr;
    emb_index_type itype = EMB_IDX_U32;
    std::vector<PlanGroup> groups;
    char *d_image = nullptr;  // descriptors + XCD maps in HBM
    uint64_t bytes = 0, n_bags = 0, n_indices = 0;
    uint64_t signature = 0;   // hash of what the launches ARE (kernel kind, grid, XCD map, per-descriptor counts) -- never of addresses
    std::vector<std::pair<uint32_t, uint64_t>> table_gens;  // (table id, generation) the plan was built on
};

namespace {

// Drop a table's hot-row set (caller holds e->mu; any launch that may read it must have finished).
void clear_hot(Table &t) {
    if (t.hot_rows) (void)hipFree(t.hot_rows);
    if (t.hot_hash) (void)hipFree(t.hot_hash);
    t.hot_rows = nullptr;
    t.hot_hash = nullptr;
    t.n_hot = t.hot_log2 = 0;
    t.hot_lds = 0;
}

struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) {
            switched = hipSetDevice(dev) == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

// User descriptors resolved against the engine's tables and split into launch groups that share
// (dtype, dim).
struct Resolved {
    std::vector<DevDesc> descs;       // grouped, contiguous per group
    std::vector<PlanGroup> groups;    // kernel kind, tile counts, XCD map; device pointers set by bind()
    uint64_t bytes = 0, n_bags = 0, n_indices = 0;
    std::vector<char> image;          // descriptors of every group, then each group's XCD map
    hipStream_t stream = nullptr;     // transient launches: the stream the launch goes to (the map cache notes who reads a map)

    // Lay descriptors and maps out in one host image; offsets go into the groups.
    void build_image() {
        size_t off = 0, di = 0;
        for (PlanGroup &g : groups) {
            g.desc_off = off;
            off += sizeof(DevDesc) * g.n;
        }
        for (PlanGroup &g : groups) {
            g.xmap_off = off;
            off += (g.xmap_words.size() * 4 + 63) / 64 * 64;
        }
        image.assign(off ? off : 64, 0);
        for (PlanGroup &g : groups) {
            memcpy(image.data() + g.desc_off, descs.data() + di, sizeof(DevDesc) * g.n);
            di += g.n;
            if (!g.xmap_words.empty())
                memcpy(image.data() + g.xmap_off, g.xmap_words.data(), g.xmap_words.size() * 4);
        }
    }
    void bind(char *d_base) {
        for (PlanGroup &g : groups) {
            g.d_descs = reinterpret_cast<DevDesc *>(d_base + g.desc_off);
            g.d_xmap = g.cached_xmap ? g.cached_xmap
                       : g.xmap_words.empty() ? nullptr : reinterpret_cast<uint32_t *>(d_base + g.xmap_off);
        }
    }
};

// Transient launches: find (or build, upload and remember) the XCD map of this launch shape.  On
// success the group points at the cached device copy and carries no map words of its own.
// Free the evicted maps whose launches are known to be over: every event recorded at their eviction has fired (a query, never a
// wait).  Round 5 kept up to 64 of them (up to 8 MB each, outside every HBM budget) and then called hipDeviceSynchronize under
// e->mu -- a stall for every launching thread, and illegal while another thread captures a stream.  wait_oldest: the graveyard
// is over its byte cap -- wait for the oldest entries' OWN events (or, for a map more than four streams have read, the device).
void reap_xmap_graveyard(emb_engine *e, bool wait_oldest) {
    size_t kept = 0;
    for (size_t i = 0; i < e->xmap_graveyard.size(); i++) {
        XmapGrave &gv = e->xmap_graveyard[i];
        const bool over = wait_oldest && e->xmap_grave_bytes > kXmapGraveBytes;
        bool done = !gv.needs_device_wait;
        if (gv.needs_device_wait && over) done = hipDeviceSynchronize() == hipSuccess;
        for (uint32_t k = 0; k < gv.n_ev && done; k++) {
            hipError_t q = over ? hipEventSynchronize(gv.ev[k]) : hipEventQuery(gv.ev[k]);
            if (q != hipSuccess) {
                (void)hipGetLastError();
                done = false;
            }
        }
        if (done) {
            for (uint32_t k = 0; k < gv.n_ev; k++) (void)hipEventDestroy(gv.ev[k]);
            (void)hipFree(gv.d_map);
            e->xmap_grave_bytes -= gv.bytes;
        } else {
            e->xmap_graveyard[kept++] = gv;
        }
    }
    e->xmap_graveyard.resize(kept);
}

int cached_xcd_map(emb_engine *e, PlanGroup &g, uint32_t bpt, const std::vector<uint32_t> &tiles_of,
                   const std::vector<uint64_t> &bytes_of, hipStream_t stream) {
    std::vector<uint64_t> key;
    key.reserve(2 + 2 * tiles_of.size());
    key.push_back((uint64_t)g.kind);
    key.push_back(bpt);
    for (size_t i = 0; i < tiles_of.size(); i++) {
        key.push_back(tiles_of[i]);
        key.push_back(bytes_of[i]);
    }
    static const bool cache_off = getenv("PIMEMB_XMAP_CACHE") && atoi(getenv("PIMEMB_XMAP_CACHE")) == 0;   // A/B: every map in the launch image
    if (cache_off) return EMB_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(e->mu);
    ++e->xmap_clock;                                   // (every transient launch with a map ages the entries)
    auto note_stream = [stream](XmapCacheEntry &c) {
        for (uint32_t k = 0; k < c.n_streams; k++)
            if (c.streams[k] == stream) return;
        if (c.n_streams < 4) c.streams[c.n_streams++] = stream;
        else c.many_streams = true;
    };
    for (XmapCacheEntry &c : e->xmap_cache)
        if (c.key == key) {
            c.last_use = e->xmap_clock;
            note_stream(c);
            g.cached_xmap = c.d_map;
            g.xgrid = c.xgrid;
            g.xdirect = c.direct;
            return EMB_OK;
        }
    // not cached.  First sighting of the shape: remember its hash and let the caller carry the map in the launch image (no
    // allocation, no copy engine, nothing to wait for) -- shapes that never come back cost their host-side build and nothing else.
    uint64_t h = 1469598103934665603ull;
    for (uint64_t v : key) h = (h ^ v) * 1099511628211ull;
    bool seen = false;
    for (uint64_t v : e->xmap_seen) seen = seen || v == h;
    if (!seen) {
        if (e->xmap_seen.size() < kXmapSeenEntries) e->xmap_seen.push_back(h);
        else e->xmap_seen[e->xmap_seen_at++ % kXmapSeenEntries] = h;
        return EMB_ERR_UNSUPPORTED;                // (any non-OK: resolve() builds the map inline)
    }
    // a full cache gives a place up only if its least recently used shape has been idle for a while: more shapes in rotation than
    // entries would otherwise evict each other in turn (48 shapes cycling through 32 entries: every launch a miss)
    size_t victim = 0;
    if (e->xmap_cache.size() >= kXmapCacheEntries) {
        for (size_t i = 1; i < e->xmap_cache.size(); i++)
            if (e->xmap_cache[i].last_use < e->xmap_cache[victim].last_use) victim = i;
        if (e->xmap_clock - e->xmap_cache[victim].last_use < 4 * kXmapCacheEntries) return EMB_ERR_UNSUPPORTED;
    }
    XmapCacheEntry n;
    std::vector<uint32_t> words;
    n.xgrid = pimemb::build_xcd_map(tiles_of, bytes_of, &words, 1);
    if (n.xgrid <= (1u << 20)) {
        std::vector<uint32_t> direct;
        pimemb::expand_xcd_map(words, n.xgrid, &direct);
        words.swap(direct);
        n.direct = true;
    }
    if (hipMalloc((void **)&n.d_map, words.size() * 4) != hipSuccess) return EMB_ERR_NOMEM;   // caller builds inline
    if (hipMemcpy(n.d_map, words.data(), words.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(n.d_map);
        return EMB_ERR_DEVICE;
    }
    if (e->xmap_cache.size() >= kXmapCacheEntries) {   // evict it: a launch in flight may still read its map, so it is only set aside here, freed later
        const XmapCacheEntry &v = e->xmap_cache[victim];
        XmapGrave gv;
        gv.d_map = v.d_map;
        gv.bytes = v.bytes;
        gv.needs_device_wait = v.many_streams;
        for (uint32_t k = 0; k < v.n_streams && !gv.needs_device_wait; k++) {     // behind the last launch that read it, on every stream that did
            hipEvent_t ev = nullptr;
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess && hipEventRecord(ev, v.streams[k]) == hipSuccess) {
                gv.ev[gv.n_ev++] = ev;
            } else {          // (the caller destroyed that stream: its launches are over or lost -- only the device can say)
                if (ev) (void)hipEventDestroy(ev);
                (void)hipGetLastError();
                gv.needs_device_wait = true;
            }
        }
        e->xmap_grave_bytes += gv.bytes;
        e->xmap_graveyard.push_back(gv);
        e->xmap_cache.erase(e->xmap_cache.begin() + (long)victim);
        reap_xmap_graveyard(e, /*wait_oldest=*/true);
    }
    n.key.swap(key);
    n.bytes = words.size() * 4;
    note_stream(n);
    n.last_use = e->xmap_clock;
    g.cached_xmap = n.d_map;
    g.xgrid = n.xgrid;
    g.xdirect = n.direct;
    e->xmap_cache.push_back(std::move(n));
    return EMB_OK;
}

// A pooling spec that asks for nothing but what emb_lookup_batched does.
bool is_plain_sum(const emb_pool_spec &ps) {
    return ps.mode == EMB_POOL_SUM && ps.per_sample_weights == nullptr && ps.flags == 0;
}
// ... or for nothing else but rows in the table's dtype: the half-output twins of emb_lookup_batched's kernels.
bool is_plain_sum_half_out(const emb_pool_spec &ps) {
    return ps.mode == EMB_POOL_SUM && ps.per_sample_weights == nullptr && ps.flags == EMB_POOL_OUT_TABLE_DTYPE;
}
bool wants_half_out(const emb_pool_spec *pools, uint32_t i) { return pools && (pools[i].flags & EMB_POOL_OUT_TABLE_DTYPE) != 0; }
// Bytes of descriptor u's pooled rows: fp32, or the table's 2-byte dtype for a half-output descriptor.
size_t out_elem_size(const emb_pool_spec *pools, uint32_t i) { return wants_half_out(pools, i) ? 2 : 4; }
// emb_lookup_strided: descriptor i's pooled rows lie out_stride[i] floats apart -- unless that says what a dense output says.
bool is_strided(const uint64_t *out_stride, uint32_t i, uint32_t dim) { return out_stride && out_stride[i] != 0 && out_stride[i] != dim; }

// st_indices / st_offsets / st_out: if non-null, per-descriptor device pointers that replace the
// caller's (the staged copies of a host-pointer call).
// row_lo: if non-null, a RANGED launch -- descriptor i serves only the bags whose row falls into
// [row_lo[i], row_lo[i] + the table's rows); one index per bag, the wave-batch kernels (EMB_RANGE_OPEN_END in row_lo[i]
// travels to the kernel as it is: ids beyond the end of the range pool to zero rows).
// served (ranged launches only): if non-null, served[i] (may be null) is a uint32 counter in HBM that descriptor i's
// launch adds the number of bags it served to.
// out_stride (emb_lookup_strided; DEVICE calls without row_lo only): if non-null, out_stride[i] floats lie between two bags'
// pooled rows of descriptor i; 0 or the table's dim is a dense descriptor like any other.
int resolve(emb_engine *e, const emb_lookup_desc *descs, uint32_t n_descs, emb_index_type itype,
            const std::vector<const void *> *st_indices, const std::vector<const void *> *st_offsets,
            const std::vector<float *> *st_out, Resolved *r, bool cache_maps = false, const uint64_t *row_lo = nullptr,
            uint32_t *const *served = nullptr, const emb_pool_spec *pools = nullptr,
            const std::vector<const float *> *st_weights = nullptr, const uint64_t *out_stride = nullptr) {
    if (itype != EMB_IDX_U32 && itype != EMB_IDX_I64) return fail(EMB_ERR_INVALID, "bad index type");
    // (dtype, dim, pooling kind, output width, strided): kind 0 = plain sum, width 0 = fp32, strided 0 = rows back to back, the
    // key every call without pooling specs and strides has
    std::map<std::tuple<int, uint32_t, uint32_t, uint32_t, uint32_t>, std::vector<uint32_t>> by_shape;
    for (uint32_t i = 0; i < n_descs; i++) {
        const emb_lookup_desc &u = descs[i];
        if (u.table_id >= e->tables.size() || e->tables[u.table_id].rows == nullptr)
            return fail(EMB_ERR_INVALID, "desc %u: table %u is not loaded", i, u.table_id);
        if (u.n_bags > 0 && u.pooled == nullptr) return fail(EMB_ERR_INVALID, "desc %u: pooled is NULL", i);
        if (u.n_indices > 0 && u.indices == nullptr)
            return fail(EMB_ERR_INVALID, "desc %u: indices is NULL", i);
        if (u.offsets == nullptr) {
            if (u.n_bags > 0 && u.fixed_pooling == 0)
                return fail(EMB_ERR_INVALID, "desc %u: offsets is NULL and fixed_pooling is 0", i);
            if ((uint64_t)u.fixed_pooling * u.n_bags != u.n_indices)
                return fail(EMB_ERR_INVALID, "desc %u: fixed_pooling*n_bags != n_indices", i);
        }
        const Table &t = e->tables[u.table_id];
        if (row_lo) {
            if (u.offsets != nullptr || u.fixed_pooling != 1)
                return fail(EMB_ERR_INVALID, "ranged lookup: desc %u: one index per bag only (offsets NULL, fixed_pooling 1)", i);
            if (t.geom.scalar_lanes)
                return fail(EMB_ERR_UNSUPPORTED, "ranged lookup: desc %u: rows must be 16-byte multiples up to 1 KiB", i);
            if (t.dtype == pimemb::kMXFP4)
                return fail(EMB_ERR_UNSUPPORTED, "ranged lookup: desc %u: table %u is MXFP4, which the lane-group kernels serve only "
                            "(no ranged, counted or typed lookup)", i, u.table_id);
        }
        uint32_t pool_kind = 0;
        if (pools && !is_plain_sum(pools[i])) {
            const emb_pool_spec &ps = pools[i];
            if (ps.mode > EMB_POOL_MAX || (ps.flags & ~(EMB_POOL_PADDING | EMB_POOL_OUT_TABLE_DTYPE)) != 0)
                return fail(EMB_ERR_INVALID, "desc %u: bad pooling spec (mode %u, flags 0x%x)", i, ps.mode, ps.flags);
            if ((ps.flags & EMB_POOL_OUT_TABLE_DTYPE) && t.dtype == pimemb::kMXFP4)
                return fail(EMB_ERR_UNSUPPORTED, "desc %u: EMB_POOL_OUT_TABLE_DTYPE: table %u is MXFP4, whose pooled rows are fp32 only", i, u.table_id);
            if ((ps.flags & EMB_POOL_OUT_TABLE_DTYPE) && t.dtype != EMB_F16 && t.dtype != EMB_BF16)
                return fail(EMB_ERR_UNSUPPORTED, "desc %u: EMB_POOL_OUT_TABLE_DTYPE needs an fp16 or bf16 table (table %u has dtype %d)", i,
                            u.table_id, (int)t.dtype);
            if (ps.per_sample_weights != nullptr && ps.mode != EMB_POOL_SUM)
                return fail(EMB_ERR_INVALID, "desc %u: per_sample_weights need EMB_POOL_SUM (as in torch)", i);
            if (t.dtype == EMB_FIXED32)
                return fail(EMB_ERR_UNSUPPORTED, "desc %u: fixed-point tables pool by plain sum only", i);
            if ((ps.flags & EMB_POOL_PADDING) && (ps.padding_idx < 0 || (uint64_t)ps.padding_idx >= t.nr_rows))
                return fail(EMB_ERR_INVALID, "desc %u: padding_idx %lld outside table %u (%llu rows)", i, (long long)ps.padding_idx,
                            u.table_id, (unsigned long long)t.nr_rows);
            if (row_lo) return fail(EMB_ERR_UNSUPPORTED, "ranged lookups pool by plain sum only");
            if (!is_plain_sum_half_out(ps)) pool_kind = 1u + ps.mode;      // (only the flag: the sum kernels' half-output twins)
        }
        const bool strided = is_strided(out_stride, i, t.dim);
        if (strided) {
            const uint64_t st = out_stride[i];
            if (t.geom.scalar_lanes)
                return fail(EMB_ERR_UNSUPPORTED, "desc %u: strided output needs rows of 16-byte multiples up to 1 KiB (table %u, dim %u, runs the "
                            "any-dim kernels, which have no strided twin)", i, u.table_id, t.dim);
            if (t.dtype == EMB_FIXED32)
                return fail(EMB_ERR_UNSUPPORTED, "desc %u: strided output: table %u is fixed-point, whose kernels have no strided twin", i, u.table_id);
            if (wants_half_out(pools, i))
                return fail(EMB_ERR_UNSUPPORTED, "desc %u: strided output is fp32 only: EMB_POOL_OUT_TABLE_DTYPE with a row stride has no kernel", i);
            if (st < t.dim || st % 4 != 0 || st > 0xffffffffull)
                return fail(EMB_ERR_INVALID, "desc %u: out_stride %llu: need dim (%u) <= stride <= 4294967295 and stride %% 4 == 0", i,
                            (unsigned long long)st, t.dim);
            if (((uintptr_t)u.pooled & 15u) != 0)
                return fail(EMB_ERR_INVALID, "desc %u: strided output: pooled (%p) must be 16-byte aligned", i, (void *)u.pooled);
        }
        by_shape[{(int)t.dtype, t.dim, pool_kind, wants_half_out(pools, i) ? 1u : 0u, strided ? 1u : 0u}].push_back(i);
    }
    const size_t isz = index_size(itype);
    for (auto &kv : by_shape) {
        PlanGroup g;
        g.dtype = std::get<0>(kv.first);
        g.pool = std::get<2>(kv.first);
        g.out_half = std::get<3>(kv.first) != 0;
        g.strided = std::get<4>(kv.first) != 0;
        g.n = (uint32_t)kv.second.size();
        const Table &t0 = e->tables[descs[kv.second[0]].table_id];
        g.geom = t0.geom;
        uint64_t group_bags = 0, group_idx = 0;
        for (uint32_t i : kv.second) {
            group_bags += descs[i].n_bags;
            group_idx += descs[i].n_indices;
        }
        g.kind = pimemb::choose_kernel(group_bags, group_idx, g.geom);
        {   // developer A/B (tools/kernel_choice_probe.py): PIMEMB_FORCE_KERNEL=group | wavebatch overrides the choice where both kernels apply
            static const char *force = getenv("PIMEMB_FORCE_KERNEL");
            if (force && g.kind != pimemb::KERNEL_ANYDIM && group_idx <= 2 * group_bags)
                g.kind = force[0] == 'g' ? pimemb::KERNEL_GROUP : pimemb::KERNEL_WAVEBATCH;
        }
        if (g.dtype == pimemb::kMXFP4) g.kind = pimemb::KERNEL_GROUP;      // (whatever the shape: MXFP4 has the lane-group kernels only)
        g.ranged = row_lo != nullptr;
        if (g.ranged && g.kind == pimemb::KERNEL_GROUP) g.kind = pimemb::KERNEL_WAVEBATCH;    // (small launches too: the predicate lives there)
        if (g.pool && g.kind == pimemb::KERNEL_WAVEBATCH2) g.kind = pimemb::KERNEL_WAVEBATCH;  // (the pooled family has one wave-batch geometry)
        if (g.kind == pimemb::KERNEL_GROUP && !g.pool && !g.out_half && !g.strided) {   // (a pooled, half-output or strided launch never takes the hot-row kernel)   // pooled launch over tables with a hot-row set: LDS-staged kernel
            for (uint32_t i : kv.second) {
                const Table &t = e->tables[descs[i].table_id];
                if (t.n_hot && t.hot_lds > g.hot_lds) g.hot_lds = (uint32_t)t.hot_lds;
            }
            if (g.hot_lds) g.kind = pimemb::KERNEL_HOT;
        }
        const uint32_t bpt = pimemb::bags_per_tile(g.kind, g.geom);
        std::vector<uint32_t> tiles_of;
        std::vector<uint64_t> bytes_of;
        for (uint32_t i : kv.second) {
            const emb_lookup_desc &u = descs[i];
            const Table &t = e->tables[u.table_id];
            uint64_t tiles = (u.n_bags + bpt - 1) / bpt;
            if (tiles > 0x0fffffffull) return fail(EMB_ERR_UNSUPPORTED, "desc %u: too many bags", i);
            DevDesc d{};
            d.weights = t.rows;
            d.indices = st_indices ? (*st_indices)[i] : u.indices;
            d.offsets = st_offsets ? (*st_offsets)[i] : u.offsets;
            d.out = st_out ? (*st_out)[i] : u.pooled;
            d.n_idx = u.n_indices;
            d.n_bags = u.n_bags;
            d.nr_rows = t.nr_rows;
            d.fixed_pooling = u.offsets ? 0u : u.fixed_pooling;
            d.n_tiles = (uint32_t)tiles;
            if (row_lo) d.ranged.row_lo = row_lo[i];
            if (row_lo && served) d.ranged.served = served[i];
            if (g.strided) d.words[pimemb::kOutStrideWord] = out_stride[i];      // (zero in every other descriptor: `DevDesc d{}`)
            if (g.pool) {           // the pooling spec rides in DevDesc::pool (pimemb_bag_kernels.h: pool_args)
                const emb_pool_spec &ps = pools[i];
                const bool weighted = ps.per_sample_weights != nullptr, padded = (ps.flags & EMB_POOL_PADDING) != 0;
                const uint32_t op = ps.mode == EMB_POOL_MAX ? pimemb::kPoolOpMax
                                    : !weighted          ? pimemb::kPoolOpAdd
                                    : padded             ? pimemb::kPoolOpMulAdd
                                                         : pimemb::kPoolOpFma;
                d.pool.weights = st_weights && weighted ? (*st_weights)[i] : ps.per_sample_weights;
                d.pool.padding_row = padded ? (uint64_t)ps.padding_idx : ~0ull;
                d.pool.op = op | (ps.mode == EMB_POOL_MEAN ? pimemb::kPoolMean : 0u);
                g.n_weighted += weighted;
                g.n_padding += padded;
                if (weighted) r->bytes += u.n_indices * 4;
            }
            if (g.kind == pimemb::KERNEL_HOT) {
                d.hot_rows = t.hot_rows;
                d.hot_hash = t.hot_hash;
                d.n_hot = t.n_hot;
                d.hot_log2 = t.hot_log2;
            }
            if (d.n_tiles > g.max_tiles) g.max_tiles = d.n_tiles;
            tiles_of.push_back(d.n_tiles);
            bytes_of.push_back(t.bytes);
            r->descs.push_back(d);
            r->n_bags += u.n_bags;
            r->n_indices += u.n_indices;
            // algorithmic bytes, SURVEY.md section 8 row D
            r->bytes += u.n_indices * ((uint64_t)row_stride(t.dtype, t.dim) + isz) +
                        (u.offsets ? u.n_bags * isz : 0) + u.n_bags * (uint64_t)t.dim * (g.out_half ? 2 : 4);
        }
        // several tables in one big one-hot launch: XCD-aware workgroup map (one table <-> one XCD's
        // L2).  Measured neutral for pooled launches and slightly negative for small ones, which
        // keep the plain 2-D grid.
        if (g.n > 1 && g.max_tiles > 0 &&
            (g.kind == pimemb::KERNEL_WAVEBATCH || g.kind == pimemb::KERNEL_WAVEBATCH2)) {
            // Plan-less launches: the map is built for tile counts rounded UP to 1/16 of their power of two (< 6.25 % more
            // workgroups; a workgroup whose tile lies beyond its descriptor's n_tiles leaves at once), so that launches whose sizes
            // wander by a few bags -- the pieces of a routed sharded step, a server's batches -- share a shape and with it a cached
            // map, instead of each paying ~8 us of host time for a map of its own (profiles/r05/xmap_cache_shapes.log).
            if (cache_maps)
                for (uint32_t &v : tiles_of)
                    if (v > 16) {
                        uint32_t q = 1;
                        while ((q << 1) <= v) q <<= 1;
                        q >>= 4;
                        v = (v + q - 1) / q * q;
                    }
            uint64_t total_tiles = 0;
            for (uint32_t t : tiles_of) total_tiles += t;
            if (total_tiles + 8 * (uint64_t)g.n > 0x7fffffffull)
                return fail(EMB_ERR_UNSUPPORTED, "launch too large for one grid");
            if (!cache_maps || cached_xcd_map(e, g, bpt, tiles_of, bytes_of, r->stream) != EMB_OK) {
                g.xgrid = pimemb::build_xcd_map(tiles_of, bytes_of, &g.xmap_words, 1);
                if (g.xgrid <= (1u << 20)) {   // <= 8 MB of map: one scalar load per workgroup instead of a search
                    std::vector<uint32_t> direct;
                    pimemb::expand_xcd_map(g.xmap_words, g.xgrid, &direct);
                    g.xmap_words.swap(direct);
                    g.xdirect = true;
                }
            }
        } else if (g.n > 65535u) {
            return fail(EMB_ERR_UNSUPPORTED, "more than 65535 descriptors of one shape");
        }
        if (g.kind == pimemb::KERNEL_HOT) {
            // ~8192 1024-thread workgroups per launch, each staging its table's hot set once and striding
            // over that table's tiles.  Swept on the 48-table C3 run (bench.py --workload c3 --hot-rows 100):
            // 512: 0.774 ms, 1024: 0.705, 2048: 0.674, 4096: 0.652, 8192: 0.642, 12288: 0.641, 16384: 0.701,
            // one workgroup per tile: 0.732; the plain lane-group kernel without hints: 0.671.
            static const uint32_t total = getenv("PIMEMB_HOT_WGS_TOTAL") ? (uint32_t)atoi(getenv("PIMEMB_HOT_WGS_TOTAL")) : 8192u;
            // ... and at least two tiles per workgroup, so staging is amortised (16 tables: 4096 in all, neutral)
            const uint32_t cap = g.max_tiles / 2u ? g.max_tiles / 2u : 1u;
            uint32_t w = total / g.n;
            g.hot_wgs = w < 1u ? 1u : (w > cap ? cap : w);
        }
        r->groups.push_back(std::move(g));
    }
    r->build_image();
    return EMB_OK;
}

int launch_groups(emb_engine *e, const std::vector<PlanGroup> &groups, emb_index_type itype,
                  hipStream_t s) {
    for (const PlanGroup &g : groups) {
        if (g.pool)
            HIP_TRY(pimemb::launch_bag_pool(g.d_descs, g.n, g.max_tiles, g.dtype, itype, g.geom, g.kind, g.d_xmap, g.xgrid,
                                            g.xdirect, s, g.out_half, g.strided));
        else if (g.kind == pimemb::KERNEL_HOT)
            HIP_TRY(pimemb::launch_bag_sum_hot(g.d_descs, g.n, g.hot_wgs, g.hot_lds, g.dtype, itype, g.geom, s));
        else
            HIP_TRY(pimemb::launch_bag_sum(g.d_descs, g.n, g.max_tiles, g.dtype, itype, g.geom, g.kind, g.d_xmap,
                                           g.xgrid, g.xdirect, s, g.ranged, g.out_half, g.strided));
        e->n_kernel_launches.fetch_add(1, std::memory_order_relaxed);
        e->n_by_kind[g.kind].fetch_add(1, std::memory_order_relaxed);
    }
    return EMB_OK;
}

// Space for an n-byte launch image on stream s: *h (host view) and *d (HBM twin or null).
int take_image_space(ImageRing &r, size_t n, hipStream_t s, char **h, char **d) {
    n = (n + 127) / 128 * 128;
    DescSlot *sl = &r.slots[r.next_slot];
    if (sl->used && (sl->used + n > sl->cap || sl->stream != s)) {   // close the segment, move on
        if (hipEventRecord(sl->done, sl->stream) == hipSuccess) {
            sl->pending = true;
            r.next_slot = (r.next_slot + 1) % kSlots;
            sl = &r.slots[r.next_slot];
        } else {                       // e.g. the caller destroyed that stream: drain everything instead
            (void)hipGetLastError();
            HIP_TRY(hipDeviceSynchronize());
            sl->used = 0;
        }
    }
    if (sl->pending) {
        HIP_TRY(hipEventSynchronize(sl->done));
        sl->pending = false;
        sl->used = 0;
    }
    if (sl->cap < n) {      // first use, or an image larger than a segment (huge uncached map)
        if (sl->used) {     // images of launches that may still be in flight
            HIP_TRY(hipDeviceSynchronize());
            sl->used = 0;
        }
        if (sl->h) (void)hipHostFree(sl->h);
        if (sl->d) (void)hipFree(sl->d);
        sl->h = nullptr;
        sl->d = nullptr;
        sl->cap = 0;
        const size_t cap = n < kSlotBytes ? kSlotBytes : n + n / 4;
        HIP_TRY(hipHostMalloc((void **)&sl->h, cap, r.slot_flags));
        if (r.desc_mode == 0) HIP_TRY(hipMalloc((void **)&sl->d, cap));
        sl->cap = cap;
    }
    if (!sl->done) HIP_TRY(hipEventCreateWithFlags(&sl->done, hipEventDisableTiming));
    *h = sl->h + sl->used;
    *d = sl->d ? sl->d + sl->used : nullptr;
    sl->used += n;
    sl->stream = s;
    return EMB_OK;
}

// PIMEMB_HOST_PROFILE=1: accumulate where a transient device-pointer call spends its host time
// (printed by emb_destroy).  Developer aid; one getenv per process.
struct HostProfile {
    bool on = getenv("PIMEMB_HOST_PROFILE") != nullptr;
    double resolve = 0, slot = 0, image = 0, h2d = 0, launch = 0;
    uint64_t calls = 0;
};
HostProfile g_prof;

// Transient launch over device-resident buffers described by `r`.
int launch_resolved(emb_engine *e, Resolved &r, emb_index_type itype, hipStream_t s,
                    bool descriptors_in_host_memory = false) {
    if (r.descs.empty()) return EMB_OK;
    const int rk = ring_of_thread();
    std::lock_guard<std::mutex> lk(e->ring_mu[rk]);
    const double p0 = g_prof.on ? now_us() : 0;
    char *h = nullptr, *d = nullptr;
    int rc = take_image_space(e->ring[rk], r.image.size(), s, &h, &d);
    if (rc) return rc;
    const double p1 = g_prof.on ? now_us() : 0;
    memcpy(h, r.image.data(), r.image.size());
    const double p2 = g_prof.on ? now_us() : 0;
    if (d == nullptr || descriptors_in_host_memory) {
        r.bind(h);         // the kernel's scalar loads read the pinned, device-visible segment itself
    } else {
        HIP_TRY(hipMemcpyAsync(d, h, r.image.size(), hipMemcpyHostToDevice, s));
        r.bind(d);
    }
    const double p3 = g_prof.on ? now_us() : 0;
    rc = launch_groups(e, r.groups, itype, s);
    if (rc) return rc;
    if (g_prof.on) {
        g_prof.slot += p1 - p0; g_prof.image += p2 - p1; g_prof.h2d += p3 - p2; g_prof.launch += now_us() - p3;
        g_prof.calls++;
    }
    return EMB_OK;
}

int ensure_stage(emb_engine *e, size_t h_bytes, size_t d_bytes) {
    if (e->h_stage_cap < h_bytes) {
        if (e->h_stage) (void)hipHostFree(e->h_stage);
        e->h_stage = nullptr;
        e->h_stage_cap = 0;
        size_t cap = h_bytes + h_bytes / 4 + 4096;
        HIP_TRY(hipHostMalloc((void **)&e->h_stage, cap, hipHostMallocMapped | hipHostMallocCoherent));
        e->h_stage_cap = cap;
    }
    if (e->d_stage_cap < d_bytes) {
        if (e->d_stage) (void)hipFree(e->d_stage);
        e->d_stage = nullptr;
        e->d_stage_cap = 0;
        size_t cap = d_bytes + d_bytes / 4 + 4096;
        HIP_TRY(hipMalloc((void **)&e->d_stage, cap));
        e->d_stage_cap = cap;
        // a staging buffer that big belongs to calls that may go out in two parts (lookup_host_split): their second stream and
        // events are made here, next to an allocation, not inside a call that is being timed (a stream costs milliseconds the first time)
        if (cap >= (8u << 20) && !e->host_s2) {
            HIP_TRY(hipStreamCreateWithFlags(&e->host_s2, hipStreamNonBlocking));
            for (hipEvent_t &ev : e->split_ev)
                if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            // ... and used once: the runtime builds a stream's hardware queue at its first launch (8-9 ms, seen as the one slow
            // call of a loop of lookup()s)
            HIP_TRY(pimemb::launch_zero_words(reinterpret_cast<uint32_t *>(e->d_stage), 1, e->host_s2));
            HIP_TRY(hipStreamSynchronize(e->host_s2));
        }
    }
    return EMB_OK;
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Host-pointer path: pack indices+offsets into pinned staging, one H2D, kernel(s), D2H per table.
// Synchronous, like the reference's lookup (emb_host.h:350 dpu_sync before return).
struct HostStage {
    std::vector<const void *> d_indices, d_offsets;
    std::vector<const float *> d_weights;   // pooled calls: staged per-sample weights (nullptr: none)
    std::vector<float *> d_out;
    size_t in_bytes = 0, out_bytes = 0;
    char *h_out = nullptr;  // pinned landing zone for small results (null if not reserved)
    bool zero_copy = false; // the kernel reads/writes the pinned host staging itself (no copies)
    bool h2d_deferred = false;   // big call with link-speed output pieces: the caller enqueues the copy-in itself, in two parts (lookup_host_split)
};

// Host-pointer calls up to 40 MB skip both copy-engine transfers: the pinned staging buffer is
// device-visible, so the kernel gathers its indices from host memory and stores the pooled rows
// straight back over PCIe; the host then unpacks them into the caller's buffers (a few threads, and
// for >= 4 MB overlapped with the kernel in up to four parts, lookup_host_pipelined).  Measured with
// emb_host_bench (26 tables x 16 columns, one index per bag, ms per lookup(); zero-copy as shipped vs
// copy-engine transfers): 512 bags 0.053 / 0.082, 2048 bags 0.15 / 0.43-0.51, 8192 bags 0.40 / 0.92,
// 16384 bags 0.80 / 1.70, 20000 bags 0.92 / 2.0.  The exception: when every table returns >= 1.5e6
// bytes the runtime's device-to-host copies into pageable memory run at link speed and are used
// instead (24000 bags: 1.19 ms either way, 39292 bags: 1.75 vs 1.92 zero-copy); smaller pieces take a
// slow staged path in the runtime (17 us + ~16 GB/s per copy).  Both limits can be overridden with
// PIMEMB_ZERO_COPY_BYTES / PIMEMB_FAST_PIECE_BYTES (tools/emb_host_bench.cpp is the probe).
static const size_t kZeroCopyBytes = getenv("PIMEMB_ZERO_COPY_BYTES") ? strtoull(getenv("PIMEMB_ZERO_COPY_BYTES"), nullptr, 10) : (40u << 20);
static const size_t kStagedOutBytes = kZeroCopyBytes > (1u << 20) ? kZeroCopyBytes : (1u << 20);
static const size_t kFastPieceBytes = getenv("PIMEMB_FAST_PIECE_BYTES") ? strtoull(getenv("PIMEMB_FAST_PIECE_BYTES"), nullptr, 10) : 1500000;   // measured boundary: 1.28 MB pieces slow, 1.536 MB pieces fast

static const size_t kSplitInBytes = getenv("PIMEMB_HOST_SPLIT_BYTES") ? strtoull(getenv("PIMEMB_HOST_SPLIT_BYTES"), nullptr, 10) : (1u << 20);

int stage_host_inputs(emb_engine *e, const emb_lookup_desc *descs, uint32_t n, emb_index_type itype,
                      hipStream_t s, HostStage *hs, bool with_outputs, bool allow_zero_copy = false, bool allow_split = false,
                      const emb_pool_spec *pools = nullptr) {
    const size_t isz = index_size(itype);
    size_t in_bytes = 0, out_bytes = 0, min_piece = SIZE_MAX;
    for (uint32_t i = 0; i < n; i++) {
        if (descs[i].table_id >= e->tables.size() || !e->tables[descs[i].table_id].rows)
            return fail(EMB_ERR_INVALID, "desc %u: table %u is not loaded", i, descs[i].table_id);
        in_bytes += align_up(descs[i].n_indices * isz, 16);
        if (descs[i].offsets) in_bytes += align_up(descs[i].n_bags * isz, 16);
        if (pools && pools[i].per_sample_weights) in_bytes += align_up(descs[i].n_indices * 4, 16);
        const size_t piece = descs[i].n_bags * (size_t)e->tables[descs[i].table_id].dim * out_elem_size(pools, i);
        out_bytes += align_up(piece, 16);
        if (piece && piece < min_piece) min_piece = piece;
    }
    const bool fast_pieces = min_piece != SIZE_MAX && min_piece >= kFastPieceBytes;   // copies run at link speed
    if (!with_outputs) out_bytes = 0;
    const size_t h_out_bytes = (out_bytes <= kStagedOutBytes && !fast_pieces) ? out_bytes : 0;
    int rc = ensure_stage(e, in_bytes + h_out_bytes, in_bytes + out_bytes);
    if (rc) return rc;
    hs->h_out = h_out_bytes ? e->h_stage + in_bytes : nullptr;
    hs->zero_copy = allow_zero_copy && with_outputs && h_out_bytes == out_bytes && !fast_pieces &&
                    in_bytes + out_bytes <= kZeroCopyBytes;
    char *in_base = hs->zero_copy ? e->h_stage : e->d_stage;   // what the kernel will read
    size_t off = 0;
    hs->d_indices.resize(n);
    hs->d_offsets.resize(n);
    hs->d_weights.assign(n, nullptr);
    hs->d_out.resize(n);
    std::vector<pimemb::CopyPiece> pack;
    pack.reserve(3 * n);
    for (uint32_t i = 0; i < n; i++) {
        const emb_lookup_desc &u = descs[i];
        if (u.n_indices && !u.indices) return fail(EMB_ERR_INVALID, "desc %u: indices is NULL", i);
        pack.push_back({e->h_stage + off, u.indices, u.n_indices * isz});
        hs->d_indices[i] = in_base + off;
        off += align_up(u.n_indices * isz, 16);
        if (u.offsets) {
            pack.push_back({e->h_stage + off, u.offsets, u.n_bags * isz});
            hs->d_offsets[i] = in_base + off;
            off += align_up(u.n_bags * isz, 16);
        } else {
            hs->d_offsets[i] = nullptr;
        }
        if (pools && pools[i].per_sample_weights) {    // weights travel with the indices
            pack.push_back({e->h_stage + off, pools[i].per_sample_weights, u.n_indices * 4});
            hs->d_weights[i] = reinterpret_cast<const float *>(in_base + off);
            off += align_up(u.n_indices * 4, 16);
        }
    }
    e->copier.copy(pack);
    size_t oo = in_bytes;
    for (uint32_t i = 0; i < n; i++) {
        hs->d_out[i] = reinterpret_cast<float *>((hs->zero_copy ? e->h_stage : e->d_stage) + oo);
        if (with_outputs)
            oo += align_up(descs[i].n_bags * (size_t)e->tables[descs[i].table_id].dim * out_elem_size(pools, i), 16);
    }
    hs->in_bytes = in_bytes;
    hs->out_bytes = out_bytes;
    hs->h2d_deferred = allow_split && !hs->zero_copy && with_outputs && fast_pieces && n >= 2 && in_bytes >= kSplitInBytes;
    if (in_bytes && !hs->zero_copy && !hs->h2d_deferred)
        HIP_TRY(hipMemcpyAsync(e->d_stage, e->h_stage, in_bytes, hipMemcpyHostToDevice, s));
    return EMB_OK;
}

// Mid-size zero-copy calls: the kernel's stores into pinned host memory are PCIe-bound and the
// host-side unpack into the caller's buffers takes about as long.  Split the tables into up to four
// parts of similar output size, launch them back to back, and unpack part k (a few host threads)
// while the kernel of part k+1 is still storing: 26 tables x 16 columns, 16384 bags: 0.96 -> 0.80 ms,
// 8192 bags: 0.53 -> 0.40 ms.
constexpr size_t kPipelineBytes = 4u << 20;

int lookup_host_pipelined(emb_engine *e, const emb_lookup_desc *descs, uint32_t n, emb_index_type itype,
                          hipStream_t s, const HostStage &hs, double t0) {
    auto piece = [&](uint32_t i) { return descs[i].n_bags * (size_t)e->tables[descs[i].table_id].dim * 4; };
    const uint32_t parts = n < 4 ? n : 4;
    uint32_t bounds[5] = {0, 0, 0, 0, 0};
    {   // contiguous parts of ~equal output bytes
        size_t acc = 0;
        uint32_t k = 1;
        for (uint32_t i = 0; i < n && k < parts; i++) {
            acc += piece(i);
            if (acc * parts >= hs.out_bytes * k && n - (i + 1) >= parts - k) bounds[k++] = i + 1;
        }
        for (; k < parts; k++) bounds[k] = bounds[k - 1] + 1;   // (degenerate size distributions)
        bounds[parts] = n;
    }
    uint64_t bags = 0, idx = 0;
    for (uint32_t k = 0; k < parts; k++) {
        const uint32_t lo = bounds[k], cnt = bounds[k + 1] - lo;
        std::vector<const void *> di(hs.d_indices.begin() + lo, hs.d_indices.begin() + lo + cnt);
        std::vector<const void *> dof(hs.d_offsets.begin() + lo, hs.d_offsets.begin() + lo + cnt);
        std::vector<float *> dout(hs.d_out.begin() + lo, hs.d_out.begin() + lo + cnt);
        Resolved r;
        r.stream = s;
        int rc = resolve(e, descs + lo, cnt, itype, &di, &dof, &dout, &r, /*cache_maps=*/true);
        if (rc == EMB_OK) rc = launch_resolved(e, r, itype, s, true);
        if (rc) {
            (void)hipStreamSynchronize(s);   // parts already launched write into the staging buffer
            return rc;
        }
        if (!e->pipe_ev[k]) HIP_TRY(hipEventCreateWithFlags(&e->pipe_ev[k], hipEventDisableTiming));
        HIP_TRY(hipEventRecord(e->pipe_ev[k], s));
        bags += r.n_bags;
        idx += r.n_indices;
    }
    std::vector<pimemb::CopyPiece> unpack;
    for (uint32_t k = 0; k < parts; k++) {
        HIP_TRY(hipEventSynchronize(e->pipe_ev[k]));
        unpack.clear();
        for (uint32_t i = bounds[k]; i < bounds[k + 1]; i++)
            if (piece(i)) unpack.push_back({descs[i].pooled, hs.d_out[i], piece(i)});
        e->copier.copy(unpack);
    }
    e->us_sync += now_us() - t0;
    e->n_bags.fetch_add(bags, std::memory_order_relaxed);
    e->n_indices.fetch_add(idx, std::memory_order_relaxed);
    return EMB_OK;
}

// Big host-pointer calls whose rows go back table by table at link speed (every table >= 1.5 MB of rows: the Criteo shape at
// 39 292 bags is 8 MB of indices in, 65 MB of rows out): copy-in, kernel and copy-out in one chain leave the link idle in one
// direction at a time -- 0.24 ms in, then 1.42 ms out.  Two parts instead: a first part (about an eighth of the Criteo shape: the cut
// is estimated from the link's rates) goes in and is looked up on the caller's stream; the REST goes in and is looked up on a second stream while the first part's rows are
// already on their way out (PCIe is full duplex, the two directions have copy engines of their own); the caller's stream waits
// for the second kernel before it copies that part's rows out.  Everything is enqueued before the first device-to-host copy
// (those block the host while they run).  emb_host_bench 26 16 1000000 39292 1: 1.77 -> 1.59-1.63 ms per lookup(); 65 536 bags:
// 2.77 -> 2.56 ms.  PIMEMB_HOST_SPLIT_BYTES: the least input bytes for which a call is split (A/B).
int lookup_host_split(emb_engine *e, const emb_lookup_desc *descs, uint32_t n, emb_index_type itype, hipStream_t s, const HostStage &hs, double t0) {
    if (!e->host_s2) HIP_TRY(hipStreamCreateWithFlags(&e->host_s2, hipStreamNonBlocking));
    for (hipEvent_t &ev : e->split_ev)
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    const char *in_base = e->d_stage;
    auto in_off = [&](uint32_t i) { return i < n ? (size_t)(static_cast<const char *>(hs.d_indices[i]) - in_base) : hs.in_bytes; };
    // where to cut: the first part's input goes in alone (nothing to overlap it with), then the second part's input and kernel
    // run next to the first part's rows going out, then the second part's rows.  Estimated with the link's measured rates
    // (profiles/r06/link_probe.log: 53 GB/s in, 46 GB/s out in table-sized copies) and the cut that minimises the sum is taken.
    auto out_bytes_of = [&](uint32_t i) { return descs[i].n_bags * (double)e->tables[descs[i].table_id].dim * 4.0; };
    uint32_t m = 1;
    {
        double best = 1e300, out_a = 0;
        for (uint32_t c = 1; c < n; c++) {
            out_a += out_bytes_of(c - 1);
            const double in_a = (double)in_off(c), in_b = (double)hs.in_bytes - in_a, out_b = (double)hs.out_bytes - out_a;
            const double second_ready = in_b / 53e3 + 30.0, first_out = out_a / 46e3;              // microseconds
            const double total = in_a / 53e3 + 20.0 + (first_out > second_ready ? first_out : second_ready) + out_b / 46e3;
            if (total < best) {
                best = total;
                m = c;
            }
        }
    }
    const uint32_t bounds[3] = {0, m, n};
    hipStream_t on[2] = {s, e->host_s2};
    HIP_TRY(hipEventRecord(e->split_ev[0], s));                       // whatever the caller queued on its stream comes first
    HIP_TRY(hipStreamWaitEvent(e->host_s2, e->split_ev[0], 0));       // (nothing of this call is enqueued yet: a failure here leaves nothing behind)
    uint64_t bags = 0, idx = 0;
    for (uint32_t k = 0; k < 2; k++) {
        const uint32_t lo = bounds[k], cnt = bounds[k + 1] - lo;
        const size_t b0 = in_off(lo), b1 = in_off(bounds[k + 1]);
        int rc = EMB_OK;
        if (b1 > b0 && hipMemcpyAsync(e->d_stage + b0, e->h_stage + b0, b1 - b0, hipMemcpyHostToDevice, on[k]) != hipSuccess)
            rc = fail(EMB_ERR_DEVICE, "host-pointer call: copy-in of part %u failed: %s", k, hipGetErrorString(hipGetLastError()));
        std::vector<const void *> di(hs.d_indices.begin() + lo, hs.d_indices.begin() + lo + cnt);
        std::vector<const void *> dof(hs.d_offsets.begin() + lo, hs.d_offsets.begin() + lo + cnt);
        std::vector<float *> dout(hs.d_out.begin() + lo, hs.d_out.begin() + lo + cnt);
        Resolved r;
        r.stream = on[k];
        if (rc == EMB_OK) rc = resolve(e, descs + lo, cnt, itype, &di, &dof, &dout, &r, /*cache_maps=*/true);
        if (rc == EMB_OK) rc = launch_resolved(e, r, itype, on[k], false);
        if (rc) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamSynchronize(e->host_s2);
            return rc;
        }
        bags += r.n_bags;
        idx += r.n_indices;
    }
    hipError_t err = hipEventRecord(e->split_ev[1], e->host_s2);
    for (uint32_t k = 0; k < 2 && err == hipSuccess; k++) {
        if (k == 1) err = hipStreamWaitEvent(s, e->split_ev[1], 0);
        for (uint32_t i = bounds[k]; i < bounds[k + 1] && err == hipSuccess; i++) {
            const size_t bytes = descs[i].n_bags * (size_t)e->tables[descs[i].table_id].dim * 4;
            if (bytes) err = hipMemcpyAsync(descs[i].pooled, hs.d_out[i], bytes, hipMemcpyDeviceToHost, s);
        }
    }
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) {          // nothing of this call may still be running when the staging buffers are handed to the next one
        (void)hipStreamSynchronize(e->host_s2);
        (void)hipStreamSynchronize(s);
        return fail(EMB_ERR_DEVICE, "host-pointer call (two parts): %s", hipGetErrorString(err));
    }
    e->us_sync += now_us() - t0;
    e->n_bags.fetch_add(bags, std::memory_order_relaxed);
    e->n_indices.fetch_add(idx, std::memory_order_relaxed);
    return EMB_OK;
}

// Host-pointer lookup.  Default: ONE enqueue chain (copy-in -> descriptor upload -> kernel ->
// copy-out) and ONE wait at the end -- the lowest latency.  With stage timing on (emb_config.flags
// & EMB_FLAG_STAGE_TIMING, emb_trace_enable, or lookup(latency_print=1)) the host waits after every
// stage and clocks it, like the reference's six TIME_NOW brackets (emb_host.h:253-355); that costs
// ~2 extra stream waits per call.  (HIP events between the stages were measured too: they push the
// small copies onto a slower path, +30 us per call on the reference's presets.)
int lookup_host(emb_engine *e, const emb_lookup_desc *descs, uint32_t n, emb_index_type itype,
                hipStream_t s, const emb_pool_spec *pools = nullptr) {
    std::lock_guard<std::mutex> host_lk(e->host_mu);
    const bool timed = e->stage_timing || e->trace_cap != 0;
    HostStage hs;
    const double t0 = now_us();
    {
        std::lock_guard<std::mutex> lk(e->mu);
        // (pooled calls: one part, one stream)
        int rc = stage_host_inputs(e, descs, n, itype, s, &hs, true, /*allow_zero_copy=*/true, /*allow_split=*/!timed && !pools, pools);
        if (rc) return rc;
    }
    if (hs.h2d_deferred) return lookup_host_split(e, descs, n, itype, s, hs, t0);
    if (timed) HIP_TRY(hipStreamSynchronize(s));
    const double t1 = now_us();
    if (hs.zero_copy && !timed && hs.out_bytes >= kPipelineBytes && n >= 2 && !pools)
        return lookup_host_pipelined(e, descs, n, itype, s, hs, t0);
    Resolved r;
    r.stream = s;
    int rc = resolve(e, descs, n, itype, &hs.d_indices, &hs.d_offsets, &hs.d_out, &r, /*cache_maps=*/true, nullptr, nullptr,
                     pools, &hs.d_weights);
    if (rc) return rc;
    // descriptor upload ("query copying" in the reference's stage list) + the fused launch
    rc = launch_resolved(e, r, itype, s, hs.zero_copy);
    if (rc) return rc;
    const double t2 = now_us();
    if (timed) HIP_TRY(hipStreamSynchronize(s));
    const double t3 = now_us();
    // Small results (the reference's presets: tens of KB per table): ONE device-to-host copy of the
    // whole output region into pinned staging, then host memcpys -- a per-table hipMemcpy costs
    // ~12 us each.  Large results go straight to the caller's buffers, table by table.
    const bool staged_out = hs.out_bytes > 0 && hs.out_bytes <= kStagedOutBytes && hs.h_out != nullptr;
    if (hs.zero_copy) {
        // nothing to copy: the kernel already wrote hs.h_out
    } else if (staged_out) {
        HIP_TRY(hipMemcpyAsync(hs.h_out, hs.d_out[0], hs.out_bytes, hipMemcpyDeviceToHost, s));
    } else {
        for (uint32_t i = 0; i < n; i++) {
            size_t bytes = descs[i].n_bags * (size_t)e->tables[descs[i].table_id].dim * out_elem_size(pools, i);
            if (bytes)
                HIP_TRY(hipMemcpyAsync(descs[i].pooled, hs.d_out[i], bytes, hipMemcpyDeviceToHost, s));
        }
    }
    const double t4 = now_us();
    if (hs.zero_copy && !timed) {
        // a small zero-copy call: the rows land in pinned memory by the kernel's own stores, so all the host needs to know is
        // "the kernel is done" -- a one-thread kernel behind it stores a sequence number into a pinned word and the host
        // polls it (hipStreamSynchronize wakes several microseconds late for a launch this short)
        if (!e->host_done) {
            void *p = nullptr;
            HIP_TRY(hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent));
            e->host_done = static_cast<volatile unsigned long long *>(p);
            *e->host_done = 0;
        }
        const unsigned long long seq = ++e->host_seq;
        HIP_TRY(pimemb::launch_store_word(e->host_done, seq, s));
        bool done = false;
        for (int spin = 0; spin < 400000 && !(done = *e->host_done == seq); spin++) {
        }
        if (!done) HIP_TRY(hipStreamSynchronize(s));
    } else {
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (staged_out) {
        std::vector<pimemb::CopyPiece> unpack;
        unpack.reserve(n);
        for (uint32_t i = 0; i < n; i++) {
            size_t bytes = descs[i].n_bags * (size_t)e->tables[descs[i].table_id].dim * out_elem_size(pools, i);
            if (bytes)
                unpack.push_back({descs[i].pooled, hs.h_out + (reinterpret_cast<char *>(hs.d_out[i]) -
                                                                reinterpret_cast<char *>(hs.d_out[0])), bytes});
        }
        e->copier.copy(unpack);
    }
    const double t5 = now_us();
    if (timed) {
        e->us_copy_in_indices += t1 - t0;
        e->us_copy_in_lengths += t2 - t1;
        e->us_launch += t3 - t2;
        e->us_copy_out += t4 - t3;
        e->us_sync += t5 - t4;
        if (e->trace_cap) {
            std::lock_guard<std::mutex> lk(e->mu);
            e->record(EMB_STAGE_COPY_IN, t0, t1);
            e->record(EMB_STAGE_DESCRIPTORS, t1, t2);
            e->record(EMB_STAGE_LAUNCH, t2, t3);
            e->record(EMB_STAGE_COPY_OUT, t3, t4);
            e->record(EMB_STAGE_SYNC, t4, t5);
            e->host_call_id++;
        }
    } else {
        e->us_sync += t5 - t0;   // the whole call: stages are not separated in this mode
    }
    e->n_bags.fetch_add(r.n_bags, std::memory_order_relaxed);
    e->n_indices.fetch_add(r.n_indices, std::memory_order_relaxed);
    return EMB_OK;
}

}  // namespace

int pimemb::fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// =================================================================================================
extern "C" {

const char *emb_last_error(void) { return g_last_error.c_str(); }

const char *emb_version(void) { return "pimemb 0.1 gfx950"; }

int emb_create(const emb_config *cfg, emb_engine **out) {
    if (!out) return fail(EMB_ERR_INVALID, "emb_create: out is NULL");
    *out = nullptr;
    int dev = cfg ? cfg->device : -1;
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (count <= 0) return fail(EMB_ERR_DEVICE, "emb_create: no HIP device visible");
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    if (dev >= count) return fail(EMB_ERR_INVALID, "emb_create: device %d of %d", dev, count);
    emb_engine *e = new (std::nothrow) emb_engine();
    if (!e) return fail(EMB_ERR_NOMEM, "emb_create: out of host memory");
    e->device = dev;
    e->stage_timing = cfg && (cfg->flags & EMB_FLAG_STAGE_TIMING);
    e->check_inputs = cfg && (cfg->flags & EMB_FLAG_CHECK_INPUTS);
    e->defer_check = cfg && (cfg->flags & EMB_FLAG_DEFER_CHECK);
    {   // transient launches read their descriptors straight from the pinned segment (measured with
        // tools/transient_probe.py: 20.6 vs 22.4 us per C2-shaped call, 5.6 vs 8.7 us at 2048 bags per
        // table); PIMEMB_DESC_MODE=copy stages them into HBM with an in-stream copy instead
        const char *m = getenv("PIMEMB_DESC_MODE");
        for (ImageRing &rg : e->ring) {
            rg.desc_mode = (m && m[0] == 'c') ? 0 : 1;
            rg.slot_flags = hipHostMallocMapped | hipHostMallocCoherent;
        }
    }
    uint32_t max_tables = (cfg && cfg->max_tables) ? cfg->max_tables : 1024;
    e->tables.resize(max_tables);
    *out = e;
    return EMB_OK;
}

static int read_verdicts(emb_engine *e, bool wait, unsigned long long own_seq = 0, unsigned long long *own_bad = nullptr);

int emb_destroy(emb_engine *e) {
    if (!e) return EMB_OK;
    if (e->live_plans.load() != 0)
        return fail(EMB_ERR_INVALID, "emb_destroy: %u prepared plan(s) still reference this engine; destroy them first",
                    e->live_plans.load());
    DeviceGuard g(e->device);
    (void)hipDeviceSynchronize();
    {       // a deferred verdict nobody read is never lost silently
        std::lock_guard<std::mutex> vlk(e->val_mu);
        if (!e->val_pending.empty()) (void)read_verdicts(e, true);
        if (e->val_owed_bad)
            fprintf(stderr, "[pimemb] emb_destroy: an unread verdict: %llu out-of-range indices / broken offsets in checked call number %llu\n",
                    e->val_owed_bad, e->val_owed_first);
    }
    if (g_prof.on && g_prof.calls) {
        const double n = (double)g_prof.calls;
        fprintf(stderr, "[pimemb host profile] %llu transient calls, us/call: resolve %.2f  slot %.2f  image memcpy %.2f  "
                        "h2d enqueue %.2f  kernel enqueue %.2f\n", (unsigned long long)g_prof.calls,
                g_prof.resolve / n, g_prof.slot / n, g_prof.image / n, g_prof.h2d / n, g_prof.launch / n);
    }
    for (Table &t : e->tables) {
        clear_hot(t);
        if (t.rows) (void)hipFree(t.rows);
    }
    for (ImageRing &rg : e->ring) rg.release();
    for (XmapCacheEntry &c : e->xmap_cache) (void)hipFree(c.d_map);
    for (XmapGrave &gv : e->xmap_graveyard) {          // (emb_destroy has waited for the device)
        for (uint32_t k = 0; k < gv.n_ev; k++) (void)hipEventDestroy(gv.ev[k]);
        (void)hipFree(gv.d_map);
    }
    for (hipEvent_t ev : e->pipe_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->split_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (e->host_s2) (void)hipStreamDestroy(e->host_s2);
    if (e->h_stage) (void)hipHostFree(e->h_stage);
    if (e->d_stage) (void)hipFree(e->d_stage);
    if (e->d_val) (void)hipFree(e->d_val);
    if (e->val_result) (void)hipHostFree(const_cast<unsigned long long *>(e->val_result));
    if (e->host_done) (void)hipHostFree(const_cast<unsigned long long *>(e->host_done));
    delete e;
    return EMB_OK;
}

static int alloc_table(emb_engine *e, uint32_t table_id, uint64_t nr_rows, uint32_t dim, int dtype,
                       bool zero_fill) {
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    if (table_id >= e->tables.size())
        return fail(EMB_ERR_INVALID, "table id %u >= max_tables %zu", table_id, e->tables.size());
    if (nr_rows == 0) return fail(EMB_ERR_INVALID, "table %u: nr_rows is 0", table_id);
    LaunchGeom geom;
    int rc = pimemb::geometry_for(dtype, dim, &geom);
    if (dtype == pimemb::kMXFP4 && rc == EMB_ERR_INVALID)
        return fail(rc, "table %u: MXFP4 rows are blocks of 32 elements: dim %u is no multiple of 32", table_id, dim);
    if (dtype == pimemb::kMXFP4 && rc == EMB_ERR_UNSUPPORTED)
        return fail(rc, "table %u: MXFP4 tables take dim 32 .. 2048 (64 lanes per row), not %u", table_id, dim);
    if (rc == EMB_ERR_UNSUPPORTED)
        return fail(rc, "table %u: dim %u of dtype %d is not supported (dim must be > 0)", table_id, dim, (int)dtype);
    if (rc) return fail(rc, "table %u: bad dtype %d", table_id, (int)dtype);
    DeviceGuard g(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    Table &t = e->tables[table_id];
    size_t bytes = (size_t)nr_rows * row_stride(dtype, dim);
    if (t.n_hot) {   // (re)loading a table invalidates its hot-row copy
        HIP_TRY(hipDeviceSynchronize());
        clear_hot(t);
        t.generation = e->next_generation++;
    }
    if (t.rows && t.bytes != bytes) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipFree(t.rows));
        e->table_bytes -= t.bytes;
        t = Table{};
    }
    if (!t.rows) {
        HIP_TRY(hipMalloc(&t.rows, bytes));
        e->table_bytes += bytes;
        t.generation = e->next_generation++;
    }
    if (zero_fill) HIP_TRY(hipMemset(t.rows, 0, bytes));   // emb_load_table overwrites every byte anyway
    if (t.nr_rows != nr_rows || t.dim != dim || t.dtype != dtype)
        t.generation = e->next_generation++;   // same bytes, different shape: plans built on the old shape are stale
    t.nr_rows = nr_rows;
    t.dim = dim;
    t.dtype = dtype;
    t.geom = geom;
    t.bytes = bytes;
    return EMB_OK;
}

int emb_alloc_table(emb_engine *e, uint32_t table_id, uint64_t nr_rows, uint32_t dim, emb_dtype dtype) {
    return alloc_table(e, table_id, nr_rows, dim, pimemb::dtype_value(dtype), /*zero_fill=*/true);
}

int emb_load_table(emb_engine *e, uint32_t table_id, uint64_t nr_rows, uint32_t dim, emb_dtype dtype,
                   const void *rows, emb_memspace space) {
    if (!rows) return fail(EMB_ERR_INVALID, "table %u: rows is NULL", table_id);
    int rc = alloc_table(e, table_id, nr_rows, dim, pimemb::dtype_value(dtype), /*zero_fill=*/false);
    if (rc) return rc;
    DeviceGuard g(e->device);
    Table &t = e->tables[table_id];
    HIP_TRY(hipMemcpy(t.rows, rows, t.bytes,
                      space == EMB_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    return EMB_OK;
}

int emb_load_table_column(emb_engine *e, uint32_t table_id, uint32_t col, const int32_t *column,
                          uint64_t nr_rows) {
    if (!e || !column) return fail(EMB_ERR_INVALID, "engine or column is NULL");
    if (table_id >= e->tables.size() || !e->tables[table_id].rows)
        return fail(EMB_ERR_INVALID, "table %u is not allocated", table_id);
    Table &t = e->tables[table_id];
    if (t.dtype == pimemb::kMXFP4)
        return fail(EMB_ERR_UNSUPPORTED, "emb_load_table_column: table %u is MXFP4: a row interleaves 32-element blocks and their scales, it has no columns to load", table_id);
    if (t.dtype != EMB_FIXED32) return fail(EMB_ERR_INVALID, "table %u is not EMB_FIXED32", table_id);
    if (col >= t.dim) return fail(EMB_ERR_INVALID, "table %u: col %u >= dim %u", table_id, col, t.dim);
    if (nr_rows > t.nr_rows)
        return fail(EMB_ERR_INVALID, "table %u: %llu rows > allocated %llu", table_id,
                    (unsigned long long)nr_rows, (unsigned long long)t.nr_rows);
    DeviceGuard g(e->device);
    std::lock_guard<std::mutex> host_lk(e->host_mu);         // (the staging buffers and the copier are the host-pointer path's)
    std::lock_guard<std::mutex> lk(e->mu);
    if (t.n_hot) {
        HIP_TRY(hipDeviceSynchronize());
        clear_hot(t);
        t.generation = e->next_generation++;
    }
    size_t bytes = nr_rows * sizeof(int32_t);
    // through the pinned staging buffer (a few host threads pack it), not straight out of the caller's pageable column: a
    // synchronous copy from pageable memory runs at ~6 GB/s on this runtime (0.69 ms for the 4 MB of a million-row column),
    // pack + copy from pinned memory at the link's rate
    int rc = ensure_stage(e, bytes, bytes);
    if (rc) return rc;
    std::vector<pimemb::CopyPiece> pack{{e->h_stage, column, bytes}};
    e->copier.copy(pack);
    HIP_TRY(hipMemcpyAsync(e->d_stage, e->h_stage, bytes, hipMemcpyHostToDevice, nullptr));
    HIP_TRY(pimemb::launch_scatter_column(static_cast<int32_t *>(t.rows),
                                          reinterpret_cast<const int32_t *>(e->d_stage), nr_rows,
                                          t.dim, col, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return EMB_OK;
}

int emb_set_hot_rows(emb_engine *e, uint32_t table_id, const uint64_t *row_ids, uint32_t n_rows) {
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    if (table_id >= e->tables.size() || !e->tables[table_id].rows)
        return fail(EMB_ERR_INVALID, "table %u is not loaded", table_id);
    if (n_rows && !row_ids) return fail(EMB_ERR_INVALID, "row_ids is NULL");
    if (e->tables[table_id].dtype == pimemb::kMXFP4)
        return fail(EMB_ERR_UNSUPPORTED, "emb_set_hot_rows: table %u is MXFP4, which has no hot-row kernel", table_id);
    DeviceGuard g(e->device);
    std::lock_guard<std::mutex> lk(e->mu);
    Table &t = e->tables[table_id];
    HIP_TRY(hipDeviceSynchronize());             // launches that still read the previous set
    clear_hot(t);
    t.generation = e->next_generation++;         // prepared plans carry the old pointers: stale now
    if (n_rows == 0) return EMB_OK;
    if (t.geom.scalar_lanes) return EMB_OK;      // element-per-thread rows: no LDS path, the hint is ignored
    const uint32_t row_bytes = t.geom.chunks * 16u;
    pimemb::HotSet hs = pimemb::build_hot_set(row_ids, n_rows, t.nr_rows, row_bytes, pimemb::kHotLdsBudget);
    if (hs.rows.empty()) return EMB_OK;
    HIP_TRY(hipMalloc(&t.hot_rows, hs.rows.size() * (size_t)row_bytes));
    hipError_t err = hipMalloc((void **)&t.hot_hash, hs.hash.size() * 8);
    {   // the rows themselves: their ids go up once, ONE kernel copies them (a copy per row cost ~10 us each: a millisecond per table)
        unsigned long long *d_ids = nullptr;
        std::vector<unsigned long long> ids(hs.rows.begin(), hs.rows.end());
        if (err == hipSuccess) err = hipMalloc((void **)&d_ids, ids.size() * 8);
        if (err == hipSuccess) err = hipMemcpy(d_ids, ids.data(), ids.size() * 8, hipMemcpyHostToDevice);
        if (err == hipSuccess) err = pimemb::launch_gather_rows(t.hot_rows, t.rows, d_ids, (uint32_t)ids.size(), row_bytes, nullptr);
        if (err == hipSuccess) err = hipStreamSynchronize(nullptr);
        if (d_ids) (void)hipFree(d_ids);
    }
    if (err == hipSuccess) err = hipMemcpy(t.hot_hash, hs.hash.data(), hs.hash.size() * 8, hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        clear_hot(t);
        return fail(EMB_ERR_DEVICE, "emb_set_hot_rows: %s", hipGetErrorString(err));
    }
    t.n_hot = (uint32_t)hs.rows.size();
    t.hot_log2 = hs.log2size;
    t.hot_lds = hs.lds_bytes(row_bytes);
    return EMB_OK;
}

int emb_learn_hot_rows(emb_engine *e, uint32_t table_id, const void *indices, uint64_t n_indices, emb_index_type itype,
                       emb_memspace space, uint32_t max_rows, float min_share, void *stream, uint32_t *n_chosen, float *share) {
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    if (table_id >= e->tables.size() || !e->tables[table_id].rows) return fail(EMB_ERR_INVALID, "table %u is not loaded", table_id);
    if (itype != EMB_IDX_U32 && itype != EMB_IDX_I64) return fail(EMB_ERR_INVALID, "bad index type");
    if (n_indices && !indices) return fail(EMB_ERR_INVALID, "emb_learn_hot_rows: indices is NULL");
    if (e->tables[table_id].dtype == pimemb::kMXFP4)
        return fail(EMB_ERR_UNSUPPORTED, "emb_learn_hot_rows: table %u is MXFP4, which has no hot-row kernel", table_id);
    if (n_chosen) *n_chosen = 0;
    if (share) *share = 0.f;
    // the sample: up to four evenly spaced runs of 65 536 ids (the whole array when it is that small) -- bags are independent
    // draws, so runs of consecutive bags are a fair sample; four of them keep a sorted batch from showing its smallest ids only
    constexpr uint64_t kRun = 65536, kRuns = 4;
    const size_t isz = index_size(itype);
    std::vector<char> host;
    uint64_t n_sample = 0;
    if (n_indices) {
        DeviceGuard g(e->device);
        const uint64_t runs = n_indices <= kRun * kRuns ? 1 : kRuns;
        const uint64_t len = runs == 1 ? n_indices : kRun;
        host.resize((size_t)(runs * len) * isz);
        hipStream_t s = static_cast<hipStream_t>(stream);
        for (uint64_t r = 0; r < runs; r++) {
            const uint64_t at = runs == 1 ? 0 : r * ((n_indices - len) / (runs - 1));
            const char *src = static_cast<const char *>(indices) + at * isz;
            if (space == EMB_MEM_DEVICE) HIP_TRY(hipMemcpyAsync(host.data() + (size_t)(r * len) * isz, src, (size_t)len * isz, hipMemcpyDeviceToHost, s));
            else memcpy(host.data() + (size_t)(r * len) * isz, src, (size_t)len * isz);
        }
        if (space == EMB_MEM_DEVICE) HIP_TRY(hipStreamSynchronize(s));
        n_sample = runs * len;
    }
    const uint64_t nr_rows = e->tables[table_id].nr_rows;
    std::unordered_map<uint64_t, uint32_t> count;
    count.reserve((size_t)std::min<uint64_t>(n_sample, 1u << 20));
    for (uint64_t i = 0; i < n_sample; i++) {
        const uint64_t id = itype == EMB_IDX_I64 ? (uint64_t)reinterpret_cast<const int64_t *>(host.data())[i]
                                                 : (uint64_t)reinterpret_cast<const uint32_t *>(host.data())[i];
        if (id < nr_rows) count[id]++;            // (an id outside the table is nobody's hot row)
    }
    std::vector<std::pair<uint32_t, uint64_t>> by_count;       // (count, id): most frequent first, smaller id first among equals
    by_count.reserve(count.size());
    for (const auto &kv : count) by_count.emplace_back(kv.second, kv.first);
    const size_t k = std::min<size_t>(max_rows, by_count.size());
    std::partial_sort(by_count.begin(), by_count.begin() + (long)k, by_count.end(),
                      [](const std::pair<uint32_t, uint64_t> &a, const std::pair<uint32_t, uint64_t> &b) {
                          return a.first != b.first ? a.first > b.first : a.second < b.second;
                      });
    uint64_t covered = 0;
    std::vector<uint64_t> ids(k);
    for (size_t i = 0; i < k; i++) {
        ids[i] = by_count[i].second;
        covered += by_count[i].first;
    }
    const float sh = n_sample ? (float)((double)covered / (double)n_sample) : 0.f;
    if (share) *share = sh;
    if (k == 0 || sh < min_share) return emb_set_hot_rows(e, table_id, nullptr, 0);       // near-uniform accesses: no LDS copy
    int rc = emb_set_hot_rows(e, table_id, ids.data(), (uint32_t)k);
    if (rc == EMB_OK && n_chosen) *n_chosen = e->tables[table_id].n_hot;
    return rc;
}

int emb_table_hot_count(emb_engine *e, uint32_t table_id, uint32_t *n_rows) {
    if (!e || !n_rows) return fail(EMB_ERR_INVALID, "engine or n_rows is NULL");
    if (table_id >= e->tables.size() || !e->tables[table_id].rows)
        return fail(EMB_ERR_INVALID, "table %u is not loaded", table_id);
    *n_rows = e->tables[table_id].n_hot;
    return EMB_OK;
}

int emb_table_info(emb_engine *e, uint32_t table_id, void **device_rows, uint64_t *nr_rows,
                   uint32_t *dim, emb_dtype *dtype) {
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    if (table_id >= e->tables.size() || !e->tables[table_id].rows)
        return fail(EMB_ERR_INVALID, "table %u is not loaded", table_id);
    const Table &t = e->tables[table_id];
    if (device_rows) *device_rows = t.rows;
    if (nr_rows) *nr_rows = t.nr_rows;
    if (dim) *dim = t.dim;
    if (dtype) pimemb::dtype_store(dtype, t.dtype);
    return EMB_OK;
}

static int validate_on(emb_engine *e, const emb_lookup_desc *descs, uint32_t n_descs, emb_index_type itype,
                       emb_memspace space, hipStream_t s, uint64_t *n_bad);
static int checked_launch(emb_engine *e, Resolved &r, emb_index_type itype, hipStream_t s, bool launch, uint64_t *n_bad, bool defer = false);

static int lookup_batched_impl(emb_engine *e, const emb_lookup_desc *descs, uint32_t n_descs, emb_index_type itype,
                               emb_memspace space, void *stream, bool check, uint64_t *n_bad, bool defer = false,
                               const emb_pool_spec *pools = nullptr, const uint64_t *out_stride = nullptr) {
    if (n_bad) *n_bad = 0;
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    if (n_descs == 0) return EMB_OK;
    if (!descs) return fail(EMB_ERR_INVALID, "descs is NULL");
    DeviceGuard g(e->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    e->n_lookup_calls.fetch_add(1, std::memory_order_relaxed);
    if (space == EMB_MEM_HOST) {
        if (check) {         // refuse the call instead of gathering a wild row
            int vrc = validate_on(e, descs, n_descs, itype, space, s, n_bad);
            if (vrc) return vrc;
        }
        return lookup_host(e, descs, n_descs, itype, s, pools);
    }
    Resolved r;
    r.stream = s;
    const double p0 = g_prof.on ? now_us() : 0;
    int rc = resolve(e, descs, n_descs, itype, nullptr, nullptr, nullptr, &r, /*cache_maps=*/true, nullptr, nullptr, pools, nullptr, out_stride);
    if (rc) return rc;
    if (g_prof.on) g_prof.resolve += now_us() - p0;
    // checked: the descriptors are resolved ONCE; the validation kernel and the lookup kernels share one launch image and
    // are enqueued back to back -- a finding disarms the lookup on the device (validate_kernel's poison) -- and the host
    // waits for the validation result only
    rc = check ? checked_launch(e, r, itype, s, /*launch=*/true, n_bad, defer) : launch_resolved(e, r, itype, s);
    if (rc != EMB_OK && !(defer && rc == EMB_ERR_RANGE)) return rc;      // (deferred: EMB_ERR_RANGE speaks of an EARLIER call; this one was launched)
    e->n_bags.fetch_add(r.n_bags, std::memory_order_relaxed);
    e->n_indices.fetch_add(r.n_indices, std::memory_order_relaxed);
    return rc;
}

int emb_lookup_batched(emb_engine *e, const emb_lookup_desc *descs, uint32_t n_descs,
                       emb_index_type itype, emb_memspace space, void *stream) {
    return lookup_batched_impl(e, descs, n_descs, itype, space, stream, e && e->check_inputs, nullptr, e && e->defer_check);
}

int emb_lookup_batched_checked_deferred(emb_engine *e, const emb_lookup_desc *descs, uint32_t n_descs,
                                        emb_index_type itype, emb_memspace space, void *stream) {
    return lookup_batched_impl(e, descs, n_descs, itype, space, stream, true, nullptr, /*defer=*/space == EMB_MEM_DEVICE);
}

int emb_lookup_batched_checked(emb_engine *e, const emb_lookup_desc *descs, uint32_t n_descs,
                               emb_index_type itype, emb_memspace space, void *stream, uint64_t *n_bad) {
    return lookup_batched_impl(e, descs, n_descs, itype, space, stream, true, n_bad);
}

// Pooled specs that all ask for plain sum (or none at all) are today's call, untouched.
static const emb_pool_spec *live_pools(const emb_pool_spec *pools, uint32_t n_descs) {
    if (pools)
        for (uint32_t i = 0; i < n_descs; i++)
            if (!is_plain_sum(pools[i])) return pools;
    return nullptr;
}

int emb_lookup_pooled(emb_engine *e, const emb_lookup_desc *descs, const emb_pool_spec *pools, uint32_t n_descs,
                      emb_index_type itype, emb_memspace space, void *stream, uint32_t check, uint64_t *n_bad) {
    if (n_bad) *n_bad = 0;
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    if (check > 2) return fail(EMB_ERR_INVALID, "emb_lookup_pooled: check must be 0, 1 or 2 (got %u)", check);
    if (n_descs && !descs) return fail(EMB_ERR_INVALID, "descs is NULL");
    const emb_pool_spec *live = live_pools(pools, n_descs);
    if (check == 0)        // as emb_lookup_batched: the engine's own flags decide
        return lookup_batched_impl(e, descs, n_descs, itype, space, stream, e->check_inputs, nullptr, e->defer_check, live);
    return lookup_batched_impl(e, descs, n_descs, itype, space, stream, true, n_bad, check == 2 && space == EMB_MEM_DEVICE, live);
}

int emb_lookup(emb_engine *e, uint32_t table_id, const void *indices, uint64_t n_indices,
               const void *offsets, uint64_t n_bags, float *pooled, emb_index_type itype,
               emb_memspace space, void *stream) {
    emb_lookup_desc d{};
    d.table_id = table_id;
    d.indices = indices;
    d.offsets = offsets;
    d.n_indices = n_indices;
    d.n_bags = n_bags;
    d.pooled = pooled;
    if (!offsets && n_bags) {
        if (n_indices % n_bags) return fail(EMB_ERR_INVALID, "offsets is NULL and n_indices %% n_bags != 0");
        d.fixed_pooling = (uint32_t)(n_indices / n_bags);
    }
    return emb_lookup_batched(e, &d, 1, itype, space, stream);
}

int emb_lookup_ranged(emb_engine *e, const emb_lookup_desc *descs, const uint64_t *row_lo, uint32_t n_descs, void *stream) {
    return emb_lookup_ranged_counted(e, descs, row_lo, nullptr, n_descs, stream);
}

int emb_lookup_ranged_counted(emb_engine *e, const emb_lookup_desc *descs, const uint64_t *row_lo, uint32_t *const *served,
                              uint32_t n_descs, void *stream) {
    return emb_lookup_ranged_typed(e, descs, row_lo, served, n_descs, EMB_IDX_U32, stream);
}

int emb_lookup_ranged_typed(emb_engine *e, const emb_lookup_desc *descs, const uint64_t *row_lo, uint32_t *const *served,
                            uint32_t n_descs, emb_index_type itype, void *stream) {
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    if (n_descs == 0) return EMB_OK;
    if (!descs || !row_lo) return fail(EMB_ERR_INVALID, "emb_lookup_ranged: NULL argument");
    DeviceGuard g(e->device);
    Resolved r;
    r.stream = static_cast<hipStream_t>(stream);
    int rc = resolve(e, descs, n_descs, itype, nullptr, nullptr, nullptr, &r, /*cache_maps=*/true, row_lo, served);
    if (rc) return rc;
    rc = launch_resolved(e, r, itype, static_cast<hipStream_t>(stream));
    if (rc) return rc;
    e->n_lookup_calls.fetch_add(1, std::memory_order_relaxed);
    e->n_bags.fetch_add(r.n_bags, std::memory_order_relaxed);
    e->n_indices.fetch_add(r.n_indices, std::memory_order_relaxed);
    return EMB_OK;
}

static int plan_create(emb_engine *e, const emb_lookup_desc *descs, const uint64_t *row_lo, uint32_t *const *served,
                       uint32_t n_descs, emb_index_type itype, emb_plan **out, const emb_pool_spec *pools = nullptr,
                       const uint64_t *out_stride = nullptr);

// Strided pooled output: emb_lookup_pooled over DEVICE buffers with a row stride per descriptor (resolve: out_stride).  Strides
// that all say "dense" (0, or the table's dim) change nothing: the groups, and with them launches, signature and text, are the
// dense call's.
int emb_lookup_strided(emb_engine *e, const emb_lookup_desc *descs, const emb_pool_spec *pools, const uint64_t *out_stride,
                       uint32_t n_descs, emb_index_type itype, void *stream, uint32_t check, uint64_t *n_bad) {
    if (n_bad) *n_bad = 0;
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    if (check > 2) return fail(EMB_ERR_INVALID, "emb_lookup_strided: check must be 0, 1 or 2 (got %u)", check);
    if (n_descs && !descs) return fail(EMB_ERR_INVALID, "descs is NULL");
    const emb_pool_spec *live = live_pools(pools, n_descs);
    if (check == 0)
        return lookup_batched_impl(e, descs, n_descs, itype, EMB_MEM_DEVICE, stream, e->check_inputs, nullptr, e->defer_check, live, out_stride);
    return lookup_batched_impl(e, descs, n_descs, itype, EMB_MEM_DEVICE, stream, true, n_bad, check == 2, live, out_stride);
}

int emb_plan_create_strided(emb_engine *e, const emb_lookup_desc *descs, const emb_pool_spec *pools, const uint64_t *out_stride,
                            uint32_t n_descs, emb_index_type itype, emb_plan **out) {
    return plan_create(e, descs, nullptr, nullptr, n_descs, itype, out, live_pools(pools, n_descs), out_stride);
}

int emb_plan_create_ranged(emb_engine *e, const emb_lookup_desc *descs, const uint64_t *row_lo, uint32_t n_descs,
                           emb_plan **out) {
    if (!row_lo) return fail(EMB_ERR_INVALID, "emb_plan_create_ranged: row_lo is NULL");
    return plan_create(e, descs, row_lo, nullptr, n_descs, EMB_IDX_U32, out);
}

int emb_plan_create_ranged_counted(emb_engine *e, const emb_lookup_desc *descs, const uint64_t *row_lo, uint32_t *const *served,
                                   uint32_t n_descs, emb_plan **out) {
    if (!row_lo) return fail(EMB_ERR_INVALID, "emb_plan_create_ranged_counted: row_lo is NULL");
    return plan_create(e, descs, row_lo, served, n_descs, EMB_IDX_U32, out);
}

int emb_plan_create_ranged_typed(emb_engine *e, const emb_lookup_desc *descs, const uint64_t *row_lo, uint32_t *const *served,
                                 uint32_t n_descs, emb_index_type itype, emb_plan **out) {
    if (!row_lo) return fail(EMB_ERR_INVALID, "emb_plan_create_ranged_typed: row_lo is NULL");
    return plan_create(e, descs, row_lo, served, n_descs, itype, out);
}

int emb_plan_create(emb_engine *e, const emb_lookup_desc *descs, uint32_t n_descs,
                    emb_index_type itype, emb_plan **out) {
    return plan_create(e, descs, nullptr, nullptr, n_descs, itype, out);
}

int emb_plan_create_pooled(emb_engine *e, const emb_lookup_desc *descs, const emb_pool_spec *pools, uint32_t n_descs,
                           emb_index_type itype, emb_plan **out) {
    return plan_create(e, descs, nullptr, nullptr, n_descs, itype, out, live_pools(pools, n_descs));
}

static int plan_create(emb_engine *e, const emb_lookup_desc *descs, const uint64_t *row_lo, uint32_t *const *served,
                       uint32_t n_descs, emb_index_type itype, emb_plan **out, const emb_pool_spec *pools, const uint64_t *out_stride) {
    if (!e || !out) return fail(EMB_ERR_INVALID, "engine or out is NULL");
    *out = nullptr;
    if (!descs || n_descs == 0) return fail(EMB_ERR_INVALID, "plan needs at least one descriptor");
    DeviceGuard g(e->device);
    Resolved r;
    int rc = resolve(e, descs, n_descs, itype, nullptr, nullptr, nullptr, &r, false, row_lo, served, pools, nullptr, out_stride);
    if (rc) return rc;
    emb_plan *p = new (std::nothrow) emb_plan();
    if (!p) return fail(EMB_ERR_NOMEM, "out of host memory");
    p->e = e;
    p->itype = itype;
    {   // launch signature (emb_plan_signature): FNV-1a over everything that shapes the launches, nothing that names a buffer
        uint64_t h = 1469598103934665603ull;
        auto mix = [&h](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
        mix((uint64_t)itype);
        size_t di = 0;
        for (const PlanGroup &g : r.groups) {
            mix(g.kind); mix((uint64_t)g.dtype); mix(g.geom.lanes_per_row); mix(g.geom.chunks); mix(g.geom.scalar_lanes); mix(g.n); mix(g.max_tiles);
            mix(g.xgrid); mix(g.xdirect); mix(g.ranged); mix(g.hot_wgs); mix(g.hot_lds); mix(pimemb::bags_per_tile(g.kind, g.geom));
            if (g.pool) mix(0x706f6f6c00ull | g.pool);     // (plain-sum groups mix exactly what they always did)
            if (g.out_half) mix(0x6f757400ull | 1u);       // (... and so do fp32-out groups)
            if (g.strided) mix(0x7374726400ull | 1u);      // (... and dense ones)
            for (uint32_t w : g.xmap_words) mix(w);
            for (uint32_t i = 0; i < g.n; i++, di++) {
                const DevDesc &d = r.descs[di];
                mix(d.n_tiles); mix(d.n_bags); mix(d.n_idx); mix(d.nr_rows); mix(d.fixed_pooling); mix(d.offsets != nullptr); mix(d.n_hot);
                if (g.strided) mix(d.words[pimemb::kOutStrideWord]);       // (a layout, never an address)
                if (g.pool) {           // the pooling spec: the weights' presence, never their address
                    mix(d.pool.weights != nullptr); mix(d.pool.padding_row); mix(d.pool.op);
                } else {
                    mix(d.ranged.row_lo); mix(d.ranged.served != nullptr);
                }
            }
        }
        p->signature = h;
    }
    p->bytes = r.bytes;
    p->n_bags = r.n_bags;
    p->n_indices = r.n_indices;
    char *d = nullptr;
    hipError_t err = hipMalloc((void **)&d, r.image.size());
    if (err == hipSuccess) err = hipMemcpy(d, r.image.data(), r.image.size(), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        if (d) (void)hipFree(d);
        delete p;
        return fail(EMB_ERR_DEVICE, "emb_plan_create: %s", hipGetErrorString(err));
    }
    r.bind(d);
    p->d_image = d;
    p->groups = r.groups;
    for (uint32_t i = 0; i < n_descs; i++)
        p->table_gens.emplace_back(descs[i].table_id, e->tables[descs[i].table_id].generation);
    e->live_plans.fetch_add(1);
    *out = p;
    return EMB_OK;
}

int emb_plan_launch(emb_plan *p, void *stream) {
    if (!p) return fail(EMB_ERR_INVALID, "plan is NULL");
    emb_engine *e = p->e;
    for (const auto &tg : p->table_gens)   // a table re-allocated since emb_plan_create would be a dangling pointer
        if (e->tables[tg.first].generation != tg.second)
            return fail(EMB_ERR_INVALID, "plan is stale: table %u was re-allocated after emb_plan_create", tg.first);
    DeviceGuard g(e->device);
    int rc = launch_groups(e, p->groups, p->itype, static_cast<hipStream_t>(stream));
    if (rc) return rc;
    e->n_lookup_calls.fetch_add(1, std::memory_order_relaxed);
    e->n_bags.fetch_add(p->n_bags, std::memory_order_relaxed);
    e->n_indices.fetch_add(p->n_indices, std::memory_order_relaxed);
    return EMB_OK;
}

int emb_plan_destroy(emb_plan *p) {
    if (!p) return EMB_OK;
    DeviceGuard g(p->e->device);
    (void)hipDeviceSynchronize();
    if (p->d_image) (void)hipFree(p->d_image);
    p->e->live_plans.fetch_sub(1);
    delete p;
    return EMB_OK;
}

int emb_plan_bytes(const emb_plan *p, uint64_t *algorithmic_bytes, uint64_t *n_bags,
                   uint64_t *n_indices) {
    if (!p) return fail(EMB_ERR_INVALID, "plan is NULL");
    if (algorithmic_bytes) *algorithmic_bytes = p->bytes;
    if (n_bags) *n_bags = p->n_bags;
    if (n_indices) *n_indices = p->n_indices;
    return EMB_OK;
}

int emb_plan_describe(const emb_plan *p, char *buf, size_t capacity) {
    if (!p || !buf || capacity == 0) return fail(EMB_ERR_INVALID, "emb_plan_describe: NULL argument");
    size_t at = 0;
    buf[0] = 0;
    for (const PlanGroup &g : p->groups) {
        const uint32_t block = g.kind == pimemb::KERNEL_ANYDIM ? 256u : (g.geom.lanes_per_row ? pimemb::bags_per_tile(g.kind, g.geom) : 0u);
        const int n = snprintf(buf + at, capacity - at, "%skind=%u dtype=%d itype=%d lanes_per_row=%u chunks=%u scalar_lanes=%u anydim_vec=%d ranged=%d descs=%u "
                               "grid=%u bags_per_tile=%u", at ? ";" : "", (unsigned)g.kind, (int)g.dtype, (int)p->itype, g.geom.lanes_per_row, g.geom.chunks,
                               g.geom.scalar_lanes, (int)g.geom.anydim_vec, (int)g.ranged, g.n, g.d_xmap ? g.xgrid : g.max_tiles * g.n, block);
        if (n < 0 || (size_t)n >= capacity - at) return fail(EMB_ERR_INVALID, "emb_plan_describe: %zu bytes do not hold the text", capacity);
        at += (size_t)n;
        if (g.pool) {
            const int m = snprintf(buf + at, capacity - at, " pool=%u weighted=%u padding=%u", g.pool - 1u, g.n_weighted, g.n_padding);
            if (m < 0 || (size_t)m >= capacity - at) return fail(EMB_ERR_INVALID, "emb_plan_describe: %zu bytes do not hold the text", capacity);
            at += (size_t)m;
        }
        if (g.out_half) {
            const int m = snprintf(buf + at, capacity - at, " out=1");
            if (m < 0 || (size_t)m >= capacity - at) return fail(EMB_ERR_INVALID, "emb_plan_describe: %zu bytes do not hold the text", capacity);
            at += (size_t)m;
        }
        if (g.strided) {
            const int m = snprintf(buf + at, capacity - at, " strided=1");
            if (m < 0 || (size_t)m >= capacity - at) return fail(EMB_ERR_INVALID, "emb_plan_describe: %zu bytes do not hold the text", capacity);
            at += (size_t)m;
        }
    }
    return EMB_OK;
}

int emb_plan_signature(const emb_plan *p, uint64_t *signature) {
    if (!p || !signature) return fail(EMB_ERR_INVALID, "emb_plan_signature: NULL argument");
    *signature = p->signature;
    return EMB_OK;
}

int emb_plan_time(emb_plan *p, void *stream, uint32_t warmup, uint32_t iters, float *avg_us) {
    if (!p || !avg_us || iters == 0) return fail(EMB_ERR_INVALID, "bad argument to emb_plan_time");
    DeviceGuard g(p->e->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (uint32_t i = 0; i < warmup; i++) {
        int rc = emb_plan_launch(p, stream);
        if (rc) return rc;
    }
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    HIP_TRY(hipEventRecord(a, s));
    for (uint32_t i = 0; i < iters; i++) {
        int rc = emb_plan_launch(p, stream);
        if (rc) return rc;
    }
    HIP_TRY(hipEventRecord(b, s));
    HIP_TRY(hipEventSynchronize(b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    *avg_us = ms * 1000.f / (float)iters;
    return EMB_OK;
}

// After a failed enqueue on the validation path: a validation kernel may or may not be queued, so its counters may or may
// not come back zeroed.  Let the device drain, zero them all, and forget the verdicts that were outstanding (whatever they
// found disarmed their lookups on the device all the same).
static void resync_validation(emb_engine *e) {
    (void)hipDeviceSynchronize();
    if (e->d_val) (void)hipMemset(e->d_val, 0, sizeof(pimemb::ValidateCtl) * emb_engine::kValSlots);
    e->val_pending.clear();
    (void)hipGetLastError();
}

// Read the verdicts of deferred checked calls, oldest first (caller holds val_mu).  wait = false: only those that have arrived;
// wait = true: all of them (a spin, then the call's stream).  What they found is ADDED to e->val_owed_bad (val_owed_first: the
// sequence number of the first call it belongs to) and stays owed until a caller hands it over (take_owed) -- a call that fails
// for a reason of its own between reading a verdict and returning does not lose it.  A refused call's lookup kernels were
// disarmed on the device: they are taken out of the launch statistics here.  own_seq / own_bad: the finding of THAT call is
// returned apart (not owed to anybody else).
static int read_verdicts(emb_engine *e, bool wait, unsigned long long own_seq, unsigned long long *own_bad) {
    if (own_bad) *own_bad = 0;
    while (!e->val_pending.empty()) {
        const emb_engine::PendingVerdict pv = e->val_pending.front();
        const uint32_t slot = (uint32_t)(pv.seq % emb_engine::kValSlots);
        volatile unsigned long long *result = e->val_result + slot;
        unsigned long long word = *result;
        if ((word >> 24) != pv.seq) {
            if (!wait) break;
            for (int spin = 0; spin < 200000 && ((word = *result) >> 24) != pv.seq; spin++) {
            }
            if ((word >> 24) != pv.seq) {
                if (hipStreamSynchronize(pv.stream) != hipSuccess) {     // (the caller may have destroyed the stream since: wait for the device)
                    (void)hipGetLastError();
                    HIP_TRY(hipDeviceSynchronize());
                }
                if (((word = *result) >> 24) != pv.seq) {
                    resync_validation(e);
                    return fail(EMB_ERR_DEVICE, "validation kernel of checked call %llu did not report", pv.seq);
                }
            }
        }
        e->val_pending.pop_front();
        const unsigned long long bad = word & pimemb::kValCountMask;
        if (bad) {
            if (own_bad && pv.seq == own_seq) {
                *own_bad = bad;
            } else {
                if (!e->val_owed_bad) e->val_owed_first = pv.seq;
                e->val_owed_bad += bad;
            }
            if (pv.launched) {
                e->n_kernel_launches.fetch_sub(pv.n_groups, std::memory_order_relaxed);
                for (uint32_t g = 0; g < pv.n_groups && g < 8; g++) e->n_by_kind[pv.kinds[g]].fetch_sub(1, std::memory_order_relaxed);
            }
        }
    }
    return EMB_OK;
}

// Validate the resolved descriptors of a call (device-resident buffers) on stream `s` and -- with `launch` -- enqueue its
// lookup kernels right behind the validation kernel, over the SAME launch image: a finding zeroes the descriptors' tile
// counts on the device, so the lookup does nothing.  The host waits for the validation result only (one pinned word the
// kernel's last workgroup writes; polled), not for the lookup -- or, `defer`, for nothing at all: the verdict is read by a
// later checked call (which returns EMB_ERR_RANGE for it, after having launched its own work) or by emb_check_report; the wait
// inside the call puts the host one launch behind the GPU on every call (21 -> 41 us per 26-table call at 39 292 bags per table).
// No allocation on this path (the counter block and the pinned result words are created once), no event, no device-wide
// synchronize.  Checked calls take turns enqueueing (val_mu); the ring mutex is held while the call enqueues, not while it waits.
static int checked_launch(emb_engine *e, Resolved &r, emb_index_type itype, hipStream_t s, bool launch, uint64_t *n_bad, bool defer) {
    if (n_bad) *n_bad = 0;
    if (r.descs.empty()) return EMB_OK;
    if (r.descs.size() > 65535u) return fail(EMB_ERR_UNSUPPORTED, "a checked call takes at most 65535 descriptors (%zu given)", r.descs.size());
    std::lock_guard<std::mutex> vlk(e->val_mu);
    unsigned long long seq = 0;
    // verdicts of earlier deferred calls: what has arrived (all of them before a slot is reused).  A call that waits for its own
    // verdict reads them behind its launch, in one wait.
    if (defer && !e->val_pending.empty()) EMB_TRY(read_verdicts(e, /*wait=*/false));
    if (e->val_pending.size() + 1 >= emb_engine::kValSlots) EMB_TRY(read_verdicts(e, /*wait=*/true));
    volatile unsigned long long *result = nullptr;
    uint32_t slot = 0;
    {
        // (d_val, val_result and the val_* bookkeeping are only touched under val_mu, held above)
        const int rk = ring_of_thread();
        std::lock_guard<std::mutex> lk(e->ring_mu[rk]);        // enqueue only; released before the wait below
        if (!e->d_val) {
            HIP_TRY(hipMalloc((void **)&e->d_val, sizeof(pimemb::ValidateCtl) * emb_engine::kValSlots));
            HIP_TRY(hipMemset(e->d_val, 0, sizeof(pimemb::ValidateCtl) * emb_engine::kValSlots));
        }
        if (!e->val_result) {     // its own pinned block, not the launch-image ring: a segment may be recycled while we wait
            void *p = nullptr;
            HIP_TRY(hipHostMalloc(&p, 8 * emb_engine::kValSlots, hipHostMallocMapped | hipHostMallocCoherent));
            memset(p, 0, 8 * emb_engine::kValSlots);
            e->val_result = static_cast<volatile unsigned long long *>(p);
        }
        seq = ++e->val_seq;
        slot = (uint32_t)(seq % emb_engine::kValSlots);
        result = e->val_result + slot;
        char *h = nullptr, *d = nullptr;
        int rc = take_image_space(e->ring[rk], r.image.size(), s, &h, &d);
        if (rc) return rc;
        memcpy(h, r.image.data(), r.image.size());
        char *base = h;        // the kernels' scalar loads read the pinned, device-visible segment itself ...
        if (d != nullptr) {    // ... or its HBM twin (PIMEMB_DESC_MODE=copy)
            HIP_TRY(hipMemcpyAsync(d, h, r.image.size(), hipMemcpyHostToDevice, s));
            base = d;
        }
        r.bind(base);
        uint64_t max_items = 1;
        for (const DevDesc &dd : r.descs) max_items = std::max<uint64_t>(max_items, std::max<uint64_t>(dd.n_idx, dd.n_bags));
        const uint32_t wgs = pimemb::validate_workgroups(max_items, itype);
        hipError_t err = pimemb::launch_validate(reinterpret_cast<DevDesc *>(base + r.groups[0].desc_off), (uint32_t)r.descs.size(),
                                                 itype, e->d_val + slot, const_cast<unsigned long long *>(result), seq, wgs,
                                                 /*poison=*/launch, s);
        if (err != hipSuccess) {
            resync_validation(e);
            return fail(EMB_ERR_DEVICE, "validation kernel: %s", hipGetErrorString(err));
        }
        if (launch) {
            rc = launch_groups(e, r.groups, itype, s);
            if (rc) {                              // (the validation kernel runs and reports; its verdict has no call to belong to)
                resync_validation(e);
                return rc;
            }
        }
        emb_engine::PendingVerdict pv{seq, s, (uint32_t)r.groups.size(), {}, launch};
        for (size_t g = 0; g < r.groups.size() && g < 8; g++) pv.kinds[g] = r.groups[g].kind;
        e->val_pending.push_back(pv);
    }
    unsigned long long bad = 0;
    if (!defer) EMB_TRY(read_verdicts(e, /*wait=*/true, seq, &bad));      // this call's own verdict, and whatever was still outstanding in front of it
    const unsigned long long earlier_bad = e->val_owed_bad, earlier_seq = e->val_owed_first;      // handed over now
    e->val_owed_bad = e->val_owed_first = 0;
    if (n_bad) *n_bad = bad + earlier_bad;
    if (bad) {
        if (earlier_bad)
            return fail(EMB_ERR_RANGE, "%llu out-of-range indices / broken offsets (and %llu in EARLIER checked calls whose verdict was deferred, "
                        "the first of them number %llu of this engine)", bad, earlier_bad, earlier_seq);
        return fail(EMB_ERR_RANGE, "%llu out-of-range indices / broken offsets", bad);
    }
    if (earlier_bad)
        return fail(EMB_ERR_RANGE, "%llu out-of-range indices / broken offsets in an EARLIER checked call (number %llu of this engine; its "
                    "lookup was disarmed on the device: outputs untouched) -- reported now: the verdict was deferred", earlier_bad, earlier_seq);
    return EMB_OK;
}

// The same for a batched call as the caller describes it; host buffers are staged into HBM first.
static int validate_on(emb_engine *e, const emb_lookup_desc *descs, uint32_t n_descs, emb_index_type itype,
                       emb_memspace space, hipStream_t s, uint64_t *n_bad) {
    HostStage hs;
    Resolved r;
    r.stream = s;
    int rc;
    std::unique_lock<std::mutex> host_lk(e->host_mu, std::defer_lock);
    if (space == EMB_MEM_HOST) host_lk.lock();
    std::vector<emb_lookup_desc> tmp(descs, descs + n_descs);
    for (uint32_t i = 0; i < n_descs; i++)
        if (!tmp[i].pooled) tmp[i].pooled = (float *)16;   // pooled pointers are not touched by validation
    if (space == EMB_MEM_HOST) {
        {
            std::lock_guard<std::mutex> lk(e->mu);
            rc = stage_host_inputs(e, descs, n_descs, itype, s, &hs, false);
        }
        if (rc) return rc;
        rc = resolve(e, tmp.data(), n_descs, itype, &hs.d_indices, &hs.d_offsets, nullptr, &r, /*cache_maps=*/true);
    } else {
        rc = resolve(e, tmp.data(), n_descs, itype, nullptr, nullptr, nullptr, &r, /*cache_maps=*/true);
    }
    if (rc) return rc;
    return checked_launch(e, r, itype, s, /*launch=*/false, n_bad);
}

int emb_validate_inputs(emb_engine *e, const emb_lookup_desc *descs, uint32_t n_descs,
                        emb_index_type itype, emb_memspace space, uint64_t *n_bad) {
    return emb_validate_inputs_on(e, descs, n_descs, itype, space, nullptr, n_bad);
}

int emb_validate_inputs_on(emb_engine *e, const emb_lookup_desc *descs, uint32_t n_descs, emb_index_type itype,
                           emb_memspace space, void *stream, uint64_t *n_bad) {
    if (!e || !descs) return fail(EMB_ERR_INVALID, "engine or descs is NULL");
    DeviceGuard g(e->device);
    return validate_on(e, descs, n_descs, itype, space, static_cast<hipStream_t>(stream), n_bad);
}

int emb_check_report(emb_engine *e, uint64_t *n_bad) {
    if (n_bad) *n_bad = 0;
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    DeviceGuard g(e->device);
    std::lock_guard<std::mutex> vlk(e->val_mu);
    EMB_TRY(read_verdicts(e, /*wait=*/true));
    const unsigned long long bad = e->val_owed_bad, first = e->val_owed_first;
    e->val_owed_bad = e->val_owed_first = 0;
    if (n_bad) *n_bad = bad;
    if (bad)
        return fail(EMB_ERR_RANGE, "%llu out-of-range indices / broken offsets in checked call number %llu of this engine (its lookup was "
                    "disarmed on the device: outputs untouched)", bad, first);
    return EMB_OK;
}

int emb_get_stats(emb_engine *e, emb_stats *out) {
    if (!e || !out) return fail(EMB_ERR_INVALID, "engine or out is NULL");
    memset(out, 0, sizeof *out);
    out->n_lookup_calls = e->n_lookup_calls.load();
    out->n_kernel_launches = e->n_kernel_launches.load();
    out->n_bags = e->n_bags.load();
    out->n_indices = e->n_indices.load();
    out->table_bytes = e->table_bytes;
    out->us_copy_in_indices = e->us_copy_in_indices;
    out->us_copy_in_lengths = e->us_copy_in_lengths;
    out->us_launch = e->us_launch;
    out->us_copy_out = e->us_copy_out;
    out->us_post_process = 0.0;
    out->us_sync = e->us_sync;
    for (int k = 0; k < 5; k++) out->n_launches_by_kind[k] = e->n_by_kind[k].load();
    return EMB_OK;
}

int emb_reset_stats(emb_engine *e) {
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    e->n_lookup_calls = 0;
    e->n_kernel_launches = 0;
    e->n_bags = 0;
    e->n_indices = 0;
    for (auto &k : e->n_by_kind) k = 0;
    e->us_copy_in_indices = e->us_copy_in_lengths = e->us_launch = e->us_copy_out = e->us_sync = 0;
    return EMB_OK;
}

int emb_set_stage_timing(emb_engine *e, int on) {
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    e->stage_timing = on != 0;
    return EMB_OK;
}

int emb_trace_enable(emb_engine *e, uint32_t capacity) {
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    e->trace_cap = capacity;
    e->trace.clear();
    e->host_call_id = 0;
    return EMB_OK;
}

int emb_trace_read(emb_engine *e, emb_trace_event *out, uint32_t max_events, uint32_t *n_events) {
    if (!e || !n_events || (max_events && !out)) return fail(EMB_ERR_INVALID, "bad argument to emb_trace_read");
    std::lock_guard<std::mutex> lk(e->mu);
    uint32_t n = 0;
    while (n < max_events && !e->trace.empty()) {
        out[n++] = e->trace.front();
        e->trace.pop_front();
    }
    *n_events = n;
    return EMB_OK;
}

int emb_device_alloc(emb_engine *e, size_t bytes, void **out) {
    if (!e || !out) return fail(EMB_ERR_INVALID, "engine or out is NULL");
    DeviceGuard g(e->device);
    *out = nullptr;
    HIP_TRY(hipMalloc(out, bytes ? bytes : 16));
    return EMB_OK;
}

int emb_device_free(emb_engine *e, void *ptr) {
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    if (!ptr) return EMB_OK;
    DeviceGuard g(e->device);
    HIP_TRY(hipFree(ptr));
    return EMB_OK;
}

int emb_copy_to_device(emb_engine *e, void *dst_device, const void *src_host, size_t bytes) {
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    if (!bytes) return EMB_OK;
    DeviceGuard g(e->device);
    HIP_TRY(hipMemcpy(dst_device, src_host, bytes, hipMemcpyHostToDevice));
    return EMB_OK;
}

int emb_copy_to_host(emb_engine *e, void *dst_host, const void *src_device, size_t bytes) {
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    if (!bytes) return EMB_OK;
    DeviceGuard g(e->device);
    HIP_TRY(hipMemcpy(dst_host, src_device, bytes, hipMemcpyDeviceToHost));
    return EMB_OK;
}

int emb_memset_device(emb_engine *e, void *dst_device, int value, size_t bytes) {
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    if (!bytes) return EMB_OK;
    DeviceGuard g(e->device);
    HIP_TRY(hipMemset(dst_device, value, bytes));
    return EMB_OK;
}

int emb_stream_create(emb_engine *e, void **stream) {
    if (!e || !stream) return fail(EMB_ERR_INVALID, "engine or stream is NULL");
    DeviceGuard g(e->device);
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *stream = st;
    return EMB_OK;
}

int emb_stream_destroy(emb_engine *e, void *stream) {
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    if (!stream) return EMB_OK;
    DeviceGuard g(e->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // Launch-image segments still open on this stream would later be closed with an event recorded ON it: drain the stream
    // and retire them now, so no ring ever touches the handle again (take_image_space's "the caller destroyed that stream"
    // branch remains for streams the caller made and destroyed with the runtime directly).
    bool drained = false;
    for (int rk = 0; rk < kRingPool; rk++) {
        std::lock_guard<std::mutex> lk(e->ring_mu[rk]);
        for (DescSlot &sl : e->ring[rk].slots)
            if (sl.stream == st && sl.used && !sl.pending) {
                if (!drained) HIP_TRY(hipStreamSynchronize(st));
                drained = true;
                sl.used = 0;
                sl.stream = nullptr;
            }
    }
    HIP_TRY(hipStreamDestroy(st));
    return EMB_OK;
}

int emb_synchronize(emb_engine *e, void *stream) {
    if (!e) return fail(EMB_ERR_INVALID, "engine is NULL");
    DeviceGuard g(e->device);
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return EMB_OK;
}

int emb_device_of(emb_engine *e, int32_t *device) {
    if (!e || !device) return fail(EMB_ERR_INVALID, "engine or device is NULL");
    *device = e->device;
    return EMB_OK;
}

// ---- request queue: R pending small lookups -> ONE launch (see pimemb.h) ---------------------------------------------------
}  // extern "C"

namespace {

constexpr int kQueueGens = 4;              // flushes whose staging / bookkeeping is alive at once
constexpr size_t kQueueBlock = 1u << 20;   // pinned staging is handed out from 1-MiB blocks (never moved: descriptors point into them)

struct QueueRequest {
    uint32_t first_desc = 0, n_descs = 0;
    std::vector<pimemb::CopyPiece> out;     // host queues: staging -> caller's buffers, done by emb_queue_wait
    bool collected = false;                 // emb_queue_wait has copied its rows out
};

struct QueueGen {
    uint64_t first_ticket = 0, flush_no = 0;
    std::vector<DevDesc> descs;
    std::vector<QueueRequest> reqs;
    uint32_t max_tiles = 0;
    uint64_t bags = 0, idx = 0;
    std::vector<char *> blocks;             // pinned staging of host queues
    size_t block_at = 0, block_used = 0;
    hipStream_t stream = nullptr;           // the stream its flush went to
    bool in_flight = false;
    uint32_t collected = 0;                 // host queues: requests whose rows have been copied out (emb_queue_wait)
};

}  // namespace

struct emb_queue {
    emb_engine *e = nullptr;
    emb_index_type itype = EMB_IDX_U32;
    emb_memspace space = EMB_MEM_DEVICE;
    std::mutex mu;
    std::condition_variable cv;             // a host queue's generation is recycled only when all its requests were collected
    QueueGen gen[kQueueGens];
    int open = 0;
    uint64_t next_ticket = 0, n_flushes = 0;
    ImageRing ring;                         // the launches' descriptor images: ONE event per 256-KiB segment, not per flush
    // host queues: done[g] = number of the last flush of generation g whose rows are in its staging (a one-thread kernel
    // behind the lookup stores it: no event -- an event between two kernels costs GPU time -- and waiters poll a word)
    volatile unsigned long long *done = nullptr;
    bool shaped = false;
    int dtype = EMB_F32;            // (an emb_dtype value, held as int: pimemb_internal.h, dtype_value)
    uint32_t dim = 0;
    LaunchGeom geom{};
    KernelKind kind = pimemb::KERNEL_GROUP;
    uint32_t bpt = 1;
};

namespace {

// `bytes` of the open generation's pinned staging, 16-byte aligned (host queues).  Blocks are kept for later flushes.
char *queue_stage(QueueGen &g, size_t bytes, int device) {
    bytes = (bytes + 15) / 16 * 16;
    if (bytes > kQueueBlock) return nullptr;
    if (g.block_at < g.blocks.size() && g.block_used + bytes > kQueueBlock) {
        g.block_at++;
        g.block_used = 0;
    }
    if (g.block_at >= g.blocks.size()) {
        void *p = nullptr;
        DeviceGuard dg(device);      // (a client thread's current device need not be the engine's: the block is mapped for THAT GPU)
        if (hipHostMalloc(&p, kQueueBlock, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return nullptr;
        g.blocks.push_back(static_cast<char *>(p));
        g.block_used = 0;
    }
    char *r = g.blocks[g.block_at] + g.block_used;
    g.block_used += bytes;
    return r;
}

// One request into the open generation (caller holds q->mu).
int queue_add_locked(emb_queue *q, const emb_lookup_desc *descs, uint32_t n_descs, uint64_t *ticket) {
    emb_engine *e = q->e;
    const size_t isz = index_size(q->itype);
    QueueGen &g = q->gen[q->open];
    const size_t first = g.descs.size();
    if (first + n_descs > 65535u) return fail(EMB_ERR_UNSUPPORTED, "emb_queue_add: more than 65535 descriptors pending: flush first");
    QueueRequest rq;
    rq.first_desc = (uint32_t)first;
    rq.n_descs = n_descs;
    const size_t block_at0 = g.block_at, block_used0 = g.block_used;
    auto undo = [&]() {
        g.descs.resize(first);
        g.block_at = block_at0;
        g.block_used = block_used0;
    };
    uint64_t bags = 0, idx = 0;
    uint32_t max_tiles = g.max_tiles;
    for (uint32_t i = 0; i < n_descs; i++) {
        const emb_lookup_desc &u = descs[i];
        if (u.table_id >= e->tables.size() || e->tables[u.table_id].rows == nullptr) {
            undo();
            return fail(EMB_ERR_INVALID, "emb_queue_add: desc %u: table %u is not loaded", i, u.table_id);
        }
        const Table &t = e->tables[u.table_id];
        if (!q->shaped) {            // the first request fixes the queue's row shape (and with it the kernel)
            q->shaped = true;
            q->dtype = t.dtype;
            q->dim = t.dim;
            q->geom = t.geom;
            q->kind = t.geom.scalar_lanes ? pimemb::KERNEL_ANYDIM : pimemb::KERNEL_GROUP;
            q->bpt = pimemb::bags_per_tile(q->kind, q->geom);
        } else if (t.dtype != q->dtype || t.dim != q->dim) {
            undo();
            return fail(EMB_ERR_UNSUPPORTED, "emb_queue_add: desc %u: table %u is dim %u / dtype %d, the queue serves dim %u / dtype %d "
                        "(one row shape per queue)", i, u.table_id, t.dim, (int)t.dtype, q->dim, (int)q->dtype);
        }
        if ((u.n_bags > 0 && !u.pooled) || (u.n_indices > 0 && !u.indices) ||
            (!u.offsets && ((u.n_bags > 0 && u.fixed_pooling == 0) || (uint64_t)u.fixed_pooling * u.n_bags != u.n_indices))) {
            undo();
            return fail(EMB_ERR_INVALID, "emb_queue_add: desc %u: bad buffers (NULL pointer, or offsets NULL and fixed_pooling*n_bags != n_indices)", i);
        }
        DevDesc d{};
        d.weights = t.rows;
        d.indices = u.indices;
        d.offsets = u.offsets;
        d.out = u.pooled;
        d.n_idx = u.n_indices;
        d.n_bags = u.n_bags;
        d.nr_rows = t.nr_rows;
        d.fixed_pooling = u.offsets ? 0u : u.fixed_pooling;
        const uint64_t tiles = (u.n_bags + q->bpt - 1) / q->bpt;
        if (tiles > 0x0fffffffull) {
            undo();
            return fail(EMB_ERR_UNSUPPORTED, "emb_queue_add: desc %u: too many bags for a queued request", i);
        }
        d.n_tiles = (uint32_t)tiles;
        if (q->space == EMB_MEM_HOST) {       // stage the inputs now; the rows come back through the same pinned memory
            const size_t ib = u.n_indices * isz, ob = u.offsets ? u.n_bags * isz : 0, rb = u.n_bags * (size_t)t.dim * 4;
            const int dev = q->e->device;
            char *pi = ib ? queue_stage(g, ib, dev) : nullptr, *po = ob ? queue_stage(g, ob, dev) : nullptr, *pr = rb ? queue_stage(g, rb, dev) : nullptr;
            if ((ib && !pi) || (ob && !po) || (rb && !pr)) {
                undo();
                return fail(EMB_ERR_UNSUPPORTED, "emb_queue_add: desc %u: a buffer of more than 1 MiB -- not a small request: use emb_lookup_batched", i);
            }
            if (ib) memcpy(pi, u.indices, ib);
            if (ob) memcpy(po, u.offsets, ob);
            d.indices = pi;
            d.offsets = po;
            d.out = reinterpret_cast<float *>(pr);
            if (rb) rq.out.push_back({u.pooled, pr, rb});
        }
        if (d.n_tiles > max_tiles) max_tiles = d.n_tiles;
        g.descs.push_back(d);
        bags += u.n_bags;
        idx += u.n_indices;
    }
    if (g.reqs.empty()) g.first_ticket = q->next_ticket;
    g.reqs.push_back(std::move(rq));
    g.max_tiles = max_tiles;
    g.bags += bags;
    g.idx += idx;
    if (ticket) *ticket = q->next_ticket;
    q->next_ticket++;
    return EMB_OK;
}

}  // namespace

namespace pimemb {
hipError_t launch_store_word(volatile unsigned long long *dst, unsigned long long value, hipStream_t stream);   // pimemb_kernels.hip
}

extern "C" {

int emb_queue_create(emb_engine *e, emb_index_type itype, emb_memspace space, emb_queue **out) {
    if (!e || !out) return fail(EMB_ERR_INVALID, "emb_queue_create: NULL argument");
    *out = nullptr;
    if (itype != EMB_IDX_U32 && itype != EMB_IDX_I64) return fail(EMB_ERR_INVALID, "emb_queue_create: bad index type");
    emb_queue *q = new (std::nothrow) emb_queue();
    if (!q) return fail(EMB_ERR_NOMEM, "out of host memory");
    q->e = e;
    q->itype = itype;
    q->space = space;
    q->ring.desc_mode = 1;
    q->ring.slot_flags = hipHostMallocMapped | hipHostMallocCoherent;
    DeviceGuard g(e->device);
    e->live_plans.fetch_add(1);      // (the engine must outlive its queues, like its plans)
    void *p = nullptr;
    if (hipHostMalloc(&p, 64 * kQueueGens, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
        (void)emb_queue_destroy(q);
        return fail(EMB_ERR_NOMEM, "emb_queue_create: pinned memory");
    }
    q->done = static_cast<volatile unsigned long long *>(p);
    for (int k = 0; k < kQueueGens; k++) q->done[8 * k] = 0;
    *out = q;
    return EMB_OK;
}

int emb_queue_add(emb_queue *q, const emb_lookup_desc *descs, uint32_t n_descs, uint64_t *ticket) {
    if (!q || !descs || n_descs == 0) return fail(EMB_ERR_INVALID, "emb_queue_add: NULL argument or empty request");
    std::lock_guard<std::mutex> lk(q->mu);
    return queue_add_locked(q, descs, n_descs, ticket);
}

int emb_queue_add_many(emb_queue *q, const emb_lookup_desc *descs, const uint32_t *n_descs, uint32_t n_requests, uint64_t *first_ticket) {
    if (!q || !descs || !n_descs || n_requests == 0) return fail(EMB_ERR_INVALID, "emb_queue_add_many: NULL argument or no request");
    std::lock_guard<std::mutex> lk(q->mu);
    size_t at = 0;
    for (uint32_t r = 0; r < n_requests; r++) {
        if (n_descs[r] == 0) return fail(EMB_ERR_INVALID, "emb_queue_add_many: request %u is empty", r);
        uint64_t t = 0;
        const int rc = queue_add_locked(q, descs + at, n_descs[r], &t);
        if (rc) return rc;            // requests 0 .. r-1 stay queued (their tickets: *first_ticket .. *first_ticket + r - 1)
        if (r == 0 && first_ticket) *first_ticket = t;
        at += n_descs[r];
    }
    return EMB_OK;
}

int emb_queue_flush(emb_queue *q, void *stream, uint32_t *n_requests) {
    if (!q) return fail(EMB_ERR_INVALID, "emb_queue_flush: queue is NULL");
    if (n_requests) *n_requests = 0;
    emb_engine *e = q->e;
    DeviceGuard dg(e->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::unique_lock<std::mutex> lk(q->mu);
    QueueGen &g = q->gen[q->open];
    if (g.reqs.empty()) return EMB_OK;
    // The generation this flush will open next still holds, in a host queue's staging, the rows of the requests flushed four
    // flushes ago until their waiters have copied them out: it is recycled only then.  A front end that flushes faster than
    // its clients collect is held back HERE, before anything of this flush is launched (requests that arrive meanwhile
    // still join it), instead of overwriting rows.
    const int next = (q->open + 1) % kQueueGens;
    QueueGen &nx = q->gen[next];
    if (nx.in_flight && q->space == EMB_MEM_HOST &&
        !q->cv.wait_for(lk, std::chrono::seconds(30), [&] { return nx.collected >= nx.reqs.size(); }))
        return fail(EMB_ERR_INVALID, "emb_queue_flush: %zu request(s) of flush %llu were never waited for (emb_queue_wait): their staging "
                    "cannot be reused", nx.reqs.size() - nx.collected, (unsigned long long)nx.flush_no);
    // requests were tiled for the lane-group kernel as they came in; a flush that adds up to a big one-hot launch runs the
    // wave-batch kernel instead (choose_kernel's rule for any launch): its tiles are larger, so the counts are redone
    KernelKind kind = q->kind;
    uint32_t max_tiles = g.max_tiles;
    if (kind == pimemb::KERNEL_GROUP) {
        kind = q->dtype == pimemb::kMXFP4 ? pimemb::KERNEL_GROUP : pimemb::choose_kernel(g.bags, g.idx, q->geom);   // (MXFP4: lane-group only)
        if (kind != pimemb::KERNEL_GROUP) {
            const uint32_t bpt = pimemb::bags_per_tile(kind, q->geom);
            max_tiles = 0;
            for (DevDesc &dd : g.descs) {
                dd.n_tiles = (uint32_t)((dd.n_bags + bpt - 1) / bpt);
                if (dd.n_tiles > max_tiles) max_tiles = dd.n_tiles;
            }
        }
    }
    const size_t bytes = g.descs.size() * sizeof(DevDesc);
    char *h = nullptr, *d = nullptr;
    int rc = take_image_space(q->ring, bytes, s, &h, &d);
    if (rc) return rc;
    memcpy(h, g.descs.data(), bytes);
    if (max_tiles)
        HIP_TRY(pimemb::launch_bag_sum(reinterpret_cast<const DevDesc *>(h), (uint32_t)g.descs.size(), max_tiles, q->dtype,
                                       q->itype, q->geom, kind, nullptr, 0, false, s));
    g.flush_no = ++q->n_flushes;
    g.stream = s;
    g.in_flight = true;
    if (q->space == EMB_MEM_HOST)      // waiters poll this word; device queues are complete in stream order and need nothing
        HIP_TRY(pimemb::launch_store_word(q->done + 8 * q->open, g.flush_no, s));
    e->n_lookup_calls.fetch_add(g.reqs.size(), std::memory_order_relaxed);
    e->n_kernel_launches.fetch_add(1, std::memory_order_relaxed);
    e->n_by_kind[kind].fetch_add(1, std::memory_order_relaxed);
    e->n_bags.fetch_add(g.bags, std::memory_order_relaxed);
    e->n_indices.fetch_add(g.idx, std::memory_order_relaxed);
    if (n_requests) *n_requests = (uint32_t)g.reqs.size();
    // open the next generation (its previous occupants were collected: checked before this flush launched anything)
    q->open = next;
    nx.in_flight = false;
    nx.collected = 0;
    nx.descs.clear();
    nx.reqs.clear();
    nx.max_tiles = 0;
    nx.bags = nx.idx = 0;
    nx.block_at = nx.block_used = 0;
    nx.first_ticket = q->next_ticket;
    return EMB_OK;
}

int emb_queue_wait(emb_queue *q, uint64_t ticket) {
    if (!q) return fail(EMB_ERR_INVALID, "emb_queue_wait: queue is NULL");
    std::vector<pimemb::CopyPiece> out;
    volatile unsigned long long *w = nullptr;
    uint64_t flush_no = 0;
    hipStream_t stream = nullptr;
    int gen_at = -1;
    {
        std::lock_guard<std::mutex> lk(q->mu);
        if (ticket >= q->next_ticket) return fail(EMB_ERR_INVALID, "emb_queue_wait: ticket %llu was never handed out", (unsigned long long)ticket);
        int at = -1;
        for (int k = 0; k < kQueueGens; k++) {
            QueueGen &c = q->gen[k];
            if (!c.reqs.empty() && ticket >= c.first_ticket && ticket < c.first_ticket + c.reqs.size()) at = k;
        }
        if (at < 0) return fail(EMB_ERR_INVALID, "emb_queue_wait: request %llu is no longer tracked (wait before the fourth flush after its own)", (unsigned long long)ticket);
        if (at == q->open) return fail(EMB_ERR_INVALID, "emb_queue_wait: request %llu has not been flushed yet", (unsigned long long)ticket);
        QueueGen &g = q->gen[at];
        if (g.reqs[ticket - g.first_ticket].collected) return EMB_OK;      // (waited for before)
        out = g.reqs[ticket - g.first_ticket].out;
        w = q->done + 8 * at;
        flush_no = g.flush_no;
        stream = g.stream;
        gen_at = at;
    }
    DeviceGuard dg(q->e->device);
    if (q->space == EMB_MEM_HOST) {
        const double t0 = now_us();
        for (uint64_t spin = 0; *w < flush_no; spin++)
            if ((spin & 0xffff) == 0xffff && now_us() - t0 > 30e6) return fail(EMB_ERR_DEVICE, "emb_queue_wait: flush %llu did not finish within 30 s", (unsigned long long)flush_no);
        for (const pimemb::CopyPiece &c : out) memcpy(c.dst, c.src, c.bytes);
    } else {
        HIP_TRY(hipStreamSynchronize(stream));      // (device queues: results are complete in stream order; this is the blunt form)
    }
    {       // the generation cannot have been recycled meanwhile: it still held this uncollected request
        std::lock_guard<std::mutex> lk(q->mu);
        QueueGen &g = q->gen[gen_at];
        QueueRequest &r = g.reqs[ticket - g.first_ticket];
        if (!r.collected) {
            r.collected = true;
            if (++g.collected >= g.reqs.size()) q->cv.notify_all();
        }
    }
    return EMB_OK;
}

int emb_queue_destroy(emb_queue *q) {
    if (!q) return EMB_OK;
    DeviceGuard dg(q->e->device);
    for (QueueGen &g : q->gen)
        if (g.in_flight) (void)hipStreamSynchronize(g.stream);
    (void)hipGetLastError();
    for (QueueGen &g : q->gen)
        for (char *b : g.blocks) (void)hipHostFree(b);
    q->ring.release();
    if (q->done) (void)hipHostFree(const_cast<unsigned long long *>(q->done));
    q->e->live_plans.fetch_sub(1);
    delete q;
    return EMB_OK;
}

int emb_route_bags_sizes(uint32_t n_tables, uint64_t n_bags, uint64_t total_indices, uint32_t n_shards,
                         uint64_t *send_bytes, uint64_t *meta_bytes, uint64_t *slots_bytes, uint64_t *work_bytes) {
    if (n_tables == 0 || n_tables > pimemb::kRouteBagMaxTables || n_shards == 0 || n_shards > 255)
        return fail(EMB_ERR_INVALID, "emb_route_bags_sizes: 1..64 tables and 1..255 shards");
    const uint64_t nk = (uint64_t)n_tables * n_shards;
    // every index once, at most min(indices, bags x shards) sub-bag offsets, < 4 padding words per array
    const uint64_t sub_max = std::min<uint64_t>(total_indices, n_bags * nk);
    if (send_bytes) *send_bytes = (total_indices + sub_max + 8 * nk + 4) * 4;
    if (meta_bytes) *meta_bytes = ((uint64_t)pimemb::route_bags_meta_words(n_tables, n_shards) + 3) / 4 * 16;
    if (slots_bytes) *slots_bytes = (nk * n_bags + 3) / 4 * 16;
    if (work_bytes) *work_bytes = (nk * n_bags + 3) / 4 * 16;
    return EMB_OK;
}

int emb_route_bags(emb_engine *e, const emb_route_table *tables, uint32_t n_tables, uint64_t n_bags,
                   uint32_t n_shards, void *send, uint32_t *meta, uint32_t *slots, void *work, void *stream) {
    return emb_route_bags_typed(e, tables, n_tables, EMB_IDX_U32, n_bags, n_shards, send, meta, slots, work, stream);
}

int emb_route_bags_typed(emb_engine *e, const emb_route_table *tables, uint32_t n_tables, emb_index_type itype, uint64_t n_bags,
                         uint32_t n_shards, void *send, uint32_t *meta, uint32_t *slots, void *work, void *stream) {
    if (!e || !tables || !send || !meta || !slots || !work) return fail(EMB_ERR_INVALID, "emb_route_bags: NULL argument");
    if (itype != EMB_IDX_U32 && itype != EMB_IDX_I64) return fail(EMB_ERR_INVALID, "emb_route_bags: bad index type");
    if (n_tables == 0 || n_tables > pimemb::kRouteBagMaxTables)
        return fail(EMB_ERR_UNSUPPORTED, "emb_route_bags: 1..%u tables per call", pimemb::kRouteBagMaxTables);
    if (n_shards == 0 || n_shards > 255 || n_bags == 0 || n_bags * n_shards > 0x7fffffffull * 256)
        return fail(EMB_ERR_INVALID, "emb_route_bags: n_shards must be 1..255 and n_bags > 0");
    pimemb::RouteBagDesc d[pimemb::kRouteBagMaxTables];
    uint64_t words = 8ull * n_tables * n_shards + 4;     // word offsets inside `send` are 32-bit
    for (uint32_t k = 0; k < n_tables; k++) {
        const emb_route_table &t = tables[k];
        words += t.n_indices + std::min<uint64_t>(t.n_indices, n_bags * n_shards);
        if (t.rows_per_shard == 0) return fail(EMB_ERR_INVALID, "emb_route_bags: tables[%u].rows_per_shard is 0", k);
        if (t.n_indices && !t.indices) return fail(EMB_ERR_INVALID, "emb_route_bags: tables[%u].indices is NULL", k);
        if (t.n_indices > 0xffffffffull) return fail(EMB_ERR_UNSUPPORTED, "emb_route_bags: tables[%u]: more than 2^32-1 indices", k);
        if (!t.offsets && (uint64_t)t.fixed_pooling * n_bags != t.n_indices)
            return fail(EMB_ERR_INVALID, "emb_route_bags: tables[%u]: fixed_pooling*n_bags != n_indices", k);
        d[k] = pimemb::RouteBagDesc{t.indices, t.offsets, t.n_indices, t.fixed_pooling, t.rows_per_shard};
    }
    if (words > 0xffffffffull)
        return fail(EMB_ERR_UNSUPPORTED, "emb_route_bags: %llu request words in one call (limit 2^32-1): route fewer tables per call",
                    (unsigned long long)words);
    DeviceGuard g(e->device);
    HIP_TRY(pimemb::launch_route_bags(d, n_tables, n_bags, n_shards, static_cast<uint32_t *>(send), meta, slots,
                                      static_cast<uint32_t *>(work), static_cast<hipStream_t>(stream), itype == EMB_IDX_I64));
    return EMB_OK;
}

int emb_route_exchange_sizes(const uint32_t *sent, const uint32_t *received, uint32_t n_tables, uint32_t n_shards,
                             uint32_t dim, uint64_t *req_out_words, uint64_t *req_in_words, uint64_t *ret_rows_back,
                             uint64_t *ret_rows_served, uint64_t *peak_req_bytes, uint64_t *peak_ret_bytes) {
    if (!sent || !received || !req_out_words || !req_in_words || !ret_rows_back || !ret_rows_served)
        return fail(EMB_ERR_INVALID, "emb_route_exchange_sizes: NULL argument");
    if (n_tables == 0 || n_tables > pimemb::kRouteBagMaxTables || n_shards == 0 || n_shards > 255)
        return fail(EMB_ERR_INVALID, "emb_route_exchange_sizes: 1..64 tables and 1..255 shards");
    auto pad4 = [](uint64_t v) { return (v + 3u) & ~(uint64_t)3u; };
    const uint32_t stride = 2 * (n_tables + 1);          // one [K+1][2] block per peer
    uint64_t peak_w = 0, peak_r = 0;
    for (uint32_t p = 0; p < n_shards; p++) {
        const uint32_t *so = sent + (size_t)p * stride, *ri = received + (size_t)p * stride;
        uint64_t wo = 0, wi = 0, rb = 0, rs = 0;
        for (uint32_t k = 0; k < n_tables; k++) {
            wo += pad4(so[2 * k]) + pad4(so[2 * k + 1]);
            wi += pad4(ri[2 * k]) + pad4(ri[2 * k + 1]);
            rb += so[2 * k];
            rs += ri[2 * k];
        }
        req_out_words[p] = wo;
        req_in_words[p] = wi;
        ret_rows_back[p] = rb;
        ret_rows_served[p] = rs;
        peak_w = std::max<uint64_t>(peak_w, ri[2 * n_tables]);         // every sender's own largest piece
        peak_r = std::max<uint64_t>(peak_r, ri[2 * n_tables + 1]);
    }
    if (peak_req_bytes) *peak_req_bytes = peak_w * 4;
    if (peak_ret_bytes) *peak_ret_bytes = peak_r * (uint64_t)dim * 4;
    return EMB_OK;
}

int emb_route_serve_descs(const uint32_t *received, uint32_t n_tables, uint32_t n_shards, uint32_t dim,
                          const uint32_t *shard_table_ids, const void *req_recv, float *ret_send,
                          emb_lookup_desc *descs, uint32_t *n_descs, uint64_t *algorithmic_bytes) {
    if (!received || !shard_table_ids || !descs || !n_descs)
        return fail(EMB_ERR_INVALID, "emb_route_serve_descs: NULL argument");
    if (n_tables == 0 || n_tables > pimemb::kRouteBagMaxTables || n_shards == 0 || n_shards > 255 || dim == 0)
        return fail(EMB_ERR_INVALID, "emb_route_serve_descs: 1..64 tables, 1..255 shards, dim > 0");
    auto pad4 = [](uint64_t v) { return (v + 3u) & ~(uint64_t)3u; };
    const uint32_t *words = static_cast<const uint32_t *>(req_recv);
    const uint32_t stride = 2 * (n_tables + 1);
    uint64_t start = 0, row0 = 0, bytes = 0;
    uint32_t n = 0;
    for (uint32_t s = 0; s < n_shards; s++)
        for (uint32_t k = 0; k < n_tables; k++) {
            const uint64_t ns = received[(size_t)s * stride + 2 * k], ni = received[(size_t)s * stride + 2 * k + 1];
            if (ns) {
                if (!req_recv || !ret_send) return fail(EMB_ERR_INVALID, "emb_route_serve_descs: NULL buffer");
                emb_lookup_desc &d = descs[n++];
                d.table_id = shard_table_ids[k];
                d.fixed_pooling = 0;
                d.offsets = words + start;
                d.indices = words + start + pad4(ns);
                d.n_indices = ni;
                d.n_bags = ns;
                d.pooled = ret_send + row0 * dim;
                bytes += ni * ((uint64_t)dim * 4 + 4) + ns * (4 + (uint64_t)dim * 4);
            }
            start += pad4(ns) + pad4(ni);
            row0 += ns;
        }
    *n_descs = n;
    if (algorithmic_bytes) *algorithmic_bytes = bytes;
    return EMB_OK;
}

int emb_unroute_bags(emb_engine *e, const float *recv, const uint32_t *meta, const uint32_t *slots,
                     uint32_t n_tables, uint64_t n_bags, uint32_t n_shards, uint32_t dim, float *pooled,
                     void *stream) {
    if (!e || !recv || !meta || !slots || !pooled) return fail(EMB_ERR_INVALID, "emb_unroute_bags: NULL argument");
    if (dim == 0 || dim % 4) return fail(EMB_ERR_UNSUPPORTED, "emb_unroute_bags: dim must be a multiple of 4");
    if (n_tables == 0 || n_tables > pimemb::kRouteBagMaxTables || n_shards == 0 || n_shards > 255)
        return fail(EMB_ERR_INVALID, "emb_unroute_bags: 1..64 tables and 1..255 shards");
    DeviceGuard g(e->device);
    HIP_TRY(pimemb::launch_unroute_bags(recv, meta, slots, n_tables, n_bags, n_shards, dim, pooled,
                                        static_cast<hipStream_t>(stream)));
    return EMB_OK;
}

}  // extern "C"
