// pimemb_rows.hip -- libpimemb_rows.so: in-place row updates of a served table (include/pimemb_rows.h).
//
// A companion of libpimemb.so with a code object of its own: the kernels below are linked into no other library, and tables
// are reached through the public ABI of pimemb.h alone (emb_table_info hands out the HBM address the kernels store to).
//
// Three kernels write, one pair prepares:
//   rows_write_group    rows of 16-byte multiples (up to 1 KiB; encoded MXFP4 rows of any stride): one row per lane group, a
//                       lane encodes and stores 16 bytes at a time -- the mirror image of the lane-group lookup kernels' loads
//   rows_write_mx       fp32 -> MXFP4: four lanes per 32-element block (eight elements = one 32-bit word of nibbles each), amax
//                       and the all-zero test by cross-lane shuffles, the block's 16 element bytes and the row's scale bytes +
//                       zero padding gathered into single lanes and stored as 16-byte vectors; nothing goes through LDS
//   rows_write_elem     any other width: one thread per element
//   rows_claim / rows_claim_mx   the duplicate pre-pass: every good position p claims its id's slot of an open-addressing hash
//                       (key by CAS) and bids for it with atomicMax(p + 1); a write kernel stores position p only if it holds
//                       its id's slot.  The MXFP4 flavour reads the source row first: a row with an inf or a NaN is bad, and a
//                       bad row must not beat an earlier good one.
//   rows_claim_clear    empties the hash before the claims
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <mutex>

#include "pimemb_rows.h"
#include "pimemb_rows_encode.h"

namespace {

using namespace pimemb_rows;

constexpr int kF32 = 0, kF16 = 1, kFixed32 = 2, kBF16 = 3, kE4M3 = 8, kE5M2 = 9, kMXFP4 = 10;
constexpr uint32_t kBlock = 256;
enum Mode : uint32_t { MODE_COPY = 0, MODE_F16 = 1, MODE_BF16 = 2, MODE_E4M3 = 3, MODE_E5M2 = 4 };   // (fp32 -> fp32 is a copy)

struct u32x4 {
    uint32_t x, y, z, w;
} __attribute__((aligned(16)));

struct WriteArgs {
    char *table;                    // the table's rows in HBM
    uint64_t nr_rows;
    uint32_t dim;
    uint32_t stride;                // bytes from one table row to the next
    const void *ids;                // uint32[n] / int64[n]
    const char *src;                // source rows
    uint32_t src_stride;            // bytes from one source row to the next
    uint32_t n;
    const unsigned long long *keys; // id hash of the duplicate pre-pass (NULL: ids are unique by the caller's promise)
    const uint32_t *win;
    uint32_t hash_shift;            // 64 - log2(slots)
    uint32_t hash_mask;             // slots - 1
    unsigned long long *bad;        // rows skipped
};

template <bool IDX64>
__device__ inline bool load_id(const void *ids, uint32_t p, uint64_t nr_rows, uint64_t *id) {
    if (IDX64) {
        const long long v = static_cast<const long long *>(ids)[p];
        *id = (uint64_t)v;
        return v >= 0 && (uint64_t)v < nr_rows;      // compared at full width: 2^32 + 5 is not row 5
    }
    *id = static_cast<const uint32_t *>(ids)[p];
    return *id < nr_rows;
}

__device__ inline uint32_t hash_slot(uint64_t id, uint32_t shift) { return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> shift); }

// Does position p hold its id's slot?  (Its id was inserted by the pre-pass, so the probe ends at the key; an empty slot
// cannot come first, and ends the loop all the same.)
__device__ inline bool is_winner(const WriteArgs &a, uint64_t id, uint32_t p) {
    if (!a.keys) return true;
    uint32_t h = hash_slot(id, a.hash_shift);
    for (uint32_t probes = 0; probes <= a.hash_mask; probes++) {
        const unsigned long long k = a.keys[h];
        if (k == id + 1) return a.win[h] == p + 1;
        if (k == 0) return false;
        h = (h + 1) & a.hash_mask;
    }
    return false;
}

__device__ inline void claim(unsigned long long *keys, uint32_t *win, uint32_t shift, uint32_t mask, uint64_t id, uint32_t p) {
    uint32_t h = hash_slot(id, shift);
    for (uint32_t probes = 0; probes <= mask; probes++) {      // (at least two slots per position: an empty one is always found)
        const unsigned long long prev = atomicCAS(&keys[h], 0ull, (unsigned long long)(id + 1));
        if (prev == 0 || prev == id + 1) {
            atomicMax(&win[h], p + 1);
            return;
        }
        h = (h + 1) & mask;
    }
}

// Empties the hash before the claims: keys and bids are 12 bytes per slot, cleared 16 bytes per thread (slots is a power of two
// >= 64: at most 3 * 2^30 pieces).  A kernel and not hipMemsetAsync: in a captured graph the memset became a memset node, and
// replays of the graph wrote no row -- every position found its key gone and lost its bid (tests/test_gpu_train_loop.py replays
// a captured update).  A kernel node keeps its place in the chain.
__global__ __launch_bounds__(kBlock) void rows_claim_clear(uint4 *pieces, uint32_t n_pieces) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n_pieces) pieces[i] = make_uint4(0u, 0u, 0u, 0u);
}

template <bool IDX64>
__global__ __launch_bounds__(kBlock) void rows_claim(const void *ids, uint32_t n, uint64_t nr_rows, unsigned long long *keys,
                                                     uint32_t *win, uint32_t shift, uint32_t mask) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    uint64_t id;
    if (load_id<IDX64>(ids, (uint32_t)p, nr_rows, &id)) claim(keys, win, shift, mask, id, (uint32_t)p);
}

__device__ inline bool nonfinite4(const float4 &v) {
    return (f32_bits(v.x) & 0x7f800000u) == 0x7f800000u || (f32_bits(v.y) & 0x7f800000u) == 0x7f800000u ||
           (f32_bits(v.z) & 0x7f800000u) == 0x7f800000u || (f32_bits(v.w) & 0x7f800000u) == 0x7f800000u;
}

// 16 lanes per source row: an fp32 row with an inf or a NaN claims nothing.
template <bool IDX64>
__global__ __launch_bounds__(kBlock) void rows_claim_mx(const void *ids, const char *src, uint32_t src_stride, uint32_t dim, uint32_t n,
                                                        uint64_t nr_rows, unsigned long long *keys, uint32_t *win, uint32_t shift,
                                                        uint32_t mask) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t p = gid >> 4;
    const uint32_t lg = (uint32_t)gid & 15u;
    const bool live = p < n;
    int bad = 0;
    if (live) {
        const float4 *row = reinterpret_cast<const float4 *>(src + p * src_stride);
        for (uint32_t c = lg; c < dim / 4; c += 16) bad |= nonfinite4(row[c]);
    }
    bad |= __shfl_xor(bad, 1);
    bad |= __shfl_xor(bad, 2);
    bad |= __shfl_xor(bad, 4);
    bad |= __shfl_xor(bad, 8);
    uint64_t id;
    if (live && lg == 0 && !bad && load_id<IDX64>(ids, (uint32_t)p, nr_rows, &id)) claim(keys, win, shift, mask, id, (uint32_t)p);
}

__device__ inline uint32_t encode(uint32_t mode, uint32_t bits) {
    switch (mode) {
        case MODE_F16: return enc_f16(bits);
        case MODE_BF16: return enc_bf16(bits);
        case MODE_E4M3: return enc_e4m3(bits);
        default: return enc_e5m2(bits);
    }
}

// One row per group of `lanes` lanes (a power of two up to 64); lane c handles the row's 16-byte pieces c, c + lanes, ...
// (more than one only for encoded MXFP4 rows beyond 1 KiB).  A piece of the table takes 16 / 32 / 64 bytes of fp32 source.
template <bool IDX64>
__global__ __launch_bounds__(kBlock) void rows_write_group(WriteArgs a, uint32_t mode, uint32_t lanes, uint32_t lanes_log2, uint32_t chunks) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t p = gid >> lanes_log2;
    const uint32_t lg = (uint32_t)gid & (lanes - 1);
    if (p >= a.n || lg >= chunks) return;
    uint64_t id;
    if (!load_id<IDX64>(a.ids, (uint32_t)p, a.nr_rows, &id)) {
        if (lg == 0) atomicAdd(a.bad, 1ull);
        return;
    }
    if (!is_winner(a, id, (uint32_t)p)) return;
    u32x4 *dst = reinterpret_cast<u32x4 *>(a.table + id * a.stride);
    const char *srow = a.src + p * a.src_stride;
    for (uint32_t c = lg; c < chunks; c += lanes) {
        u32x4 o;
        if (mode == MODE_COPY) {
            o = reinterpret_cast<const u32x4 *>(srow)[c];
        } else if (mode == MODE_F16 || mode == MODE_BF16) {
            const u32x4 lo = reinterpret_cast<const u32x4 *>(srow)[2 * c], hi = reinterpret_cast<const u32x4 *>(srow)[2 * c + 1];
            o.x = encode(mode, lo.x) | (encode(mode, lo.y) << 16);
            o.y = encode(mode, lo.z) | (encode(mode, lo.w) << 16);
            o.z = encode(mode, hi.x) | (encode(mode, hi.y) << 16);
            o.w = encode(mode, hi.z) | (encode(mode, hi.w) << 16);
        } else {
            uint32_t w[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const u32x4 v = reinterpret_cast<const u32x4 *>(srow)[4 * c + j];
                w[j] = encode(mode, v.x) | (encode(mode, v.y) << 8) | (encode(mode, v.z) << 16) | (encode(mode, v.w) << 24);
            }
            o = u32x4{w[0], w[1], w[2], w[3]};
        }
        dst[c] = o;
    }
}

// One thread per element; esz = bytes of a table element.
template <bool IDX64>
__global__ __launch_bounds__(kBlock) void rows_write_elem(WriteArgs a, uint32_t mode, uint32_t esz) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t p = gid / a.dim;
    const uint32_t c = (uint32_t)(gid - p * a.dim);
    if (p >= a.n) return;
    uint64_t id;
    if (!load_id<IDX64>(a.ids, (uint32_t)p, a.nr_rows, &id)) {
        if (c == 0) atomicAdd(a.bad, 1ull);
        return;
    }
    if (!is_winner(a, id, (uint32_t)p)) return;
    char *drow = a.table + id * a.stride;
    const char *srow = a.src + p * a.src_stride;
    if (mode == MODE_COPY) {
        if (esz == 4) reinterpret_cast<uint32_t *>(drow)[c] = reinterpret_cast<const uint32_t *>(srow)[c];
        else if (esz == 2) reinterpret_cast<uint16_t *>(drow)[c] = reinterpret_cast<const uint16_t *>(srow)[c];
        else reinterpret_cast<uint8_t *>(drow)[c] = reinterpret_cast<const uint8_t *>(srow)[c];
        return;
    }
    const uint32_t v = encode(mode, reinterpret_cast<const uint32_t *>(srow)[c]);
    if (esz == 2) reinterpret_cast<uint16_t *>(drow)[c] = (uint16_t)v;
    else reinterpret_cast<uint8_t *>(drow)[c] = (uint8_t)v;
}

// fp32 -> MXFP4.  nb = dim / 32 blocks per row; a row's group is `lanes` = clamp(pow2ceil(4 nb), 4, 64) lanes and takes
// ceil(4 nb / lanes) <= 4 passes of lanes / 4 blocks each (dim <= 2048).  Everything a pass produces stays in registers until the
// whole row has been seen: a row with a non-finite value anywhere must not be written at all.
// Layout of what is stored (pimemb.h): piece b < nb = the 16 element bytes of block b; pieces nb .. = the nb scale bytes, then
// zeros up to the stride -- pass `it` of a 64-lane group produces scale bytes 16 it .. 16 it + 15, i.e. exactly tail piece `it`.
// Every lane of the wavefront runs every shuffle: rows past n, bad ids and lanes past the row only switch loads and stores off.
template <bool IDX64>
__global__ __launch_bounds__(kBlock) void rows_write_mx(WriteArgs a, uint32_t lanes, uint32_t lanes_log2, uint32_t passes) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t p = gid >> lanes_log2;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lg = lane & (lanes - 1), base = lane & ~(lanes - 1);
    const uint32_t nb = a.dim / 32u;
    const bool live = p < a.n;
    const char *srow = a.src + (live ? p : 0) * a.src_stride;
    u32x4 elems[4], tail[4];
    int bad_value = 0;
#pragma unroll
    for (uint32_t it = 0; it < 4; it++) {
        elems[it] = tail[it] = u32x4{0, 0, 0, 0};
        if (it < passes) {      // (uniform)
            const uint32_t b = it * (lanes / 4) + lg / 4;
            uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (live && b < nb) {
                const u32x4 *s = reinterpret_cast<const u32x4 *>(srow + ((size_t)b * 32 + (lg & 3u) * 8) * 4);
                const u32x4 lo = s[0], hi = s[1];
                v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
                v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
            }
            uint32_t amax = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t ab = v[j] & 0x7fffffffu;
                amax = ab > amax ? ab : amax;
            }
            bad_value |= amax >= 0x7f800000u;
            uint32_t o = (uint32_t)__shfl_xor((int)amax, 1);
            amax = o > amax ? o : amax;
            o = (uint32_t)__shfl_xor((int)amax, 2);
            amax = o > amax ? o : amax;                      // the block's amax, in all four of its lanes
            uint32_t s = mx_scale_of(amax);
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) word |= (mx_code_of(v[j] & 0x7fffffffu, s) | ((v[j] >> 28) & 8u)) << (4 * j);
            int zeros = (word & 0x77777777u) == 0;
            zeros &= __shfl_xor(zeros, 1);
            zeros &= __shfl_xor(zeros, 2);
            if (zeros) s = 127;
            if (b >= nb) s = 0;                                // lanes past the row contribute padding
            const uint32_t q = lane & ~3u;
            elems[it] = u32x4{(uint32_t)__shfl((int)word, (int)q), (uint32_t)__shfl((int)word, (int)q + 1),
                              (uint32_t)__shfl((int)word, (int)q + 2), (uint32_t)__shfl((int)word, (int)q + 3)};
            // scale bytes: lane lg < 4 of the group packs word lg of the pass's tail piece from the lanes that lead blocks 4 lg .. 4 lg + 3
            uint32_t tw = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t from = 16 * lg + 4 * j;
                const uint32_t sb = (uint32_t)__shfl((int)s, (int)(base + (from & (lanes - 1))));
                if (from < lanes) tw |= sb << (8 * j);
            }
            tail[it] = u32x4{(uint32_t)__shfl((int)tw, (int)base), (uint32_t)__shfl((int)tw, (int)base + 1),
                             (uint32_t)__shfl((int)tw, (int)base + 2), (uint32_t)__shfl((int)tw, (int)base + 3)};
        }
    }
    for (uint32_t off = 1; off < lanes; off <<= 1) bad_value |= __shfl_xor(bad_value, (int)off);     // (uniform trip count)
    if (!live) return;
    uint64_t id;
    const bool id_ok = load_id<IDX64>(a.ids, (uint32_t)p, a.nr_rows, &id);
    if (!id_ok || bad_value) {
        if (lg == 0) atomicAdd(a.bad, 1ull);
        return;
    }
    if (!is_winner(a, id, (uint32_t)p)) return;
    u32x4 *dst = reinterpret_cast<u32x4 *>(a.table + id * a.stride);
#pragma unroll
    for (uint32_t it = 0; it < 4; it++) {
        if (it < passes) {
            const uint32_t b = it * (lanes / 4) + lg / 4;
            if ((lg & 3u) == 0 && b < nb) dst[b] = elems[it];
            if (lg == 0 && it * 16 < nb) dst[nb + it] = tail[it];
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------

thread_local char t_err[512] = "";

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t_err, sizeof t_err, fmt, ap);
    va_end(ap);
    return code;
}
int fail_engine(int code, const char *what) { return fail(code, "%s: %s", what, emb_last_error()); }

#define ROWS_HIP(expr)                                                                          \
    do {                                                                                        \
        hipError_t err_ = (expr);                                                               \
        if (err_ != hipSuccess) return fail(EMB_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(err_)); \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

uint64_t pow2ceil(uint64_t v) {
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}
uint32_t log2of(uint64_t pow2) {
    uint32_t l = 0;
    while ((1ull << l) < pow2) l++;
    return l;
}
uint64_t slots_for(uint64_t n_rows) { return pow2ceil(n_rows * 2 < 64 ? 64 : n_rows * 2); }
constexpr uint64_t kCounterBytes = 256;
constexpr uint64_t kMaxRows = 0x7fffffffull;

}  // namespace

struct emb_rows {
    emb_engine *e = nullptr;
    int device = 0;
    uint64_t max_rows = 0;
    char *scratch = nullptr;               // [hash: slots * 12][counters: 256]; the hash of a call uses the first slots_for(n) * 12 bytes
    unsigned long long *counters = nullptr;   // [0] device-pointer calls since the last report, [1] the host-pointer call in flight
    char *stage = nullptr;                 // pinned, two halves
    char *stage_dev = nullptr;             // the same memory as the device addresses it
    uint64_t stage_bytes = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    std::mutex mu;
};

extern "C" {

const char *emb_rows_last_error(void) { return t_err; }

uint64_t emb_rows_scratch_bytes(uint64_t max_rows_per_call) {
    if (max_rows_per_call > kMaxRows) max_rows_per_call = kMaxRows;
    return slots_for(max_rows_per_call) * 12 + kCounterBytes;
}

uint64_t emb_rows_stage_bytes(uint64_t max_rows_per_call) {
    if (max_rows_per_call > kMaxRows) max_rows_per_call = kMaxRows;
    uint64_t b = max_rows_per_call * 520;
    if (b < (256ull << 10)) b = 256ull << 10;
    if (b > (64ull << 20)) b = 64ull << 20;
    return (b + 31) & ~31ull;
}

int emb_rows_create(emb_engine *e, uint64_t max_rows_per_call, emb_rows **out) {
    if (!e || !out) return fail(EMB_ERR_INVALID, "emb_rows_create: engine or out is NULL");
    if (max_rows_per_call == 0 || max_rows_per_call > kMaxRows)
        return fail(EMB_ERR_INVALID, "emb_rows_create: max_rows_per_call must be 1 .. 2^31 - 1");
    int32_t dev = 0;
    if (int rc = emb_device_of(e, &dev)) return fail_engine(rc, "emb_rows_create");
    emb_rows *w = new emb_rows;
    w->e = e;
    w->device = dev;
    w->max_rows = max_rows_per_call;
    DeviceGuard g(dev);
    const uint64_t bytes = emb_rows_scratch_bytes(max_rows_per_call);
    void *p = nullptr;
    if (int rc = emb_device_alloc(e, bytes, &p)) {
        delete w;
        return fail_engine(rc, "emb_rows_create");
    }
    w->scratch = static_cast<char *>(p);
    w->counters = reinterpret_cast<unsigned long long *>(w->scratch + bytes - kCounterBytes);
    w->stage_bytes = emb_rows_stage_bytes(max_rows_per_call);
    hipError_t err = hipMemset(w->counters, 0, kCounterBytes);
    if (err == hipSuccess) err = hipHostMalloc((void **)&w->stage, w->stage_bytes, hipHostMallocDefault);
    if (err == hipSuccess) err = hipHostGetDevicePointer((void **)&w->stage_dev, w->stage, 0);
    for (int i = 0; i < 2 && err == hipSuccess; i++) err = hipEventCreateWithFlags(&w->ev[i], hipEventDisableTiming);
    if (err != hipSuccess) {
        fail(EMB_ERR_DEVICE, "emb_rows_create: %s", hipGetErrorString(err));
        (void)emb_rows_destroy(w);
        return EMB_ERR_DEVICE;
    }
    *out = w;
    return EMB_OK;
}

int emb_rows_destroy(emb_rows *w) {
    if (!w) return EMB_OK;
    DeviceGuard g(w->device);
    (void)hipDeviceSynchronize();
    for (hipEvent_t ev : w->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (w->stage) (void)hipHostFree(w->stage);
    if (w->scratch) (void)emb_device_free(w->e, w->scratch);
    delete w;
    return EMB_OK;
}

}  // extern "C"

namespace {

struct TableShape {
    char *rows;
    uint64_t nr_rows;
    uint32_t dim;
    int dtype;
    uint32_t stride;       // bytes per table row
    uint32_t esz;          // bytes per element (0: MXFP4)
};

// hash clear, duplicate pre-pass and write kernel of one piece of at most max_rows rows: enqueues only.
int enqueue_piece(emb_rows *w, const TableShape &t, const void *ids, bool idx64, uint32_t n, const char *src, bool f32_src,
                  bool unique, unsigned long long *bad, hipStream_t s) {
    WriteArgs a{};
    a.table = t.rows;
    a.nr_rows = t.nr_rows;
    a.dim = t.dim;
    a.stride = t.stride;
    a.ids = ids;
    a.src = src;
    a.src_stride = f32_src ? t.dim * 4u : t.stride;
    a.n = n;
    a.bad = bad;
    const bool mx = t.dtype == kMXFP4 && f32_src;
    if (!unique) {
        const uint64_t slots = slots_for(n);
        unsigned long long *keys = reinterpret_cast<unsigned long long *>(w->scratch);
        uint32_t *win = reinterpret_cast<uint32_t *>(w->scratch + slots * 8);
        const uint32_t shift = 64 - log2of(slots), mask = (uint32_t)(slots - 1);
        const uint32_t pieces = (uint32_t)(slots * 12 / 16);
        rows_claim_clear<<<dim3((pieces + kBlock - 1) / kBlock), dim3(kBlock), 0, s>>>(reinterpret_cast<uint4 *>(w->scratch), pieces);
        if (mx) {
            const uint64_t blocks = ((uint64_t)n * 16 + kBlock - 1) / kBlock;
            if (idx64) rows_claim_mx<true><<<dim3((uint32_t)blocks), dim3(kBlock), 0, s>>>(ids, src, a.src_stride, t.dim, n, t.nr_rows, keys, win, shift, mask);
            else rows_claim_mx<false><<<dim3((uint32_t)blocks), dim3(kBlock), 0, s>>>(ids, src, a.src_stride, t.dim, n, t.nr_rows, keys, win, shift, mask);
        } else {
            const uint32_t blocks = (n + kBlock - 1) / kBlock;
            if (idx64) rows_claim<true><<<dim3(blocks), dim3(kBlock), 0, s>>>(ids, n, t.nr_rows, keys, win, shift, mask);
            else rows_claim<false><<<dim3(blocks), dim3(kBlock), 0, s>>>(ids, n, t.nr_rows, keys, win, shift, mask);
        }
        ROWS_HIP(hipGetLastError());
        a.keys = keys;
        a.win = win;
        a.hash_shift = shift;
        a.hash_mask = mask;
    }
    uint32_t mode = MODE_COPY;
    if (f32_src) mode = t.dtype == kF16 ? MODE_F16 : t.dtype == kBF16 ? MODE_BF16 : t.dtype == kE4M3 ? MODE_E4M3 : t.dtype == kE5M2 ? MODE_E5M2 : MODE_COPY;
    uint64_t blocks;
    if (mx) {
        const uint32_t nb = t.dim / 32u;
        uint32_t lanes = (uint32_t)pow2ceil(4ull * nb);
        lanes = lanes < 4 ? 4 : lanes > 64 ? 64 : lanes;
        const uint32_t passes = (4 * nb + lanes - 1) / lanes;
        if (passes > 4) return fail(EMB_ERR_UNSUPPORTED, "emb_rows_update: MXFP4 dim %u is beyond 2048", t.dim);
        blocks = ((uint64_t)n * lanes + kBlock - 1) / kBlock;
        if (idx64) rows_write_mx<true><<<dim3((uint32_t)blocks), dim3(kBlock), 0, s>>>(a, lanes, log2of(lanes), passes);
        else rows_write_mx<false><<<dim3((uint32_t)blocks), dim3(kBlock), 0, s>>>(a, lanes, log2of(lanes), passes);
    } else if (t.stride % 16 == 0 && (t.stride <= 1024 || t.dtype == kMXFP4)) {
        const uint32_t chunks = t.stride / 16;
        uint32_t lanes = (uint32_t)pow2ceil(chunks);
        lanes = lanes > 64 ? 64 : lanes;
        blocks = ((uint64_t)n * lanes + kBlock - 1) / kBlock;
        if (idx64) rows_write_group<true><<<dim3((uint32_t)blocks), dim3(kBlock), 0, s>>>(a, mode, lanes, log2of(lanes), chunks);
        else rows_write_group<false><<<dim3((uint32_t)blocks), dim3(kBlock), 0, s>>>(a, mode, lanes, log2of(lanes), chunks);
    } else {
        blocks = ((uint64_t)n * t.dim + kBlock - 1) / kBlock;
        if (blocks > 0x7fffffffull)
            return fail(EMB_ERR_UNSUPPORTED, "emb_rows_update: %u rows of dim %u are more elements than one launch of the element-wise kernel takes", n, t.dim);
        if (idx64) rows_write_elem<true><<<dim3((uint32_t)blocks), dim3(kBlock), 0, s>>>(a, mode, t.esz);
        else rows_write_elem<false><<<dim3((uint32_t)blocks), dim3(kBlock), 0, s>>>(a, mode, t.esz);
    }
    ROWS_HIP(hipGetLastError());
    return EMB_OK;
}

}  // namespace

extern "C" {

int emb_rows_update(emb_rows *w, uint32_t table_id, const void *row_ids, emb_index_type itype, uint64_t n_rows, const void *src,
                    emb_rows_src src_kind, emb_memspace space, uint32_t flags, void *stream, uint64_t *n_bad) {
    if (n_bad) *n_bad = 0;
    if (!w) return fail(EMB_ERR_INVALID, "emb_rows_update: writer is NULL");
    if (itype != EMB_IDX_U32 && itype != EMB_IDX_I64) return fail(EMB_ERR_INVALID, "emb_rows_update: bad index type");
    if (src_kind != EMB_ROWS_SRC_F32 && src_kind != EMB_ROWS_SRC_TABLE_DTYPE) return fail(EMB_ERR_INVALID, "emb_rows_update: bad source kind");
    if (space != EMB_MEM_HOST && space != EMB_MEM_DEVICE) return fail(EMB_ERR_INVALID, "emb_rows_update: bad memory space");
    if (flags & ~EMB_ROWS_UNIQUE_IDS) return fail(EMB_ERR_INVALID, "emb_rows_update: unknown flag bits 0x%x", flags & ~EMB_ROWS_UNIQUE_IDS);
    TableShape t{};
    void *rows = nullptr;
    emb_dtype dt;
    if (int rc = emb_table_info(w->e, table_id, &rows, &t.nr_rows, &t.dim, &dt)) return fail_engine(rc, "emb_rows_update");
    __builtin_memcpy(&t.dtype, &dt, sizeof(int));      // (the fp8 / MXFP4 values lie outside the enum's range: pimemb.h)
    t.rows = static_cast<char *>(rows);
    uint32_t n_hot = 0;
    if (int rc = emb_table_hot_count(w->e, table_id, &n_hot)) return fail_engine(rc, "emb_rows_update");
    if (n_hot)
        return fail(EMB_ERR_UNSUPPORTED,
                    "emb_rows_update: table %u has a hot set of %u rows staged, a copy taken when it was set that lookups would go on "
                    "serving: clear the set (emb_set_hot_rows with n_rows = 0), update, then set it again", table_id, n_hot);
    const bool f32_src = src_kind == EMB_ROWS_SRC_F32;
    if (f32_src && t.dtype == kFixed32)
        return fail(EMB_ERR_UNSUPPORTED, "emb_rows_update: table %u is EMB_FIXED32: a fixed-point table takes EMB_ROWS_SRC_TABLE_DTYPE rows only", table_id);
    t.esz = t.dtype == kMXFP4 ? 0u : (t.dtype == kF32 || t.dtype == kFixed32) ? 4u : (t.dtype == kF16 || t.dtype == kBF16) ? 2u : 1u;
    t.stride = t.dtype == kMXFP4 ? EMB_MXFP4_ROW_STRIDE(t.dim) : t.dim * t.esz;
    if (n_rows == 0) return EMB_OK;
    if (!row_ids || !src) return fail(EMB_ERR_INVALID, "emb_rows_update: row_ids or src is NULL");
    const bool idx64 = itype == EMB_IDX_I64, unique = (flags & EMB_ROWS_UNIQUE_IDS) != 0;
    const size_t isz = idx64 ? 8 : 4;
    const uint64_t src_row = f32_src ? (uint64_t)t.dim * 4 : t.stride;
    const bool vector_rows = t.dtype == kMXFP4 || (t.stride % 16 == 0 && t.stride <= 1024);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard g(w->device);
    if (space == EMB_MEM_DEVICE) {
        if (n_rows > w->max_rows)
            return fail(EMB_ERR_INVALID, "emb_rows_update: %llu rows in one device-pointer call, the writer was created for %llu",
                        (unsigned long long)n_rows, (unsigned long long)w->max_rows);
        if ((uintptr_t)src % (vector_rows ? 16 : 4) || (uintptr_t)row_ids % isz)
            return fail(EMB_ERR_INVALID, "emb_rows_update: src must be %d-byte aligned for this table, row_ids naturally aligned", vector_rows ? 16 : 4);
        return enqueue_piece(w, t, row_ids, idx64, (uint32_t)n_rows, static_cast<const char *>(src), f32_src, unique, &w->counters[0], s);
    }
    // host pointers: ids and rows through the two halves of the pinned buffer, which the kernels read in place
    std::lock_guard<std::mutex> lk(w->mu);
    const uint64_t half = w->stage_bytes / 2;
    const uint64_t per_row = src_row + isz;
    if (half < per_row + 32) return fail(EMB_ERR_UNSUPPORTED, "emb_rows_update: one source row of %llu bytes does not fit the writer's staging buffer", (unsigned long long)src_row);
    uint64_t chunk = (half - 32) / per_row;
    if (chunk > w->max_rows) chunk = w->max_rows;
    ROWS_HIP(hipMemsetAsync(&w->counters[1], 0, 8, s));
    int rc = EMB_OK;
    uint64_t k = 0;
    for (uint64_t at = 0; at < n_rows && rc == EMB_OK; at += chunk, k++) {
        const uint64_t n = n_rows - at < chunk ? n_rows - at : chunk;
        const int h = (int)(k & 1);
        if (k >= 2) ROWS_HIP(hipEventSynchronize(w->ev[h]));         // the kernels that read this half two chunks ago
        const uint64_t ids_at = (n * src_row + 15) & ~15ull;
        char *hb = w->stage + h * half;
        memcpy(hb, static_cast<const char *>(src) + at * src_row, n * src_row);
        memcpy(hb + ids_at, static_cast<const char *>(row_ids) + at * isz, n * isz);
        const char *db = w->stage_dev + h * half;
        rc = enqueue_piece(w, t, db + ids_at, idx64, (uint32_t)n, db, f32_src, unique, &w->counters[1], s);
        if (rc == EMB_OK) ROWS_HIP(hipEventRecord(w->ev[h], s));
    }
    unsigned long long bad = 0;
    hipError_t err = hipStreamSynchronize(s);
    if (err == hipSuccess) err = hipMemcpy(&bad, &w->counters[1], 8, hipMemcpyDeviceToHost);
    if (err != hipSuccess) return fail(EMB_ERR_DEVICE, "emb_rows_update: %s", hipGetErrorString(err));
    if (rc) return rc;
    if (n_bad) *n_bad = bad;
    if (bad)
        return fail(EMB_ERR_RANGE, "emb_rows_update: %llu of %llu rows were skipped (an id outside [0, %llu)%s); the others were written",
                    bad, (unsigned long long)n_rows, (unsigned long long)t.nr_rows, t.dtype == kMXFP4 && f32_src ? ", or an inf / NaN in an MXFP4 source row" : "");
    return EMB_OK;
}

int emb_rows_report(emb_rows *w, uint64_t *n_bad) {
    if (!w) return fail(EMB_ERR_INVALID, "emb_rows_report: writer is NULL");
    DeviceGuard g(w->device);
    unsigned long long bad = 0;
    ROWS_HIP(hipDeviceSynchronize());
    ROWS_HIP(hipMemcpy(&bad, &w->counters[0], 8, hipMemcpyDeviceToHost));
    ROWS_HIP(hipMemset(&w->counters[0], 0, 8));
    if (n_bad) *n_bad = bad;
    return EMB_OK;
}

}  // extern "C"
