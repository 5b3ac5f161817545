// pimemb_grad.hip -- libpimemb_grad.so: the EmbeddingBag backward pass over a served table (include/pimemb_grad.h).
//
// A companion of libpimemb.so with a code object of its own, like the row writer: the kernels below are linked into no other
// library, and tables are reached through the public ABI of pimemb.h alone.
//
// The pre-pass:
//   grad_classify       one thread per position: its bag (binary search in offsets), good / bad / padding, the sort key (the row
//                       id of a good position, nr_rows for every other one: they sort behind every row), cnt per bag for mean
//   grad_sort_count / grad_scan_chunks / grad_scan_sums / grad_sort_scatter
//                       a stable LSD radix sort of (key, position) pairs, 8 bits a pass: digit counts per tile of 1024
//                       positions, an exclusive scan over the [digit][tile] matrix in two levels, and a scatter that ranks
//                       the positions of a tile in their order (wavefront ballots, then counts per 64-position slice)
//   grad_scan_chunks<true>   the same scan over the run-head flags of the sorted keys: the number of every unique row
// The hot kernels (one instantiation per result: the sparse gradient, the SGD step, the Adagrad step, the row-wise Adagrad step):
//   grad_rows_group     one lane group per unique row, a lane owns 4 consecutive fp32 elements: walks the row's run in position
//                       order, the 16-byte loads of eight occurrences issued before the first add, the adds in order
//   grad_rows_elem      any other dim / alignment: one thread per element of a unique row (no row-wise Adagrad)
// The multi-table step (emb_grad_sgd_multi / emb_grad_step_multi: one pre-pass and one hot launch per group of up to 16 tables):
//   grad_multi_classify grad_classify over the concatenated positions of a group: a position finds its descriptor, then its bag,
//                       its class and its key = key_base[descriptor] + row id in that descriptor's terms
//   grad_multi_rows     grad_rows_group over the runs of the composite keys: a lane group finds its run's descriptor from the
//                       key and walks the run with that descriptor's pointers -- the same device functions, the same bits
// The segmented order (a context of EMB_GRAD_ORDER_SEGMENTED: a run longer than S is summed segment by segment, then over the segments):
//   grad_seg_partials / grad_seg_multi_partials     one lane group per sorted place, working where a segment of a long run starts:
//                       that segment's sum, stored into the context's partial buffer (csrc/pimemb_grad_segments.h numbers the slots)
//   grad_seg_rows_group / grad_seg_multi_rows / grad_seg_rows_elem     the hot kernels' twins: a long run is the sum of its partials
// The gradient of per_sample_weights (emb_grad_weights: no pre-pass, one launch per descriptor; csrc/pimemb_grad_dot.h):
//   grad_psw_group      one lane group per BAG, the forward's geometry: its piece of G[b] loaded once, the row gathers of eight
//                       positions in flight, products folded per piece and summed over the group by the row-wise xor butterfly
//   grad_psw_elem       any other dim / alignment: one lane group per position, scalar element loads, the same tree
// The stochastically rounded steps (emb_grad_sgd_sr / emb_grad_step_sr; csrc/pimemb_grad_sr.h; a code object of their own, libpimemb_grad_sr.so):
//   grad_sr_rows_group / grad_sr_rows_elem     the hot kernels' twins in both orders: the same walk, the last rounding by a Philox word
// The Adagrad tails (csrc/pimemb_grad_optim.h) end the same kernels; the row-wise one sums the row's squares over its lane group
// with an xor butterfly -- a fixed tree, stated over dim alone in the header: the same bits on every run.
// Every fp32 operation of the definition is a statement of its own under `fp contract(off)` (and the unit is compiled with
// -ffp-contract=off): nothing is fused into an FMA.
// The host side works in two phases.  The PLAN checks every descriptor of a call and lays out its launch chains (one per descriptor,
// or per group), refusing whatever cannot run; the ENQUEUE then runs chain after chain through one function and can fail on a
// HIP error only.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "pimemb_grad.h"
#include "pimemb_grad_dot.h"
#include "pimemb_grad_master.h"
#include "pimemb_grad_optim.h"
#include "pimemb_grad_segments.h"
#include "pimemb_grad_sr.h"
#include "pimemb_grad_step.h"

// This file is compiled three times (csrc/Makefile): as libpimemb_grad.so, and with -DPIMEMB_GRAD_MASTER_UNIT / -DPIMEMB_GRAD_SR_UNIT as
// the code objects of the master-weight and the stochastically rounded steps, which hold their own kernels and launchers alone.
#if defined(PIMEMB_GRAD_MASTER_UNIT) || defined(PIMEMB_GRAD_SR_UNIT)
#define PIMEMB_GRAD_KERNEL_UNIT 1
#endif

namespace {

using namespace pimemb_grad;

constexpr int kF32 = 0, kF16 = 1, kFixed32 = 2, kBF16 = 3;
constexpr uint32_t kBlock = 256;
constexpr uint32_t kTile = 1024;            // positions per workgroup of the sort, entries per workgroup of the scan
constexpr uint32_t kSlices = kTile / 64;    // 64-position slices of a tile: (round, wavefront) pairs, in position order
constexpr uint32_t kNoBag = 0xffffffffu;
enum CoefMode : uint32_t { COEF_SUM = 0, COEF_WEIGHTED = 1, COEF_MEAN = 2 };

struct u32x2 {
    uint32_t x, y;
} __attribute__((aligned(8)));

// ---- pre-pass ---------------------------------------------------------------------------------------------------------------

// The last b in [0, B) with offsets[b] <= p, or kNoBag.  A plain binary search: whatever the offsets hold, it reads inside [0, B).
template <bool IDX64>
__device__ inline uint32_t bag_of(const void *offsets, uint32_t fixed_pooling, uint32_t B, uint32_t p) {
    if (B == 0) return kNoBag;
    if (!offsets) {
        const uint32_t b = p / fixed_pooling;
        return b < B ? b : B - 1;
    }
    uint32_t lo = 0, hi = B;                 // the first b with offsets[b] > p lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        bool le;
        if (IDX64) le = static_cast<const long long *>(offsets)[mid] <= (long long)p;
        else le = static_cast<const uint32_t *>(offsets)[mid] <= p;
        if (le) lo = mid + 1;
        else hi = mid;
    }
    return lo == 0 ? kNoBag : lo - 1;
}

template <bool IDX64>
__global__ __launch_bounds__(kBlock) void grad_classify(const void *ids, const void *offsets, uint32_t fixed_pooling, uint32_t n,
                                                        uint32_t B, uint32_t nr_rows, uint32_t pad_on, uint64_t pad_idx,
                                                        uint32_t *keys, uint32_t *vals, uint32_t *bagof, uint32_t *cnt /* or NULL */,
                                                        unsigned long long *bad) {
    const uint64_t p64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p64 >= n) return;
    const uint32_t p = (uint32_t)p64;
    uint64_t id;
    bool in_table;
    if (IDX64) {
        const long long v = static_cast<const long long *>(ids)[p];
        id = (uint64_t)v;
        in_table = v >= 0 && id < nr_rows;      // compared at full width: 2^32 + 5 is not row 5
    } else {
        id = static_cast<const uint32_t *>(ids)[p];
        in_table = id < nr_rows;
    }
    const uint32_t b = bag_of<IDX64>(offsets, fixed_pooling, B, p);
    const bool padding = pad_on && id == pad_idx;
    uint32_t key = nr_rows;                     // not good: behind every row
    if (b != kNoBag && !padding) {
        if (cnt) atomicAdd(&cnt[b], 1u);        // good or bad: what the forward's mean divided by (integer adds: any order)
        if (in_table) key = (uint32_t)id;
        else atomicAdd(bad, 1ull);
    }
    keys[p] = key;
    vals[p] = p;
    bagof[p] = b;
}

// Exclusive scan of one value per thread over the workgroup (256 threads); *total = the workgroup's sum.
__device__ inline uint32_t block_scan(uint32_t v, uint32_t *total, uint32_t *wave_sums /* LDS, 4 */) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, off);
        if (lane >= off) inc += o;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBlock / 64; w++) {
        const uint32_t s = wave_sums[w];
        if (w < wave) base += s;
        tot += s;
    }
    __syncthreads();                            // (wave_sums may be written again by the caller's next round)
    *total = tot;
    return base + inc - v;
}

__device__ inline uint32_t head_flag(const uint32_t *keys, uint32_t i, uint32_t n, uint32_t nr_rows) {
    if (i >= n) return 0;
    const uint32_t k = keys[i];
    return k < nr_rows && (i == 0 || keys[i - 1] != k);
}

// Level one of the scan: workgroup `blk` scans entries [1024 blk, 1024 blk + 1024) of `data` (HEADS: of the run-head flags of the
// sorted `keys`) into out[], relative to the chunk's start, and leaves the chunk's sum in sums[blk].
template <bool HEADS>
__global__ __launch_bounds__(kBlock) void grad_scan_chunks(const uint32_t *data, uint32_t len, uint32_t nr_rows, uint32_t *out, uint32_t *sums) {
    __shared__ uint32_t wave_sums[kBlock / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * kTile + threadIdx.x * 4u;
    uint32_t a[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint64_t i = i0 + j;
        if (HEADS) a[j] = i < len ? head_flag(data, (uint32_t)i, len, nr_rows) : 0u;
        else a[j] = i < len ? data[i] : 0u;
    }
    uint32_t total;
    uint32_t run = block_scan(a[0] + a[1] + a[2] + a[3], &total, wave_sums);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        if (i0 + j < len) out[i0 + j] = run;
        run += a[j];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// Level two: ONE workgroup scans the chunk sums in place; *total_out (may be NULL) = the sum of everything.
#ifndef PIMEMB_GRAD_KERNEL_UNIT      // (a kernel of libpimemb_grad.so alone: the master and SR units emit only their own)
__global__ __launch_bounds__(kBlock) void grad_scan_sums(uint32_t *sums, uint32_t n_chunks, unsigned long long *total_out) {
    __shared__ uint32_t wave_sums[kBlock / 64];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_chunks; base += kTile) {      // (uniform trip count)
        const uint32_t i0 = base + threadIdx.x * 4u;
        uint32_t a[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) a[j] = i0 + j < n_chunks ? sums[i0 + j] : 0u;
        uint32_t total;
        uint32_t run = carry + block_scan(a[0] + a[1] + a[2] + a[3], &total, wave_sums);
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            if (i0 + j < n_chunks) sums[i0 + j] = run;
            run += a[j];
        }
        carry += total;
    }
    if (total_out && threadIdx.x == 0) *total_out = carry;
}
#endif

// Digit counts of tile `blk`, stored digit-major -- hist[digit * n_tiles + blk] -- so that one exclusive scan over the whole
// matrix gives every (digit, tile) pair the place of its first position.
#ifndef PIMEMB_GRAD_KERNEL_UNIT      // (a kernel of libpimemb_grad.so alone: the master and SR units emit only their own)
__global__ __launch_bounds__(kBlock) void grad_sort_count(const uint32_t *keys, uint32_t n, uint32_t shift, uint32_t *hist, uint32_t n_tiles) {
    __shared__ uint32_t counts[256];
    counts[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kTile;
#pragma unroll
    for (uint32_t r = 0; r < kTile / kBlock; r++) {
        const uint64_t i = base + r * kBlock + threadIdx.x;
        if (i < n) atomicAdd(&counts[(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * n_tiles + blockIdx.x] = counts[threadIdx.x];
}
#endif

// The stable scatter of one pass.  A tile is 16 slices of 64 consecutive positions (round r of wavefront w: slice 4 r + w).  Inside
// a slice, the lanes that hold the same digit find each other with 8 ballots: a position's rank among them is the number of
// such lanes below it, and the lowest of them records their count.  Thread d then turns digit d's 16 slice counts into
// offsets, and a position goes to   (scanned hist of its digit and tile) + (its slice's offset) + (its rank in the slice).
#ifndef PIMEMB_GRAD_KERNEL_UNIT      // (a kernel of libpimemb_grad.so alone: the master and SR units emit only their own)
__global__ __launch_bounds__(kBlock) void grad_sort_scatter(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out,
                                                            uint32_t *vals_out, uint32_t n, uint32_t shift, const uint32_t *hist,
                                                            const uint32_t *sums, uint32_t n_tiles) {
    __shared__ uint32_t slice_counts[kSlices][256];
    __shared__ uint32_t digit_base[256];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t s = 0; s < kSlices; s++) slice_counts[s][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kTile;
    uint32_t key[kTile / kBlock], val[kTile / kBlock], rank[kTile / kBlock];
#pragma unroll
    for (uint32_t r = 0; r < kTile / kBlock; r++) {
        const uint64_t i = base + r * kBlock + threadIdx.x;
        const bool live = i < n;
        key[r] = live ? keys_in[i] : 0u;
        val[r] = live ? vals_in[i] : 0u;
        const uint32_t d = (key[r] >> shift) & 255u;
        unsigned long long same = __ballot(live);
#pragma unroll
        for (uint32_t bit = 0; bit < 8; bit++) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long m = __ballot(one);
            same &= one ? m : ~m;
        }
        rank[r] = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (live && rank[r] == 0) slice_counts[r * (kBlock / 64) + wave][d] = (uint32_t)__popcll(same);
    }
    __syncthreads();
    {
        const uint32_t d = threadIdx.x;
        uint32_t run = 0;
#pragma unroll
        for (uint32_t s = 0; s < kSlices; s++) {
            const uint32_t c = slice_counts[s][d];
            slice_counts[s][d] = run;
            run += c;
        }
        const uint64_t at = (uint64_t)d * n_tiles + blockIdx.x;
        digit_base[d] = hist[at] + sums[at / kTile];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kTile / kBlock; r++) {
        const uint64_t i = base + r * kBlock + threadIdx.x;
        if (i >= n) continue;
        const uint32_t d = (key[r] >> shift) & 255u;
        const uint32_t dst = digit_base[d] + slice_counts[r * (kBlock / 64) + wave][d] + rank[r];
        if (dst < n) {                         // (always, the counts being those of these very keys: kept as the bound of the store)
            keys_out[dst] = key[r];
            vals_out[dst] = val[r];
        }
    }
}
#endif

// ---- the hot kernels --------------------------------------------------------------------------------------------------------

struct RowArgs {
    const uint32_t *keys;        // sorted: the row id of every good position, runs of equal ids in position order; then nr_rows
    const uint32_t *vals;        // the position behind every key
    const uint32_t *bagof;       // position -> bag
    const uint32_t *cnt;         // bag -> cnt (mean)
    const float *weights;        // position -> w (weighted sum)
    const float *grad;           // G
    uint64_t ld;                 // floats from one row of G to the next
    uint32_t n;
    uint32_t n_bags;
    uint32_t nr_rows;
    uint32_t dim;
    uint32_t coef;               // CoefMode
    // the sparse gradient
    const uint32_t *uidx;        // sorted place -> number of its unique row, relative to its chunk of 1024 places
    const uint32_t *usums;       // ... + this per chunk
    long long *rows_out;
    float *grads_out;
    // the fused step
    char *table;
    uint32_t stride;             // bytes from one table row to the next
    int dtype;
    float lr;
    // the Adagrad steps
    float *state;                // S: float[nr_rows][dim] (element-wise) or float[nr_rows] (row-wise)
    float eps;
};

// The scalar a position's G row is multiplied with (weighted) or divided by (mean); 0 for a plain sum.
__device__ inline float coef_of(const RowArgs &a, uint32_t p, uint32_t b) {
    if (a.coef == COEF_WEIGHTED) return a.weights[p];
    if (a.coef == COEF_MEAN) return (float)a.cnt[b];
    return 0.f;
}

__device__ inline float contribution(uint32_t coef, float g, float s) {
#pragma clang fp contract(off)
    if (coef == COEF_WEIGHTED) return s * g;
    if (coef == COEF_MEAN) return __fdiv_rn(g, s);
    return g;
}

__device__ inline float add_in_order(float acc, float c) {
#pragma clang fp contract(off)
    return acc + c;
}

constexpr uint32_t kAhead = 8;      // occurrences whose loads are in flight before the first add

// What a hot kernel does with g[r]: write it out, or step the row with it.
enum ResultKind : int { RES_SPARSE = 0, RES_SGD = 1, RES_ADAGRAD = 2, RES_ROWWISE = 3 };

// The run walk of one 16-byte piece: g[row][4c .. 4c + 3], the run that starts at sorted place i summed in position order.
__device__ __forceinline__ float4 walk_piece(const RowArgs &a, uint32_t i, uint32_t row, uint32_t c) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t j = i;
    for (;;) {
        bool live[kAhead];
        float4 g[kAhead];
        float s[kAhead];
#pragma unroll
        for (uint32_t k = 0; k < kAhead; k++) {      // the loads of up to kAhead occurrences (a dead slot re-reads the run's first)
            live[k] = k == 0 || (live[k - 1] && j + k < a.n && a.keys[j + k] == row);
            const uint32_t p = min(a.vals[live[k] ? j + k : j], a.n - 1u);      // (what the pre-pass wrote lies below these bounds:
            const uint32_t b = min(a.bagof[p], a.n_bags - 1u);                  //  they are the bounds of the loads all the same)
            s[k] = coef_of(a, p, b);
            g[k] = *reinterpret_cast<const float4 *>(a.grad + (uint64_t)b * a.ld + 4u * c);
        }
#pragma unroll
        for (uint32_t k = 0; k < kAhead; k++) {      // the adds, in position order
            if (live[k]) {
                acc.x = add_in_order(acc.x, contribution(a.coef, g[k].x, s[k]));
                acc.y = add_in_order(acc.y, contribution(a.coef, g[k].y, s[k]));
                acc.z = add_in_order(acc.z, contribution(a.coef, g[k].z, s[k]));
                acc.w = add_in_order(acc.w, contribution(a.coef, g[k].w, s[k]));
            }
        }
        if (!live[kAhead - 1]) break;
        j += kAhead;
        if (j >= a.n || a.keys[j] != row) break;
    }
    return acc;
}

// The tail of a stepped row's piece c: decode / step / encode and ONE vector store (16 bytes fp32, 8 bytes fp16 / bf16).  `rate` is
// lr (RES_SGD, RES_ADAGRAD) or the row's step size (RES_ROWWISE); RES_ADAGRAD reads, steps and stores the piece of the state too.
template <int KIND>
__device__ __forceinline__ void step_piece(const RowArgs &a, uint32_t row, uint32_t c, float4 acc, float rate) {
    float4 *sp = nullptr;
    float4 st = make_float4(0.f, 0.f, 0.f, 0.f);
    if (KIND == RES_ADAGRAD) {
        sp = reinterpret_cast<float4 *>(a.state + (uint64_t)row * a.dim) + c;
        st = *sp;
    }
    if (a.dtype == kStepF32) {
        float4 *w = reinterpret_cast<float4 *>(a.table + (uint64_t)row * a.stride) + c;
        float4 v = *w;
        if (KIND == RES_ADAGRAD) {
            v.x = bits_f32(adagrad_step(kStepF32, f32_bits(v.x), acc.x, &st.x, rate, a.eps));
            v.y = bits_f32(adagrad_step(kStepF32, f32_bits(v.y), acc.y, &st.y, rate, a.eps));
            v.z = bits_f32(adagrad_step(kStepF32, f32_bits(v.z), acc.z, &st.z, rate, a.eps));
            v.w = bits_f32(adagrad_step(kStepF32, f32_bits(v.w), acc.w, &st.w, rate, a.eps));
        } else {
            v.x = step_f32(v.x, acc.x, rate);
            v.y = step_f32(v.y, acc.y, rate);
            v.z = step_f32(v.z, acc.z, rate);
            v.w = step_f32(v.w, acc.w, rate);
        }
        *w = v;
    } else {
        u32x2 *w = reinterpret_cast<u32x2 *>(a.table + (uint64_t)row * a.stride) + c;
        const u32x2 v = *w;
        u32x2 o;
        if (KIND == RES_ADAGRAD) {
            o.x = adagrad_step(a.dtype, v.x & 0xffffu, acc.x, &st.x, rate, a.eps) | (adagrad_step(a.dtype, v.x >> 16, acc.y, &st.y, rate, a.eps) << 16);
            o.y = adagrad_step(a.dtype, v.y & 0xffffu, acc.z, &st.z, rate, a.eps) | (adagrad_step(a.dtype, v.y >> 16, acc.w, &st.w, rate, a.eps) << 16);
        } else {
            o.x = step(a.dtype, v.x & 0xffffu, acc.x, rate) | (step(a.dtype, v.x >> 16, acc.y, rate) << 16);
            o.y = step(a.dtype, v.y & 0xffffu, acc.z, rate) | (step(a.dtype, v.y >> 16, acc.w, rate) << 16);
        }
        *w = o;
    }
    if (KIND == RES_ADAGRAD) *sp = st;
}

// t[c] of the row-wise definition: ((sq0 + sq1) + sq2) + sq3 over a piece's squares.
__device__ __forceinline__ float piece_squares(float4 g) {
    return adagrad_add(adagrad_add(adagrad_add(adagrad_square(g.x), adagrad_square(g.y)), adagrad_square(g.z)), adagrad_square(g.w));
}

// One unique row per group of `lanes` lanes (a power of two up to 64); lane lg handles the row's 16-byte pieces lg, lg + lanes
// (two only beyond dim 256).  Place i of the sorted order is worked on only where a run starts there.
// RES_ROWWISE needs the whole row's g before the first table store: a lane walks the run for piece lg, then for piece lg + lanes,
// and keeps both sums (two accumulators -- the second walk's loads reuse the first's registers: no scratch in the ISA); the
// lanes of a group with no piece (dim 48: 12 pieces, 16 lanes) stay, hold +0 and take part in every shuffle.  The shuffles sit
// behind the walk, where the lanes of a group have come together again -- the groups of one wavefront walk runs of different
// lengths, and the groups that are no run head have left -- and reach across xor distances below `lanes` only: never into
// another group, never into a lane that has returned.
template <int KIND>
__global__ __launch_bounds__(kBlock) void grad_rows_group(RowArgs a, uint32_t lanes, uint32_t lanes_log2, uint32_t chunks) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t i64 = gid >> lanes_log2;
    const uint32_t lg = (uint32_t)gid & (lanes - 1);
    if (i64 >= a.n || (KIND != RES_ROWWISE && lg >= chunks)) return;
    const uint32_t i = (uint32_t)i64;
    const uint32_t row = a.keys[i];
    if (row >= a.nr_rows || (i > 0 && a.keys[i - 1] == row)) return;      // (uniform over the lane group)
    if (KIND == RES_ROWWISE) {
        const bool own0 = lg < chunks, own1 = lg + lanes < chunks;        // (own1: beyond dim 256 only, where lanes == 64)
        float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f), acc1 = acc0;
        if (own0) acc0 = walk_piece(a, i, row, lg);
        if (own1) acc1 = walk_piece(a, i, row, lg + lanes);
        float v = piece_squares(acc0);                                    // (+0 in a lane without a piece)
        if (own1) v = adagrad_add(v, piece_squares(acc1));
        for (uint32_t h = 1; h < lanes; h <<= 1) v = adagrad_add(v, __shfl_xor(v, (int)h));      // the pair tree: the same bits in every lane
        float s = a.state[row];
        const float rate = rowwise_step_size(v, a.dim, &s, a.lr, a.eps);
        if (lg == 0) a.state[row] = s;                                    // (every lane's load of S[r] feeds its own s: it is done before this store issues)
        if (own0) step_piece<KIND>(a, row, lg, acc0, rate);
        if (own1) step_piece<KIND>(a, row, lg + lanes, acc1, rate);
        return;
    }
    for (uint32_t c = lg; c < chunks; c += lanes) {
        const float4 acc = walk_piece(a, i, row, c);
        if (KIND == RES_SPARSE) {
            const uint32_t u = a.uidx[i] + a.usums[i / kTile];
            if (c == 0) a.rows_out[u] = (long long)row;
            *reinterpret_cast<float4 *>(a.grads_out + (uint64_t)u * a.dim + 4u * c) = acc;
        } else {
            step_piece<KIND>(a, row, c, acc, a.lr);
        }
    }
}

// ---- the multi-table step: one classify and one hot launch for a group of descriptors -------------------------------------------

constexpr uint32_t kMultiMax = EMB_GRAD_MULTI_MAX;

// One descriptor of a group, as the two kernels below need it.  Positions, bags and keys of the group are the descriptors'
// laid end to end: descriptor k owns positions [pos_base, pos_base + n), cnt[bag_base ...] and keys [key_base, key_base + nr_rows).
struct MultiDesc {
    const void *ids;
    const void *offsets;
    const float *weights;        // position (of this descriptor) -> w, or NULL
    const float *grad;
    uint64_t ld;
    uint64_t pad_idx;
    char *table;
    float *state;
    uint32_t pos_base, n;
    uint32_t bag_base, n_bags;
    uint32_t key_base, nr_rows;
    uint32_t fixed_pooling;
    uint32_t pad_on;
    uint32_t coef;               // CoefMode
    uint32_t stride;
    int dtype;
    uint32_t unused;
};

// The records of a group travel BY VALUE, as kernel arguments (16 x 112 bytes and a few words: well under the 4 KB a launch takes):
// the call stays a pure enqueue, with nothing to copy and nothing that must outlive it.  The kernels read them straight from the
// argument segment, with the descriptor's number as the index (the ISA shows plain loads, no scratch).
struct MultiArgs {
    MultiDesc d[kMultiMax];
    uint32_t k;                  // descriptors in use: 2 .. 16
    uint32_t n;                  // positions of the group
    uint32_t key_end;            // the sum of nr_rows: the key of every position that is not good
    uint32_t dim;
};

// The classify of a group: one thread per position of the concatenation.  It finds its descriptor among the <= 16 position bases
// and then does what grad_classify does inside that descriptor: the bag in ITS offsets, good / bad / padding against ITS table,
// cnt in ITS share of cnt[].  bagof[] holds the bag number inside the descriptor; vals[] the position in the group.
template <bool IDX64>
__global__ __launch_bounds__(kBlock) void grad_multi_classify(const MultiArgs m, uint32_t *keys, uint32_t *vals, uint32_t *bagof, uint32_t *cnt,
                                                              unsigned long long *bad) {
    const uint64_t p64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p64 >= m.n) return;
    const uint32_t pg = (uint32_t)p64;
    uint32_t k = 0;
    for (uint32_t j = 1; j < m.k; j++)           // (uniform trip count; the bases ascend)
        if (m.d[j].pos_base <= pg) k = j;
    const MultiDesc &d = m.d[k];
    const uint32_t p = pg - d.pos_base;
    uint64_t id;
    bool in_table;
    if (IDX64) {
        const long long v = static_cast<const long long *>(d.ids)[p];
        id = (uint64_t)v;
        in_table = v >= 0 && id < d.nr_rows;    // compared at full width, against this descriptor's table
    } else {
        id = static_cast<const uint32_t *>(d.ids)[p];
        in_table = id < d.nr_rows;
    }
    const uint32_t b = bag_of<IDX64>(d.offsets, d.fixed_pooling, d.n_bags, p);
    const bool padding = d.pad_on && id == d.pad_idx;
    uint32_t key = m.key_end;                   // not good: behind every row of every table
    if (b != kNoBag && !padding) {
        if (d.coef == COEF_MEAN) atomicAdd(&cnt[d.bag_base + b], 1u);
        if (in_table) key = d.key_base + (uint32_t)id;
        else atomicAdd(bad, 1ull);
    }
    keys[pg] = key;
    vals[pg] = pg;
    bagof[pg] = b;
}

// The row-wise tail between the run walk and the table stores, in grad_rows_group's order: the row's squares over the lane group
// (the same pair tree), S[row] stepped and stored by lane 0, the row's step size in every lane.
__device__ __forceinline__ float rowwise_rate(const RowArgs &a, uint32_t row, uint32_t lg, uint32_t lanes, float4 acc0, float4 acc1, bool own1) {
    float v = piece_squares(acc0);                                        // (+0 in a lane without a piece)
    if (own1) v = adagrad_add(v, piece_squares(acc1));
    for (uint32_t h = 1; h < lanes; h <<= 1) v = adagrad_add(v, __shfl_xor(v, (int)h));
    float s = a.state[row];
    const float rate = rowwise_step_size(v, a.dim, &s, a.lr, a.eps);
    if (lg == 0) a.state[row] = s;
    return rate;
}

// The hot kernel of a group: grad_rows_group with the RowArgs of the run's descriptor, found once per run from its key.
template <int KIND>
__global__ __launch_bounds__(kBlock) void grad_multi_rows(const MultiArgs m, const uint32_t *keys, const uint32_t *vals, const uint32_t *bagof,
                                                          const uint32_t *cnt, float lr, float eps, uint32_t lanes, uint32_t lanes_log2,
                                                          uint32_t chunks) {
    static_assert(KIND != RES_SPARSE, "the multi-table path steps; emb_grad_sparse stays single");
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t i64 = gid >> lanes_log2;
    const uint32_t lg = (uint32_t)gid & (lanes - 1);
    if (i64 >= m.n || (KIND != RES_ROWWISE && lg >= chunks)) return;
    const uint32_t i = (uint32_t)i64;
    const uint32_t key = keys[i];
    if (key >= m.key_end || (i > 0 && keys[i - 1] == key)) return;        // (uniform over the lane group)
    uint32_t k = 0;
    for (uint32_t j = 1; j < m.k; j++)
        if (m.d[j].key_base <= key) k = j;
    const MultiDesc &d = m.d[k];
    RowArgs a{};
    a.keys = keys;
    a.vals = vals;
    a.bagof = bagof;
    a.cnt = cnt + d.bag_base;
    a.weights = d.weights ? d.weights - d.pos_base : nullptr;             // (vals[] hold positions of the group)
    a.grad = d.grad;
    a.ld = d.ld;
    a.n = m.n;
    a.n_bags = d.n_bags;
    a.nr_rows = d.nr_rows;
    a.dim = m.dim;
    a.coef = d.coef;
    a.table = d.table;
    a.stride = d.stride;
    a.dtype = d.dtype;
    a.lr = lr;
    a.state = d.state;
    a.eps = eps;
    // from here on grad_rows_group's steps, with the run's key and the row it names apart (that kernel keeps its own text: its
    // machine code is the one its profile was taken on); every operation on values is in the device functions both call
    const uint32_t row = key - d.key_base;
    if (KIND == RES_ROWWISE) {
        const bool own0 = lg < chunks, own1 = lg + lanes < chunks;
        float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f), acc1 = acc0;
        if (own0) acc0 = walk_piece(a, i, key, lg);
        if (own1) acc1 = walk_piece(a, i, key, lg + lanes);
        const float rate = rowwise_rate(a, row, lg, lanes, acc0, acc1, own1);
        if (own0) step_piece<KIND>(a, row, lg, acc0, rate);
        if (own1) step_piece<KIND>(a, row, lg + lanes, acc1, rate);
        return;
    }
    for (uint32_t c = lg; c < chunks; c += lanes) step_piece<KIND>(a, row, c, walk_piece(a, i, key, c), a.lr);
}

// One thread per (sorted place, element): works where a run starts.  (No RES_ROWWISE: no thread here sees a whole row of g.)
template <int KIND>
__global__ __launch_bounds__(kBlock) void grad_rows_elem(RowArgs a) {
    static_assert(KIND != RES_ROWWISE, "the element-wise kernel has no row-wide view of g");
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t i64 = gid / a.dim;
    const uint32_t c = (uint32_t)(gid - i64 * a.dim);
    if (i64 >= a.n) return;
    const uint32_t i = (uint32_t)i64;
    const uint32_t row = a.keys[i];
    if (row >= a.nr_rows || (i > 0 && a.keys[i - 1] == row)) return;
    float acc = 0.f;
    for (uint32_t j = i; j < a.n && a.keys[j] == row; j++) {
        const uint32_t p = min(a.vals[j], a.n - 1u);
        const uint32_t b = min(a.bagof[p], a.n_bags - 1u);
        acc = add_in_order(acc, contribution(a.coef, a.grad[(uint64_t)b * a.ld + c], coef_of(a, p, b)));
    }
    if (KIND == RES_SPARSE) {
        const uint32_t u = a.uidx[i] + a.usums[i / kTile];
        if (c == 0) a.rows_out[u] = (long long)row;
        a.grads_out[(uint64_t)u * a.dim + c] = acc;
        return;
    }
    float *sp = KIND == RES_ADAGRAD ? a.state + (uint64_t)row * a.dim + c : nullptr;
    float st = KIND == RES_ADAGRAD ? *sp : 0.f;
    if (a.dtype == kStepF32) {
        float *w = reinterpret_cast<float *>(a.table + (uint64_t)row * a.stride) + c;
        if (KIND == RES_ADAGRAD) *w = bits_f32(adagrad_step(kStepF32, f32_bits(*w), acc, &st, a.lr, a.eps));
        else *w = step_f32(*w, acc, a.lr);
    } else {
        uint16_t *w = reinterpret_cast<uint16_t *>(a.table + (uint64_t)row * a.stride) + c;
        if (KIND == RES_ADAGRAD) *w = (uint16_t)adagrad_step(a.dtype, *w, acc, &st, a.lr, a.eps);
        else *w = (uint16_t)step(a.dtype, *w, acc, a.lr);
    }
    if (KIND == RES_ADAGRAD) *sp = st;
}

// ---- EMB_GRAD_ORDER_SEGMENTED: the same kernels over a second, equally fixed order of additions -----------------------------------
// A run longer than S is summed in two levels: t_j, the sum of its j-th segment of S occurrences in position order from +0, and
// g = ((t_0 + t_1) + t_2) + ...  The partials launch computes every t_j of every long run in parallel, one lane group per segment,
// into the context's partial buffer (csrc/pimemb_grad_segments.h numbers the slots); the hot kernels' segmented twins read them
// back in segment order.  A run of up to S occurrences is walked as before.  The kernels above keep their text and their machine
// code: what is segmented lives in the kernels below, and their extra arguments travel in SegArgs, not in RowArgs / MultiArgs.

struct SegArgs {
    float4 *partials;            // [n_slots][chunks]: t_j of the segment in slot seg_slot(its first sorted place), piece by piece
    uint32_t S, S_log2;
    uint32_t n_slots;            // slots the buffer holds at this call's `chunks`: the bound of every slot number
};

// Whether sorted place i (key `key`, a good one) starts a segment of a long run: 0 no, 1 yes, 2 yes and it is the run's head.
// A head starts one iff the run reaches S places further.  Any other place lies fewer than S places behind its head unless
// keys[i - S] is the same key; only then is the head looked for, as the lower bound of `key` in the sorted keys [0, i - S].
__device__ __forceinline__ int seg_start_kind(const uint32_t *keys, uint32_t n, uint32_t i, uint32_t key, uint32_t S) {
    if (i == 0 || keys[i - 1] != key) return i + S < n && keys[i + S] == key ? 2 : 0;      // (i < n <= 2^30, S <= 1024)
    if (i < S || keys[i - S] != key) return 0;
    uint32_t lo = 0, hi = i - S;                 // keys[hi] == key: the head lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return ((i - lo) & (S - 1u)) == 0 ? 1 : 0;
}

// walk_piece bounded to one segment: t_j[4c .. 4c + 3] of the segment that starts at sorted place i, its up to S occurrences summed
// in position order from +0, eight loads in flight (S is a multiple of eight: a full segment is whole rounds).
__device__ __forceinline__ float4 walk_segment(const RowArgs &a, uint32_t i, uint32_t row, uint32_t c, uint32_t S) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t end = min(i + S, a.n);
    uint32_t j = i;
    for (;;) {
        bool live[kAhead];
        float4 g[kAhead];
        float s[kAhead];
#pragma unroll
        for (uint32_t k = 0; k < kAhead; k++) {      // (a dead slot re-reads the round's first occurrence)
            live[k] = k == 0 || (live[k - 1] && j + k < end && a.keys[j + k] == row);
            const uint32_t p = min(a.vals[live[k] ? j + k : j], a.n - 1u);
            const uint32_t b = min(a.bagof[p], a.n_bags - 1u);
            s[k] = coef_of(a, p, b);
            g[k] = *reinterpret_cast<const float4 *>(a.grad + (uint64_t)b * a.ld + 4u * c);
        }
#pragma unroll
        for (uint32_t k = 0; k < kAhead; k++) {      // the adds, in position order
            if (live[k]) {
                acc.x = add_in_order(acc.x, contribution(a.coef, g[k].x, s[k]));
                acc.y = add_in_order(acc.y, contribution(a.coef, g[k].y, s[k]));
                acc.z = add_in_order(acc.z, contribution(a.coef, g[k].z, s[k]));
                acc.w = add_in_order(acc.w, contribution(a.coef, g[k].w, s[k]));
            }
        }
        if (!live[kAhead - 1]) break;
        j += kAhead;
        if (j >= end || a.keys[j] != row) break;
    }
    return acc;
}

// The run walk of one piece in the segmented order.  A run of up to S occurrences is walk_piece's; a longer one is the sum of its
// partials, starting from t_0: the loads of eight of them (and of the keys that say whether their segments exist) are independent
// of each other and in flight together, the adds in segment order.  The slot of a segment follows from its place alone.
__device__ __forceinline__ float4 seg_walk_piece(const RowArgs &a, const SegArgs &sg, uint32_t i, uint32_t row, uint32_t c, uint32_t chunks) {
    if (!(i + sg.S < a.n && a.keys[i + sg.S] == row)) return walk_piece(a, i, row, c);
    float4 acc = sg.partials[(uint64_t)min(seg_slot(i, sg.S_log2, true), sg.n_slots - 1u) * chunks + c];      // t_0 itself: the sum starts from it
    uint32_t j = i + sg.S;                       // where the round's first segment starts: t_1 exists, the run being long
    for (;;) {
        uint32_t live = 1;                       // segments of this round that exist: the first `live` of its eight
        float4 t[kAhead];
#pragma unroll
        for (uint32_t k = 0; k < kAhead; k++) {      // (a dead slot re-reads the round's first partial)
            const uint32_t at = j + k * sg.S;        // (j < n <= 2^30, k * S < 2^13)
            if (k > 0 && live == k && at < a.n && a.keys[at] == row) live = k + 1;
            const uint32_t slot = min(seg_slot(k < live ? at : j, sg.S_log2, false), sg.n_slots - 1u);
            t[k] = sg.partials[(uint64_t)slot * chunks + c];
        }
#pragma unroll
        for (uint32_t k = 0; k < kAhead; k++) {      // the adds, in segment order
            if (k < live) {
                acc.x = add_in_order(acc.x, t[k].x);
                acc.y = add_in_order(acc.y, t[k].y);
                acc.z = add_in_order(acc.z, t[k].z);
                acc.w = add_in_order(acc.w, t[k].w);
            }
        }
        if (live < kAhead) break;
        j += kAhead * sg.S;
        if (j >= a.n || a.keys[j] != row) break;
    }
    return acc;
}

// The partials of the long runs' segments: a lane group that starts one sums it, lane lg the pieces lg, lg + lanes, and stores
// them with plain vector stores.
__device__ __forceinline__ void seg_partials_body(const RowArgs &a, const SegArgs &sg, uint32_t i, uint32_t key, int kind, uint32_t lg, uint32_t lanes,
                                                  uint32_t chunks) {
    const uint32_t slot = min(seg_slot(i, sg.S_log2, kind == 2), sg.n_slots - 1u);
    for (uint32_t c = lg; c < chunks; c += lanes) sg.partials[(uint64_t)slot * chunks + c] = walk_segment(a, i, key, c, sg.S);
}

// One lane group per sorted place, as grad_rows_group is launched; it works where a segment of a long run starts.
#ifndef PIMEMB_GRAD_KERNEL_UNIT      // (a kernel of libpimemb_grad.so alone: the master and SR units emit only their own)
__global__ __launch_bounds__(kBlock) void grad_seg_partials(RowArgs a, SegArgs sg, uint32_t lanes, uint32_t lanes_log2, uint32_t chunks) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t i64 = gid >> lanes_log2;
    const uint32_t lg = (uint32_t)gid & (lanes - 1);
    if (i64 >= a.n || lg >= chunks) return;
    const uint32_t i = (uint32_t)i64;
    const uint32_t row = a.keys[i];
    if (row >= a.nr_rows) return;
    const int kind = seg_start_kind(a.keys, a.n, i, row, sg.S);           // (uniform over the lane group)
    if (kind) seg_partials_body(a, sg, i, row, kind, lg, lanes, chunks);
}
#endif

// What grad_rows_group does with a run, in the segmented order; `key` is what the run's places hold, `row` the table row it names.
template <int KIND>
__device__ __forceinline__ void seg_rows_body(const RowArgs &a, const SegArgs &sg, uint32_t i, uint32_t key, uint32_t row, uint32_t lg, uint32_t lanes,
                                              uint32_t chunks) {
    if (KIND == RES_ROWWISE) {
        const bool own0 = lg < chunks, own1 = lg + lanes < chunks;
        float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f), acc1 = acc0;
        if (own0) acc0 = seg_walk_piece(a, sg, i, key, lg, chunks);
        if (own1) acc1 = seg_walk_piece(a, sg, i, key, lg + lanes, chunks);
        const float rate = rowwise_rate(a, row, lg, lanes, acc0, acc1, own1);
        if (own0) step_piece<KIND>(a, row, lg, acc0, rate);
        if (own1) step_piece<KIND>(a, row, lg + lanes, acc1, rate);
        return;
    }
    for (uint32_t c = lg; c < chunks; c += lanes) {
        const float4 acc = seg_walk_piece(a, sg, i, key, c, chunks);
        if (KIND == RES_SPARSE) {
            const uint32_t u = a.uidx[i] + a.usums[i / kTile];
            if (c == 0) a.rows_out[u] = (long long)row;
            *reinterpret_cast<float4 *>(a.grads_out + (uint64_t)u * a.dim + 4u * c) = acc;
        } else {
            step_piece<KIND>(a, row, c, acc, a.lr);
        }
    }
}

// grad_rows_group in the segmented order (launched behind grad_seg_partials, with the same geometry).
template <int KIND>
__global__ __launch_bounds__(kBlock) void grad_seg_rows_group(RowArgs a, SegArgs sg, uint32_t lanes, uint32_t lanes_log2, uint32_t chunks) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t i64 = gid >> lanes_log2;
    const uint32_t lg = (uint32_t)gid & (lanes - 1);
    if (i64 >= a.n || (KIND != RES_ROWWISE && lg >= chunks)) return;
    const uint32_t i = (uint32_t)i64;
    const uint32_t row = a.keys[i];
    if (row >= a.nr_rows || (i > 0 && a.keys[i - 1] == row)) return;      // (uniform over the lane group)
    seg_rows_body<KIND>(a, sg, i, row, row, lg, lanes, chunks);
}

// The RowArgs of the descriptor a composite key belongs to, as grad_multi_rows fills them; *row = the table row the key names.
__device__ __forceinline__ RowArgs multi_row_args(const MultiArgs &m, uint32_t key, const uint32_t *keys, const uint32_t *vals, const uint32_t *bagof,
                                                  const uint32_t *cnt, float lr, float eps, uint32_t *row) {
    uint32_t k = 0;
    for (uint32_t j = 1; j < m.k; j++)
        if (m.d[j].key_base <= key) k = j;
    const MultiDesc &d = m.d[k];
    RowArgs a{};
    a.keys = keys;
    a.vals = vals;
    a.bagof = bagof;
    a.cnt = cnt + d.bag_base;
    a.weights = d.weights ? d.weights - d.pos_base : nullptr;             // (vals[] hold positions of the group)
    a.grad = d.grad;
    a.ld = d.ld;
    a.n = m.n;
    a.n_bags = d.n_bags;
    a.nr_rows = d.nr_rows;
    a.dim = m.dim;
    a.coef = d.coef;
    a.table = d.table;
    a.stride = d.stride;
    a.dtype = d.dtype;
    a.lr = lr;
    a.state = d.state;
    a.eps = eps;
    *row = key - d.key_base;
    return a;
}

// grad_seg_partials over the runs of a group's composite keys: adjacent keys of two tables are two runs, as everywhere.
#ifndef PIMEMB_GRAD_KERNEL_UNIT      // (a kernel of libpimemb_grad.so alone: the master and SR units emit only their own)
__global__ __launch_bounds__(kBlock) void grad_seg_multi_partials(const MultiArgs m, const uint32_t *keys, const uint32_t *vals, const uint32_t *bagof,
                                                                  const uint32_t *cnt, SegArgs sg, uint32_t lanes, uint32_t lanes_log2, uint32_t chunks) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t i64 = gid >> lanes_log2;
    const uint32_t lg = (uint32_t)gid & (lanes - 1);
    if (i64 >= m.n || lg >= chunks) return;
    const uint32_t i = (uint32_t)i64;
    const uint32_t key = keys[i];
    if (key >= m.key_end) return;
    const int kind = seg_start_kind(keys, m.n, i, key, sg.S);
    if (!kind) return;
    uint32_t row;
    const RowArgs a = multi_row_args(m, key, keys, vals, bagof, cnt, 0.f, 0.f, &row);
    seg_partials_body(a, sg, i, key, kind, lg, lanes, chunks);
}
#endif

// grad_multi_rows in the segmented order.
template <int KIND>
__global__ __launch_bounds__(kBlock) void grad_seg_multi_rows(const MultiArgs m, const uint32_t *keys, const uint32_t *vals, const uint32_t *bagof,
                                                              const uint32_t *cnt, float lr, float eps, SegArgs sg, uint32_t lanes, uint32_t lanes_log2,
                                                              uint32_t chunks) {
    static_assert(KIND != RES_SPARSE, "the multi-table path steps; emb_grad_sparse stays single");
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t i64 = gid >> lanes_log2;
    const uint32_t lg = (uint32_t)gid & (lanes - 1);
    if (i64 >= m.n || (KIND != RES_ROWWISE && lg >= chunks)) return;
    const uint32_t i = (uint32_t)i64;
    const uint32_t key = keys[i];
    if (key >= m.key_end || (i > 0 && keys[i - 1] == key)) return;        // (uniform over the lane group)
    uint32_t row;
    const RowArgs a = multi_row_args(m, key, keys, vals, bagof, cnt, lr, eps, &row);
    seg_rows_body<KIND>(a, sg, i, key, row, lg, lanes, chunks);
}

// grad_rows_elem in the segmented order: the thread of an element folds segment after segment itself, a nested loop in one
// chain -- the same bits as the lane-group kernels, no partial buffer, and no gain in speed.
template <int KIND>
__global__ __launch_bounds__(kBlock) void grad_seg_rows_elem(RowArgs a, uint32_t S) {
    static_assert(KIND != RES_ROWWISE, "the element-wise kernel has no row-wide view of g");
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t i64 = gid / a.dim;
    const uint32_t c = (uint32_t)(gid - i64 * a.dim);
    if (i64 >= a.n) return;
    const uint32_t i = (uint32_t)i64;
    const uint32_t row = a.keys[i];
    if (row >= a.nr_rows || (i > 0 && a.keys[i - 1] == row)) return;
    float acc = 0.f, t = 0.f;
    uint32_t in_seg = 0;
    bool first = true;                           // t_0 is taken as it is: the sum of the partials starts from it
    for (uint32_t j = i; j < a.n && a.keys[j] == row; j++) {
        const uint32_t p = min(a.vals[j], a.n - 1u);
        const uint32_t b = min(a.bagof[p], a.n_bags - 1u);
        t = add_in_order(t, contribution(a.coef, a.grad[(uint64_t)b * a.ld + c], coef_of(a, p, b)));
        if (++in_seg == S) {
            acc = first ? t : add_in_order(acc, t);
            first = false;
            t = 0.f;
            in_seg = 0;
        }
    }
    if (in_seg) acc = first ? t : add_in_order(acc, t);
    if (KIND == RES_SPARSE) {
        const uint32_t u = a.uidx[i] + a.usums[i / kTile];
        if (c == 0) a.rows_out[u] = (long long)row;
        a.grads_out[(uint64_t)u * a.dim + c] = acc;
        return;
    }
    float *sp = KIND == RES_ADAGRAD ? a.state + (uint64_t)row * a.dim + c : nullptr;
    float st = KIND == RES_ADAGRAD ? *sp : 0.f;
    if (a.dtype == kStepF32) {
        float *w = reinterpret_cast<float *>(a.table + (uint64_t)row * a.stride) + c;
        if (KIND == RES_ADAGRAD) *w = bits_f32(adagrad_step(kStepF32, f32_bits(*w), acc, &st, a.lr, a.eps));
        else *w = step_f32(*w, acc, a.lr);
    } else {
        uint16_t *w = reinterpret_cast<uint16_t *>(a.table + (uint64_t)row * a.stride) + c;
        if (KIND == RES_ADAGRAD) *w = (uint16_t)adagrad_step(a.dtype, *w, acc, &st, a.lr, a.eps);
        else *w = (uint16_t)step(a.dtype, *w, acc, a.lr);
    }
    if (KIND == RES_ADAGRAD) *sp = st;
}

// ---- the master-weight steps: M' = step(M, g), W = enc_T(M') (csrc/pimemb_grad_master.h) -------------------------------------------
// The same pre-pass, sort and run walk; the tail reads and writes the caller's fp32 master row where the kernels above decode the
// table row, and stores the table row encoded from the new master: the table is never read.  The kernels above keep their text:
// what is new travels in MasterArgs beside RowArgs (a.table / a.stride / a.lr / a.eps / a.state are used as they are, a.dtype is not).

struct MasterArgs {
    float *master;               // M: float[nr_rows][dim], no padding
    int enc;                     // the table's dtype: kMasterF16 / kMasterBF16 / kMasterE4M3 / kMasterE5M2 / kMasterMXFP4
    unsigned long long *unenc;   // MXFP4: rows whose new master holds an inf or a NaN (their table bytes are kept)
};

// (the master kinds are the step kinds plus this: the tails below are instantiated for these three alone)
enum MasterKind : int { RES_MASTER_SGD = 4, RES_MASTER_ADAGRAD = 5, RES_MASTER_ROWWISE = 6 };

// The kernels of the master steps are compiled into a code object of their own: this file is compiled a second time with
// -DPIMEMB_GRAD_MASTER_UNIT into libpimemb_grad_master.so (csrc/Makefile), which holds them and exports their two launch functions;
// libpimemb_grad.so's code object is the one it was (tests pin the set of its kernels), and its host side calls the launchers.
#ifdef PIMEMB_GRAD_MASTER_UNIT

// cnt[0 .. n) = 0 ahead of a mean-mode classify.  A kernel, not a memset node.  What was observed, on this runtime: a graph of
// {prepared lookup, a copy, a mean-mode master step, prepared lookup} captured with hipMemsetAsync here replayed to tables that
// differed from the reference in every named row, with SGD and row-wise alike, while the same graph in sum mode (no clear) and the
// same mean-mode step uncaptured were exact; with this kernel the replays are exact (tests/test_gpu_master_step.py keeps both
// modes).  The row writer's hash clear showed the same under capture and became a kernel too.  What was NOT observed: emb_grad_sgd /
// emb_grad_step in mean mode under capture -- they keep their memset, tests/test_gpu_grad_graph.py replays a mean-mode batch through
// them and passes; whether they can be affected in other graphs is an open question for an issue of its own, not settled here.
__global__ __launch_bounds__(kBlock) void grad_master_clear(uint32_t *cnt, uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) cnt[i] = 0u;
}

// One master element stepped.  `rate` is lr (SGD, Adagrad) or the row's step size (row-wise); Adagrad steps *st as adagrad_step does.
template <int KIND>
__device__ __forceinline__ float master_elem(float m, float g, float *st, float rate, float eps) {
    if (KIND == RES_MASTER_ADAGRAD) return bits_f32(adagrad_step(kStepF32, f32_bits(m), g, st, rate, eps));
    return step_f32(m, g, rate);
}

// The master tail of piece c: one 16-byte load of M, the step, one 16-byte store of M' (Adagrad: the same for the piece of S).
// Returns M'[row][4c .. 4c + 3].
template <int KIND>
__device__ __forceinline__ float4 master_piece(const RowArgs &a, const MasterArgs &ma, uint32_t row, uint32_t c, float4 acc, float rate) {
    float4 *sp = nullptr;
    float4 st = make_float4(0.f, 0.f, 0.f, 0.f);
    if (KIND == RES_MASTER_ADAGRAD) {
        sp = reinterpret_cast<float4 *>(a.state + (uint64_t)row * a.dim) + c;
        st = *sp;
    }
    float4 *mp = reinterpret_cast<float4 *>(ma.master + (uint64_t)row * a.dim) + c;
    float4 m = *mp;
    m.x = master_elem<KIND>(m.x, acc.x, &st.x, rate, a.eps);
    m.y = master_elem<KIND>(m.y, acc.y, &st.y, rate, a.eps);
    m.z = master_elem<KIND>(m.z, acc.z, &st.z, rate, a.eps);
    m.w = master_elem<KIND>(m.w, acc.w, &st.w, rate, a.eps);
    *mp = m;
    if (KIND == RES_MASTER_ADAGRAD) *sp = st;
    return m;
}

// The encoded piece c of a 2-byte or 1-byte table row: ONE vector store of 8 or 4 bytes, adjacent lanes adjacent bytes.
__device__ __forceinline__ void master_store_piece(const RowArgs &a, const MasterArgs &ma, uint32_t row, uint32_t c, float4 m) {
    const uint32_t bits[4] = {f32_bits(m.x), f32_bits(m.y), f32_bits(m.z), f32_bits(m.w)};
    char *w = a.table + (uint64_t)row * a.stride;
    if (ma.enc == kMasterF16 || ma.enc == kMasterBF16) {
        u32x2 o;
        master_enc_piece16(ma.enc, bits, &o.x, &o.y);
        reinterpret_cast<u32x2 *>(w)[c] = o;
    } else {
        reinterpret_cast<uint32_t *>(w)[c] = master_enc_piece8(ma.enc, bits);
    }
}

struct u32x4 {
    uint32_t x, y, z, w;
} __attribute__((aligned(16)));

// One block's share of the MXFP4 tail, for the pieces the group's lanes hold at one of their two slots (slot 0: piece lg, slot 1:
// piece lg + 64): eight adjacent lanes are block `blk` (live: blk < nb; a lane without a piece holds +0).  Every lane of the group runs
// every shuffle.  Returns the block's 16 element bytes in its leading lane (lg % 8 == 0) and *scale = its scale byte in all eight
// (0 for a block past the row: padding); *amax_or collects the magnitudes for the row's inf / NaN flag.
__device__ __forceinline__ u32x4 master_mx_block(float4 m, bool live, uint32_t *scale, uint32_t *amax_or) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t bits[4] = {f32_bits(m.x), f32_bits(m.y), f32_bits(m.z), f32_bits(m.w)};
    uint32_t amax = mx_piece_amax(bits);
    amax = mx_max(amax, (uint32_t)__shfl_xor((int)amax, 1));
    amax = mx_max(amax, (uint32_t)__shfl_xor((int)amax, 2));
    amax = mx_max(amax, (uint32_t)__shfl_xor((int)amax, 4));      // the block's amax, in all eight of its lanes
    *amax_or = mx_max(*amax_or, amax);
    uint32_t s = pimemb_rows::mx_scale_of(amax);
    const uint32_t codes = mx_piece_codes(bits, s);
    int zeros = mx_piece_zeros(codes);
    zeros &= __shfl_xor(zeros, 1);
    zeros &= __shfl_xor(zeros, 2);
    zeros &= __shfl_xor(zeros, 4);
    if (zeros) s = 127;
    *scale = live ? s : 0u;
    const int q = (int)(lane & ~7u);
    uint32_t k[8];
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = (uint32_t)__shfl((int)codes, q + j);
    return u32x4{k[0] | (k[1] << 16), k[2] | (k[3] << 16), k[4] | (k[5] << 16), k[6] | (k[7] << 16)};
}

// The MXFP4 tail of a row whose new master pieces the group holds (m0: piece lg, m1: piece lg + lanes, +0 where a lane has none).
// dim <= 512: at most 16 blocks, their scale bytes are exactly one 16-byte tail piece with its zero padding.
__device__ __forceinline__ void master_mx_row(const RowArgs &a, const MasterArgs &ma, uint32_t row, uint32_t lg, uint32_t lanes, float4 m0, float4 m1) {
    const uint32_t nb = a.dim / 32u, blk = lg / 8u;
    const uint32_t base = (threadIdx.x & 63u) & ~(lanes - 1u);
    uint32_t s0, s1, amax = 0;
    const u32x4 e0 = master_mx_block(m0, blk < nb, &s0, &amax);
    const u32x4 e1 = master_mx_block(m1, blk + lanes / 8u < nb, &s1, &amax);      // (live only beyond dim 256, where lanes == 64)
    for (uint32_t h = 8; h < lanes; h <<= 1) amax = mx_max(amax, (uint32_t)__shfl_xor((int)amax, (int)h));      // (blocks are uniform already)
    // the tail piece: byte b = the scale of block b, from the lane that leads the block (slot 0: blocks 0 .. lanes / 8 - 1, slot 1: the next eight)
    uint32_t t[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t b = 0; b < 8; b++) {
        const uint32_t from = 8u * b;
        const uint32_t v0 = (uint32_t)__shfl((int)s0, (int)(base + (from & (lanes - 1u))));
        const uint32_t v1 = (uint32_t)__shfl((int)s1, (int)(base + (from & (lanes - 1u))));
        if (from < lanes) {
            t[b / 4] |= v0 << (8u * (b & 3u));
            t[2 + b / 4] |= v1 << (8u * (b & 3u));      // (lanes == 64 where slot 1 is live: blocks 8 .. 15 are bytes 8 .. 15)
        }
    }
    if (mx_non_finite(amax)) {                   // uniform over the group: the row keeps its table bytes and is counted
        if (lg == 0) atomicAdd(ma.unenc, 1ull);
        return;
    }
    u32x4 *dst = reinterpret_cast<u32x4 *>(a.table + (uint64_t)row * a.stride);
    if ((lg & 7u) == 0) {
        if (blk < nb) dst[blk] = e0;
        if (blk + lanes / 8u < nb) dst[blk + lanes / 8u] = e1;
    }
    if (lg == 0) dst[nb] = u32x4{t[0], t[1], t[2], t[3]};
}

// grad_rows_group / grad_seg_rows_group with the master tail.  The row-wise kind and MXFP4 need the whole row before the first
// table store (the row's step size; the blocks' amax and the row's inf / NaN flag): there every lane of a run-head group stays
// through the shuffles, lanes without a piece hold +0, and beyond dim 256 a lane keeps both pieces' sums -- as in the row-wise
// step.  All shuffles sit behind the run walk, with xor distances (and source lanes) inside the group.
template <int KIND, bool SEG>
__global__ __launch_bounds__(kBlock) void grad_master_rows_group(RowArgs a, SegArgs sg, MasterArgs ma, uint32_t lanes, uint32_t lanes_log2, uint32_t chunks) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t i64 = gid >> lanes_log2;
    const uint32_t lg = (uint32_t)gid & (lanes - 1);
    const bool wide = KIND == RES_MASTER_ROWWISE || ma.enc == kMasterMXFP4;      // (uniform over the launch)
    if (i64 >= a.n || (!wide && lg >= chunks)) return;
    const uint32_t i = (uint32_t)i64;
    const uint32_t row = a.keys[i];
    if (row >= a.nr_rows || (i > 0 && a.keys[i - 1] == row)) return;      // (uniform over the lane group)
    if (!wide) {
        for (uint32_t c = lg; c < chunks; c += lanes) {
            const float4 acc = SEG ? seg_walk_piece(a, sg, i, row, c, chunks) : walk_piece(a, i, row, c);
            master_store_piece(a, ma, row, c, master_piece<KIND>(a, ma, row, c, acc, a.lr));
        }
        return;
    }
    const bool own0 = lg < chunks, own1 = lg + lanes < chunks;            // (own1: beyond dim 256 only, where lanes == 64)
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc0 = zero, acc1 = zero;
    if (own0) acc0 = SEG ? seg_walk_piece(a, sg, i, row, lg, chunks) : walk_piece(a, i, row, lg);
    if (own1) acc1 = SEG ? seg_walk_piece(a, sg, i, row, lg + lanes, chunks) : walk_piece(a, i, row, lg + lanes);
    float rate = a.lr;
    if (KIND == RES_MASTER_ROWWISE) rate = rowwise_rate(a, row, lg, lanes, acc0, acc1, own1);
    float4 m0 = zero, m1 = zero;
    if (own0) m0 = master_piece<KIND>(a, ma, row, lg, acc0, rate);
    if (own1) m1 = master_piece<KIND>(a, ma, row, lg + lanes, acc1, rate);
    if (ma.enc == kMasterMXFP4) {
        master_mx_row(a, ma, row, lg, lanes, m0, m1);
        return;
    }
    if (own0) master_store_piece(a, ma, row, lg, m0);
    if (own1) master_store_piece(a, ma, row, lg + lanes, m1);
}

// grad_rows_elem / grad_seg_rows_elem with the master tail: one thread per (sorted place, element), the 2-byte and 1-byte dtypes.
// (No row-wise kind and no MXFP4: no thread here sees a whole row, or a whole block.)
template <int KIND, bool SEG>
__global__ __launch_bounds__(kBlock) void grad_master_rows_elem(RowArgs a, MasterArgs ma, uint32_t S) {
    static_assert(KIND != RES_MASTER_ROWWISE, "the element-wise kernel has no row-wide view of g");
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t i64 = gid / a.dim;
    const uint32_t c = (uint32_t)(gid - i64 * a.dim);
    if (i64 >= a.n) return;
    const uint32_t i = (uint32_t)i64;
    const uint32_t row = a.keys[i];
    if (row >= a.nr_rows || (i > 0 && a.keys[i - 1] == row)) return;
    float acc = 0.f, t = 0.f;
    uint32_t in_seg = 0;
    bool first = true;                           // (SEG) t_0 is taken as it is: the sum of the partials starts from it
    for (uint32_t j = i; j < a.n && a.keys[j] == row; j++) {
        const uint32_t p = min(a.vals[j], a.n - 1u);
        const uint32_t b = min(a.bagof[p], a.n_bags - 1u);
        const float cp = contribution(a.coef, a.grad[(uint64_t)b * a.ld + c], coef_of(a, p, b));
        if (!SEG) {
            acc = add_in_order(acc, cp);
            continue;
        }
        t = add_in_order(t, cp);
        if (++in_seg == S) {
            acc = first ? t : add_in_order(acc, t);
            first = false;
            t = 0.f;
            in_seg = 0;
        }
    }
    if (SEG && in_seg) acc = first ? t : add_in_order(acc, t);
    float *sp = KIND == RES_MASTER_ADAGRAD ? a.state + (uint64_t)row * a.dim + c : nullptr;
    float st = KIND == RES_MASTER_ADAGRAD ? *sp : 0.f;
    float *mp = ma.master + (uint64_t)row * a.dim + c;
    const float m = master_elem<KIND>(*mp, acc, &st, a.lr, a.eps);
    *mp = m;
    if (KIND == RES_MASTER_ADAGRAD) *sp = st;
    const uint32_t o = master_enc(ma.enc, f32_bits(m));
    char *w = a.table + (uint64_t)row * a.stride;
    if (ma.enc == kMasterF16 || ma.enc == kMasterBF16) reinterpret_cast<uint16_t *>(w)[c] = (uint16_t)o;
    else reinterpret_cast<uint8_t *>(w)[c] = (uint8_t)o;
}

}  // namespace

// The two launch functions libpimemb_grad_master.so exports (plain C; the argument records are this file's own RowArgs, SegArgs and
// MasterArgs, which both compilations lay out alike).  Errors are left to the caller's hipGetLastError().
extern "C" __attribute__((visibility("default"))) void pimemb_grad_master_clear(uint32_t *cnt, uint32_t n, void *stream) {
    grad_master_clear<<<dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, static_cast<hipStream_t>(stream)>>>(cnt, n);
}

// The hot launch of a master-weight step (a chain of one): the lane-group kernel or the element-wise one, in the context's order.
// kind: RES_SGD / RES_ADAGRAD / RES_ROWWISE; lane: the lane-group kernel with this geometry, else elem_blocks workgroups element-wise.
extern "C" __attribute__((visibility("default"))) void pimemb_grad_master_launch(const void *row_args, const void *seg_args, const void *master_args, int kind,
                                                                                  int seg, int lane, uint32_t lanes, uint32_t lanes_log2, uint32_t chunks,
                                                                                  uint32_t blocks, uint32_t elem_blocks, uint32_t S, void *stream) {
    const RowArgs &a = *static_cast<const RowArgs *>(row_args);
    const SegArgs &sg = *static_cast<const SegArgs *>(seg_args);
    const MasterArgs &ma = *static_cast<const MasterArgs *>(master_args);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(kBlock);
    if (lane) {
        const dim3 grid(blocks);
        if (kind == RES_SGD && seg) grad_master_rows_group<RES_MASTER_SGD, true><<<grid, block, 0, s>>>(a, sg, ma, lanes, lanes_log2, chunks);
        else if (kind == RES_SGD) grad_master_rows_group<RES_MASTER_SGD, false><<<grid, block, 0, s>>>(a, sg, ma, lanes, lanes_log2, chunks);
        else if (kind == RES_ADAGRAD && seg) grad_master_rows_group<RES_MASTER_ADAGRAD, true><<<grid, block, 0, s>>>(a, sg, ma, lanes, lanes_log2, chunks);
        else if (kind == RES_ADAGRAD) grad_master_rows_group<RES_MASTER_ADAGRAD, false><<<grid, block, 0, s>>>(a, sg, ma, lanes, lanes_log2, chunks);
        else if (seg) grad_master_rows_group<RES_MASTER_ROWWISE, true><<<grid, block, 0, s>>>(a, sg, ma, lanes, lanes_log2, chunks);
        else grad_master_rows_group<RES_MASTER_ROWWISE, false><<<grid, block, 0, s>>>(a, sg, ma, lanes, lanes_log2, chunks);
        return;
    }
    const dim3 grid(elem_blocks);                // (the row-wise kind never gets here: the plan refused it)
    if (kind == RES_SGD && seg) grad_master_rows_elem<RES_MASTER_SGD, true><<<grid, block, 0, s>>>(a, ma, S);
    else if (kind == RES_SGD) grad_master_rows_elem<RES_MASTER_SGD, false><<<grid, block, 0, s>>>(a, ma, 0u);
    else if (seg) grad_master_rows_elem<RES_MASTER_ADAGRAD, true><<<grid, block, 0, s>>>(a, ma, S);
    else grad_master_rows_elem<RES_MASTER_ADAGRAD, false><<<grid, block, 0, s>>>(a, ma, 0u);
}

namespace {
#else      // libpimemb_grad.so: the launchers are libpimemb_grad_master.so's
}  // namespace
extern "C" void pimemb_grad_master_clear(uint32_t *cnt, uint32_t n, void *stream);
extern "C" void pimemb_grad_master_launch(const void *row_args, const void *seg_args, const void *master_args, int kind, int seg, int lane, uint32_t lanes,
                                          uint32_t lanes_log2, uint32_t chunks, uint32_t blocks, uint32_t elem_blocks, uint32_t S, void *stream);
namespace {
#endif

// ---- the stochastically rounded steps: W' = enc_sr_T(dec(W) - ..., R) (csrc/pimemb_grad_sr.h) ---------------------------------------
// emb_grad_sgd / emb_grad_step on fp16 and bf16 tables with the last rounding alone replaced: the same pre-pass, sort, segment launch
// and run walk; the tail computes ONE Philox block per piece -- counter (row, piece, t), the lane's four elements take its four words --
// and stores the encoded piece with the vector store of step_piece.  The kernels above keep their text: what is new travels in SrArgs.

struct SrArgs {
    uint64_t seed;
    uint64_t step;               // spec.step + the descriptor's number in its call
    const uint64_t *step_dev;    // or NULL: a device word added to `step` when the kernel runs (a captured graph replays with new words)
};

// Like the master steps' kernels these live in a code object of their own: this file compiled with -DPIMEMB_GRAD_SR_UNIT into
// libpimemb_grad_sr.so (csrc/Makefile), which exports their launch function; libpimemb_grad.so's host side calls it.
#ifdef PIMEMB_GRAD_SR_UNIT

// The step number of this launch: read once per thread, the same word in every lane (a uniform load).
__device__ __forceinline__ uint64_t sr_step_of(const SrArgs &sr) { return sr.step + (sr.step_dev ? *sr.step_dev : 0ull); }

// step_piece with the stochastic encoder, on the 2-byte dtypes (the plan refuses fp32: nothing to round).
template <int KIND>
__device__ __forceinline__ void sr_step_piece(const RowArgs &a, uint64_t seed, uint64_t t, uint32_t row, uint32_t c, float4 acc, float rate) {
    float4 *sp = nullptr;
    float4 st = make_float4(0.f, 0.f, 0.f, 0.f);
    if (KIND == RES_ADAGRAD) {
        sp = reinterpret_cast<float4 *>(a.state + (uint64_t)row * a.dim) + c;
        st = *sp;
    }
    u32x2 *w = reinterpret_cast<u32x2 *>(a.table + (uint64_t)row * a.stride) + c;
    const u32x2 v = *w;
    uint32_t R[4];
    sr_words(seed, t, row, c, R);
    u32x2 o;
    if (KIND == RES_ADAGRAD) {
        o.x = adagrad_step_sr(a.dtype, v.x & 0xffffu, acc.x, &st.x, rate, a.eps, R[0]) | (adagrad_step_sr(a.dtype, v.x >> 16, acc.y, &st.y, rate, a.eps, R[1]) << 16);
        o.y = adagrad_step_sr(a.dtype, v.y & 0xffffu, acc.z, &st.z, rate, a.eps, R[2]) | (adagrad_step_sr(a.dtype, v.y >> 16, acc.w, &st.w, rate, a.eps, R[3]) << 16);
    } else {
        o.x = step_sr(a.dtype, v.x & 0xffffu, acc.x, rate, R[0]) | (step_sr(a.dtype, v.x >> 16, acc.y, rate, R[1]) << 16);
        o.y = step_sr(a.dtype, v.y & 0xffffu, acc.z, rate, R[2]) | (step_sr(a.dtype, v.y >> 16, acc.w, rate, R[3]) << 16);
    }
    *w = o;
    if (KIND == RES_ADAGRAD) *sp = st;
}

// grad_rows_group / grad_seg_rows_group with the stochastic tail: the same exits, the same walks, the same row-wise butterfly.
template <int KIND, bool SEG>
__global__ __launch_bounds__(kBlock) void grad_sr_rows_group(RowArgs a, SegArgs sg, SrArgs sr, uint32_t lanes, uint32_t lanes_log2, uint32_t chunks) {
    static_assert(KIND == RES_SGD || KIND == RES_ADAGRAD || KIND == RES_ROWWISE, "a stepping kind");
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t i64 = gid >> lanes_log2;
    const uint32_t lg = (uint32_t)gid & (lanes - 1);
    if (i64 >= a.n || (KIND != RES_ROWWISE && lg >= chunks)) return;
    const uint32_t i = (uint32_t)i64;
    const uint32_t row = a.keys[i];
    if (row >= a.nr_rows || (i > 0 && a.keys[i - 1] == row)) return;      // (uniform over the lane group)
    const uint64_t t = sr_step_of(sr);
    if (KIND == RES_ROWWISE) {
        const bool own0 = lg < chunks, own1 = lg + lanes < chunks;        // (own1: beyond dim 256 only, where lanes == 64)
        float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f), acc1 = acc0;
        if (own0) acc0 = SEG ? seg_walk_piece(a, sg, i, row, lg, chunks) : walk_piece(a, i, row, lg);
        if (own1) acc1 = SEG ? seg_walk_piece(a, sg, i, row, lg + lanes, chunks) : walk_piece(a, i, row, lg + lanes);
        const float rate = rowwise_rate(a, row, lg, lanes, acc0, acc1, own1);
        if (own0) sr_step_piece<KIND>(a, sr.seed, t, row, lg, acc0, rate);
        if (own1) sr_step_piece<KIND>(a, sr.seed, t, row, lg + lanes, acc1, rate);
        return;
    }
    for (uint32_t c = lg; c < chunks; c += lanes) {
        const float4 acc = SEG ? seg_walk_piece(a, sg, i, row, c, chunks) : walk_piece(a, i, row, c);
        sr_step_piece<KIND>(a, sr.seed, t, row, c, acc, a.lr);
    }
}

// grad_rows_elem / grad_seg_rows_elem with the stochastic tail: the thread of element c runs the block of its piece c / 4 and takes
// word c % 4 -- the bits of the lane-group kernel.  (The word is chosen by selects: an indexed array would live in scratch.)
template <int KIND, bool SEG>
__global__ __launch_bounds__(kBlock) void grad_sr_rows_elem(RowArgs a, SrArgs sr, uint32_t S) {
    static_assert(KIND == RES_SGD || KIND == RES_ADAGRAD, "the element-wise kernel has no row-wide view of g");
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t i64 = gid / a.dim;
    const uint32_t c = (uint32_t)(gid - i64 * a.dim);
    if (i64 >= a.n) return;
    const uint32_t i = (uint32_t)i64;
    const uint32_t row = a.keys[i];
    if (row >= a.nr_rows || (i > 0 && a.keys[i - 1] == row)) return;
    float acc = 0.f, t = 0.f;
    uint32_t in_seg = 0;
    bool first = true;                           // (SEG) t_0 is taken as it is: the sum of the partials starts from it
    for (uint32_t j = i; j < a.n && a.keys[j] == row; j++) {
        const uint32_t p = min(a.vals[j], a.n - 1u);
        const uint32_t b = min(a.bagof[p], a.n_bags - 1u);
        const float cp = contribution(a.coef, a.grad[(uint64_t)b * a.ld + c], coef_of(a, p, b));
        if (!SEG) {
            acc = add_in_order(acc, cp);
            continue;
        }
        t = add_in_order(t, cp);
        if (++in_seg == S) {
            acc = first ? t : add_in_order(acc, t);
            first = false;
            t = 0.f;
            in_seg = 0;
        }
    }
    if (SEG && in_seg) acc = first ? t : add_in_order(acc, t);
    uint32_t R[4];
    sr_words(sr.seed, sr_step_of(sr), row, c >> 2, R);
    const uint32_t j = c & 3u;
    const uint32_t word = j == 0 ? R[0] : j == 1 ? R[1] : j == 2 ? R[2] : R[3];
    float *sp = KIND == RES_ADAGRAD ? a.state + (uint64_t)row * a.dim + c : nullptr;
    float st = KIND == RES_ADAGRAD ? *sp : 0.f;
    uint16_t *w = reinterpret_cast<uint16_t *>(a.table + (uint64_t)row * a.stride) + c;
    if (KIND == RES_ADAGRAD) *w = (uint16_t)adagrad_step_sr(a.dtype, *w, acc, &st, a.lr, a.eps, word);
    else *w = (uint16_t)step_sr(a.dtype, *w, acc, a.lr, word);
    if (KIND == RES_ADAGRAD) *sp = st;
}

}  // namespace

// The launch function libpimemb_grad_sr.so exports (plain C; RowArgs, SegArgs and SrArgs are this file's own, which every compilation
// lays out alike).  The hot launch of a stochastically rounded step (a chain of one): the lane-group kernel or the element-wise one, in
// the context's order.  kind: RES_SGD / RES_ADAGRAD / RES_ROWWISE.  Errors are left to the caller's hipGetLastError().
extern "C" __attribute__((visibility("default"))) void pimemb_grad_sr_launch(const void *row_args, const void *seg_args, const void *sr_args, int kind, int seg,
                                                                              int lane, uint32_t lanes, uint32_t lanes_log2, uint32_t chunks, uint32_t blocks,
                                                                              uint32_t elem_blocks, uint32_t S, void *stream) {
    const RowArgs &a = *static_cast<const RowArgs *>(row_args);
    const SegArgs &sg = *static_cast<const SegArgs *>(seg_args);
    const SrArgs &sr = *static_cast<const SrArgs *>(sr_args);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(kBlock);
    if (lane) {
        const dim3 grid(blocks);
        if (kind == RES_SGD && seg) grad_sr_rows_group<RES_SGD, true><<<grid, block, 0, s>>>(a, sg, sr, lanes, lanes_log2, chunks);
        else if (kind == RES_SGD) grad_sr_rows_group<RES_SGD, false><<<grid, block, 0, s>>>(a, sg, sr, lanes, lanes_log2, chunks);
        else if (kind == RES_ADAGRAD && seg) grad_sr_rows_group<RES_ADAGRAD, true><<<grid, block, 0, s>>>(a, sg, sr, lanes, lanes_log2, chunks);
        else if (kind == RES_ADAGRAD) grad_sr_rows_group<RES_ADAGRAD, false><<<grid, block, 0, s>>>(a, sg, sr, lanes, lanes_log2, chunks);
        else if (seg) grad_sr_rows_group<RES_ROWWISE, true><<<grid, block, 0, s>>>(a, sg, sr, lanes, lanes_log2, chunks);
        else grad_sr_rows_group<RES_ROWWISE, false><<<grid, block, 0, s>>>(a, sg, sr, lanes, lanes_log2, chunks);
        return;
    }
    const dim3 grid(elem_blocks);                // (the row-wise kind never gets here: the plan refused it)
    if (kind == RES_SGD && seg) grad_sr_rows_elem<RES_SGD, true><<<grid, block, 0, s>>>(a, sr, S);
    else if (kind == RES_SGD) grad_sr_rows_elem<RES_SGD, false><<<grid, block, 0, s>>>(a, sr, 0u);
    else if (seg) grad_sr_rows_elem<RES_ADAGRAD, true><<<grid, block, 0, s>>>(a, sr, S);
    else grad_sr_rows_elem<RES_ADAGRAD, false><<<grid, block, 0, s>>>(a, sr, 0u);
}

namespace {
#else      // libpimemb_grad.so (and the master unit, which never calls it): the launcher is libpimemb_grad_sr.so's
}  // namespace
extern "C" void pimemb_grad_sr_launch(const void *row_args, const void *seg_args, const void *sr_args, int kind, int seg, int lane, uint32_t lanes,
                                      uint32_t lanes_log2, uint32_t chunks, uint32_t blocks, uint32_t elem_blocks, uint32_t S, void *stream);
namespace {
#endif

// ---- the gradient of per_sample_weights: dw[p] = < G[bag(p)] , dec(W[ids[p]]) > (csrc/pimemb_grad_dot.h) ------------------------
// No pre-pass: nothing is sorted, a position's value depends on its own row and its bag's row of G alone.  The kernels above keep
// their text; these read the batch as the forward does.

struct PswArgs {
    const void *ids;
    const void *offsets;         // or NULL: bags of fixed_pooling positions
    const float *grad;           // G
    uint64_t ld;
    const char *table;
    float *dw;                   // [n]
    unsigned long long *bad;
    uint64_t pad_idx;
    uint32_t n, n_bags, nr_rows, dim;
    uint32_t stride;             // bytes from one table row to the next
    int dtype;
    uint32_t fixed_pooling, pad_on;
};

enum PswClass : int { PSW_GOOD = 0, PSW_BAD = 1, PSW_SKIP = 2, PSW_DEAD = 3 };      // (SKIP: padding or no bag; DEAD: no position)

// The id of position p (< n) at full width: an int64 id as its bits, a uint32 id zero-extended.
template <bool IDX64>
__device__ __forceinline__ uint64_t psw_load_id(const PswArgs &a, uint32_t p) {
    if (IDX64) return (uint64_t) static_cast<const long long *>(a.ids)[p];
    return static_cast<const uint32_t *>(a.ids)[p];
}

// A position in a bag with this id: good, bad or padding; *row = its table row where it is good.  Ids are compared at full width
// (a negative int64 id is a value of 2^63 or more here: outside every table).
__device__ __forceinline__ int psw_class_of(const PswArgs &a, uint64_t id, uint32_t *row) {
    const bool in_table = id < a.nr_rows;
    *row = in_table ? (uint32_t)id : 0u;
    if (a.pad_on && id == a.pad_idx) return PSW_SKIP;
    return in_table ? PSW_GOOD : PSW_BAD;
}

// offsets[b] (b < n_bags), clamped into [0, n]: whatever the offsets hold, a walk stays inside the batch.
template <bool IDX64>
__device__ __forceinline__ uint32_t psw_bag_start(const PswArgs &a, uint32_t b) {
    uint64_t o;
    if (!a.offsets) o = (uint64_t)b * a.fixed_pooling;
    else if (IDX64) o = (uint64_t) static_cast<const long long *>(a.offsets)[b];
    else o = static_cast<const uint32_t *>(a.offsets)[b];
    return o < a.n ? (uint32_t)o : a.n;
}

__device__ __forceinline__ float4 psw_dec(int, float4 w) { return w; }
__device__ __forceinline__ float4 psw_dec(int dtype, u32x2 w) {
    return make_float4(bits_f32(dec(dtype, w.x & 0xffffu)), bits_f32(dec(dtype, w.x >> 16)), bits_f32(dec(dtype, w.y & 0xffffu)),
                       bits_f32(dec(dtype, w.y >> 16)));
}

// t[c] of the definition from a piece of G and the decoded piece of the row
__device__ __forceinline__ float psw_piece(float4 g, float4 w) { return dot_fold4(dot_mul(g.x, w.x), dot_mul(g.y, w.y), dot_mul(g.z, w.z), dot_mul(g.w, w.w)); }

// The positions [start, end) of one bag, eight at a time.  A round's ids are in registers when it starts -- the loads of the NEXT
// round's ids are issued first and travel with this round's row gathers; then the row pieces of the good positions (RAW is a lane's
// 16 bytes of an fp32 row or its 8 bytes of an fp16 / bf16 row), all in flight before the first multiply; then the products and the
// fold per position, and the butterfly of the eight positions side by side: eight independent shuffles per xor distance.  A slot
// without a good position holds +0 and takes part.  Everything that branches is uniform over the lane group: its lanes reach
// every shuffle together, and the xor distances stay below `lanes`.
template <bool IDX64, typename RAW>
__device__ __forceinline__ void psw_walk(const PswArgs &a, uint32_t start, uint32_t end, uint32_t lg, uint32_t lanes, bool own0, bool own1, float4 g0,
                                         float4 g1) {
    uint64_t next[kAhead];
#pragma unroll
    for (uint32_t k = 0; k < kAhead; k++) next[k] = psw_load_id<IDX64>(a, start + k < end ? start + k : start);      // (start < end <= n)
    for (uint32_t j = start; j < end; j += kAhead) {
        int cls[kAhead];
        RAW w0[kAhead], w1[kAhead];
        uint32_t row[kAhead];
#pragma unroll
        for (uint32_t k = 0; k < kAhead; k++) {
            row[k] = 0;
            cls[k] = j + k < end ? psw_class_of(a, next[k], &row[k]) : (int)PSW_DEAD;
            const uint32_t p = j + kAhead + k;                            // (a slot beyond the bag re-reads the round's first id)
            next[k] = psw_load_id<IDX64>(a, p < end ? p : j);
        }
#pragma unroll
        for (uint32_t k = 0; k < kAhead; k++) {
            const RAW *r = reinterpret_cast<const RAW *>(a.table + (uint64_t)row[k] * a.stride);
            w0[k] = RAW{};
            w1[k] = RAW{};
            if (cls[k] == PSW_GOOD && own0) w0[k] = r[lg];
            if (cls[k] == PSW_GOOD && own1) w1[k] = r[lg + lanes];
        }
        float v[kAhead];
#pragma unroll
        for (uint32_t k = 0; k < kAhead; k++) {
            v[k] = 0.f;                                                   // (+0 in a lane without a piece, and for a position that is not good)
            if (cls[k] == PSW_GOOD && own0) v[k] = psw_piece(g0, psw_dec(a.dtype, w0[k]));
            if (cls[k] == PSW_GOOD && own1) v[k] = dot_add(v[k], psw_piece(g1, psw_dec(a.dtype, w1[k])));
        }
        for (uint32_t h = 1; h < lanes; h <<= 1) {
#pragma unroll
            for (uint32_t k = 0; k < kAhead; k++) v[k] = dot_add(v[k], __shfl_xor(v[k], (int)h));
        }
        if (lg == 0) {
#pragma unroll
            for (uint32_t k = 0; k < kAhead; k++) {
                if (cls[k] == PSW_DEAD) continue;
                a.dw[j + k] = cls[k] == PSW_GOOD ? v[k] : 0.f;
                if (cls[k] == PSW_BAD) atomicAdd(a.bad, 1ull);
            }
        }
    }
}

// One BAG per group of `lanes` lanes; lane lg owns the 16-byte pieces lg and lg + lanes (two only beyond dim 256) of G[b] and of
// every row the bag names.  The group of bag 0 also writes the +0 of the positions before offsets[0] (all of them where there is
// no bag at all: the launch has one group then).
template <bool IDX64>
__global__ __launch_bounds__(kBlock) void grad_psw_group(PswArgs a, uint32_t lanes, uint32_t lanes_log2, uint32_t chunks) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t b64 = gid >> lanes_log2;
    const uint32_t lg = (uint32_t)gid & (lanes - 1);
    if (b64 >= (a.n_bags ? a.n_bags : 1u)) return;
    const uint32_t b = (uint32_t)b64;
    const uint32_t start = a.n_bags ? psw_bag_start<IDX64>(a, b) : a.n;
    if (b == 0)
        for (uint32_t p = lg; p < start; p += lanes) a.dw[p] = 0.f;
    if (!a.n_bags) return;
    const uint32_t end = b + 1 < a.n_bags ? psw_bag_start<IDX64>(a, b + 1) : a.n;
    if (start >= end) return;                                             // (uniform over the lane group, like everything above)
    const bool own0 = lg < chunks, own1 = lg + lanes < chunks;
    const float4 *g = reinterpret_cast<const float4 *>(a.grad + (uint64_t)b * a.ld);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 g0 = own0 ? g[lg] : zero, g1 = own1 ? g[lg + lanes] : zero;
    if (a.dtype == kStepF32) psw_walk<IDX64, float4>(a, start, end, lg, lanes, own0, own1, g0, g1);
    else psw_walk<IDX64, u32x2>(a, start, end, lg, lanes, own0, own1, g0, g1);
}

// Any other shape: one POSITION per group of dot_lanes(dim) lanes, its bag by binary search, lane l the leaf v[l] of the tree with
// scalar element loads (dot_leaf: the text the host check compiles), then the same butterfly.
template <bool IDX64>
__global__ __launch_bounds__(kBlock) void grad_psw_elem(PswArgs a, uint32_t lanes, uint32_t lanes_log2) {
    const uint64_t gid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t p64 = gid >> lanes_log2;
    const uint32_t lg = (uint32_t)gid & (lanes - 1);
    if (p64 >= a.n) return;
    const uint32_t p = (uint32_t)p64;
    const uint32_t b = bag_of<IDX64>(a.offsets, a.fixed_pooling, a.n_bags, p);
    uint32_t row = 0;
    const int cls = b == kNoBag ? (int)PSW_SKIP : psw_class_of(a, psw_load_id<IDX64>(a, p), &row);      // (uniform over the lane group)
    if (cls != PSW_GOOD) {
        if (lg == 0) {
            a.dw[p] = 0.f;
            if (cls == PSW_BAD) atomicAdd(a.bad, 1ull);
        }
        return;
    }
    float v = dot_leaf(a.dtype, a.table + (uint64_t)row * a.stride, a.grad + (uint64_t)b * a.ld, a.dim, lg);
    for (uint32_t h = 1; h < lanes; h <<= 1) v = dot_add(v, __shfl_xor(v, (int)h));
    if (lg == 0) a.dw[p] = v;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
#ifndef PIMEMB_GRAD_KERNEL_UNIT      // (to the end of the file: the master and SR units hold kernels and their launchers alone)

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

#define GRAD_HIP(expr)                                                                          \
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

constexpr uint64_t kMaxIndices = 1ull << 30, kMaxBags = 0x7fffffffull, kCounterBytes = 256;
uint64_t up256(uint64_t b) { return (b + 255) & ~255ull; }
uint64_t tiles_of(uint64_t n) { return (n + kTile - 1) / kTile; }

// The scratch area: offsets of its pieces for a context of N indices and B bags.
struct Layout {
    uint64_t keys[2], vals[2], bagof, uidx, hist, sums, cnt, counters, partials, total;
};
// (seg_S == 0: the position order, whose area is what it was; otherwise the partial buffer of the segmented order lies behind it)
Layout layout_of(uint64_t N, uint64_t B, uint32_t seg_S = 0, uint32_t max_dim = 0) {
    if (N > kMaxIndices) N = kMaxIndices;
    if (B > kMaxBags) B = kMaxBags;
    if (N == 0) N = 1;
    Layout l{};
    uint64_t at = 0;
    auto take = [&](uint64_t bytes) {
        const uint64_t here = at;
        at += up256(bytes);
        return here;
    };
    l.keys[0] = take(N * 4);
    l.keys[1] = take(N * 4);
    l.vals[0] = take(N * 4);
    l.vals[1] = take(N * 4);
    l.bagof = take(N * 4);
    l.uidx = take(N * 4);
    const uint64_t hist_len = 256 * tiles_of(N);
    l.hist = take(hist_len * 4);
    l.sums = take((tiles_of(hist_len > N ? hist_len : N) + 1) * 4);
    l.cnt = take((B ? B : 1) * 4);
    l.counters = take(kCounterBytes);
    l.partials = at;
    if (seg_S) take(seg_buffer_bytes(N, seg_S, max_dim));
    l.total = at;
    return l;
}

}  // namespace

struct emb_grad {
    emb_engine *e = nullptr;
    int device = 0;
    uint64_t max_indices = 0, max_bags = 0;
    char *scratch = nullptr;
    Layout lay{};
    unsigned long long *counters = nullptr;      // [0] bad positions since the last report; [1] MXFP4 rows a master step could not encode
    emb_grad_config cfg{};                       // the order of additions of every call on this context
    uint32_t seg_log2 = 0;                       // EMB_GRAD_ORDER_SEGMENTED: log2 of cfg.segment
    bool segmented() const { return cfg.order == EMB_GRAD_ORDER_SEGMENTED; }
};

namespace {

// Everything that can be refused about a config; NULL text: it is fine.
const char *config_fault(const emb_grad_config *cfg) {
    if (!cfg) return "the config is NULL";
    if (cfg->reserved != 0) return "the config's reserved field must be 0";
    if (cfg->order == EMB_GRAD_ORDER_POSITION) return cfg->segment || cfg->max_dim ? "segment and max_dim must be 0 with EMB_GRAD_ORDER_POSITION" : nullptr;
    if (cfg->order != EMB_GRAD_ORDER_SEGMENTED) return "unknown order";
    if (!seg_length_ok(cfg->segment)) return "segment must be a power of two in 8 .. 1024";
    if (cfg->max_dim == 0) return "max_dim must be at least 1";
    return nullptr;
}

}  // namespace

extern "C" {

const char *emb_grad_last_error(void) { return t_err; }

uint64_t emb_grad_scratch_bytes(uint64_t max_indices, uint64_t max_bags) { return layout_of(max_indices, max_bags).total; }

uint64_t emb_grad_scratch_bytes_ex(uint64_t max_indices, uint64_t max_bags, const emb_grad_config *cfg) {
    if (config_fault(cfg)) return 0;
    return layout_of(max_indices, max_bags, cfg->order == EMB_GRAD_ORDER_SEGMENTED ? cfg->segment : 0u, cfg->max_dim).total;
}

int emb_grad_create(emb_engine *e, uint64_t max_indices, uint64_t max_bags, emb_grad **out) {
    const emb_grad_config position{EMB_GRAD_ORDER_POSITION, 0, 0, 0};
    return emb_grad_create_ex(e, max_indices, max_bags, &position, out);
}

int emb_grad_config_of(const emb_grad *g, emb_grad_config *out) {
    if (!g || !out) return fail(EMB_ERR_INVALID, "emb_grad_config_of: context or out is NULL");
    *out = g->cfg;
    return EMB_OK;
}

int emb_grad_create_ex(emb_engine *e, uint64_t max_indices, uint64_t max_bags, const emb_grad_config *cfg, emb_grad **out) {
    if (const char *fault = config_fault(cfg))
        return fail(EMB_ERR_INVALID, "emb_grad_create: %s (order %u, segment %u, max_dim %u, reserved %u)", fault, cfg ? cfg->order : 0u, cfg ? cfg->segment : 0u,
                    cfg ? cfg->max_dim : 0u, cfg ? cfg->reserved : 0u);
    if (!e || !out) return fail(EMB_ERR_INVALID, "emb_grad_create: engine or out is NULL");
    if (max_indices == 0 || max_indices > kMaxIndices) return fail(EMB_ERR_INVALID, "emb_grad_create: max_indices must be 1 .. 2^30");
    if (max_bags == 0 || max_bags > kMaxBags) return fail(EMB_ERR_INVALID, "emb_grad_create: max_bags must be 1 .. 2^31 - 1");
    int32_t dev = 0;
    if (int rc = emb_device_of(e, &dev)) return fail_engine(rc, "emb_grad_create");
    emb_grad *g = new emb_grad;
    g->e = e;
    g->device = dev;
    g->max_indices = max_indices;
    g->max_bags = max_bags;
    g->cfg = *cfg;
    g->seg_log2 = g->segmented() ? seg_log2(cfg->segment) : 0u;
    g->lay = layout_of(max_indices, max_bags, g->segmented() ? cfg->segment : 0u, cfg->max_dim);
    DeviceGuard guard(dev);
    void *p = nullptr;
    if (int rc = emb_device_alloc(e, g->lay.total, &p)) {
        delete g;
        return fail_engine(rc, "emb_grad_create");
    }
    g->scratch = static_cast<char *>(p);
    g->counters = reinterpret_cast<unsigned long long *>(g->scratch + g->lay.counters);
    const hipError_t err = hipMemset(g->counters, 0, kCounterBytes);
    if (err != hipSuccess) {
        fail(EMB_ERR_DEVICE, "emb_grad_create: %s", hipGetErrorString(err));
        (void)emb_grad_destroy(g);
        return EMB_ERR_DEVICE;
    }
    *out = g;
    return EMB_OK;
}

int emb_grad_destroy(emb_grad *g) {
    if (!g) return EMB_OK;
    DeviceGuard guard(g->device);
    (void)hipDeviceSynchronize();
    if (g->scratch) (void)emb_device_free(g->e, g->scratch);
    delete g;
    return EMB_OK;
}

}  // extern "C"

namespace {

struct TableShape {
    char *rows;
    uint64_t nr_rows;
    uint32_t dim;
    int dtype;
    uint32_t stride;
};

// Everything that can be refused about one descriptor, before anything is enqueued.
int check_desc(emb_grad *g, const emb_grad_desc &d, emb_index_type itype, const char *step /* "an SGD", "an Adagrad"; NULL: no step */, const char *who, TableShape *t) {
    void *rows = nullptr;
    emb_dtype dt;
    if (int rc = emb_table_info(g->e, d.table_id, &rows, &t->nr_rows, &t->dim, &dt)) return fail_engine(rc, who);
    __builtin_memcpy(&t->dtype, &dt, sizeof(int));      // (the fp8 / MXFP4 values lie outside the enum's range: pimemb.h)
    t->rows = static_cast<char *>(rows);
    if (t->dtype == kFixed32) return fail(EMB_ERR_UNSUPPORTED, "%s: table %u is EMB_FIXED32: a fixed-point table has no gradient here", who, d.table_id);
    if (g->segmented() && t->dim > g->cfg.max_dim)
        return fail(EMB_ERR_INVALID, "%s: table %u has dim %u, the context's segmented order was created for a max_dim of %u", who, d.table_id, t->dim,
                    g->cfg.max_dim);
    if (d.pool.mode == EMB_POOL_MAX)
        return fail(EMB_ERR_UNSUPPORTED, "%s: EMB_POOL_MAX needs the forward's per-element argmax, which no kernel records", who);
    if (d.pool.mode != EMB_POOL_SUM && d.pool.mode != EMB_POOL_MEAN) return fail(EMB_ERR_INVALID, "%s: unknown pooling mode %u", who, d.pool.mode);
    if (d.pool.flags & ~EMB_POOL_PADDING) return fail(EMB_ERR_INVALID, "%s: pooling flag bits 0x%x have no meaning here", who, d.pool.flags & ~EMB_POOL_PADDING);
    if (d.pool.per_sample_weights && d.pool.mode != EMB_POOL_SUM) return fail(EMB_ERR_INVALID, "%s: per_sample_weights go with EMB_POOL_SUM only", who);
    if ((d.pool.flags & EMB_POOL_PADDING) && (d.pool.padding_idx < 0 || (uint64_t)d.pool.padding_idx >= t->nr_rows))
        return fail(EMB_ERR_INVALID, "%s: padding_idx %lld lies outside table %u", who, (long long)d.pool.padding_idx, d.table_id);
    if (step) {
        if (t->dtype != kF32 && t->dtype != kF16 && t->dtype != kBF16)
            return fail(EMB_ERR_UNSUPPORTED,
                        "%s: table %u is fp8 or MXFP4: %s step in the stored precision mostly rounds away (and an MXFP4 block shares "
                        "its scale); keep fp32 master rows, take emb_grad_sparse and write rows with emb_rows_update", who, d.table_id, step);
        uint32_t n_hot = 0;
        if (int rc = emb_table_hot_count(g->e, d.table_id, &n_hot)) return fail_engine(rc, who);
        if (n_hot)
            return fail(EMB_ERR_UNSUPPORTED,
                        "%s: table %u has a hot set of %u rows staged, a copy taken when it was set that lookups would go on serving: "
                        "clear the set (emb_set_hot_rows with n_rows = 0), step, then set it again", who, d.table_id, n_hot);
    }
    t->stride = t->dim * (t->dtype == kF32 ? 4u : 2u);      // (used by the step only)
    if (t->nr_rows >= 0xffffffffull) return fail(EMB_ERR_UNSUPPORTED, "%s: table %u has 2^32 - 1 rows or more", who, d.table_id);
    if (d.n_indices > g->max_indices)
        return fail(EMB_ERR_INVALID, "%s: %llu indices in one call, the context was created for %llu", who, (unsigned long long)d.n_indices,
                    (unsigned long long)g->max_indices);
    if (d.n_bags > g->max_bags)
        return fail(EMB_ERR_INVALID, "%s: %llu bags in one call, the context was created for %llu", who, (unsigned long long)d.n_bags,
                    (unsigned long long)g->max_bags);
    if (d.n_indices == 0) return EMB_OK;
    if (!d.indices || !d.grad) return fail(EMB_ERR_INVALID, "%s: indices or grad is NULL", who);
    if (!d.offsets && d.fixed_pooling == 0) return fail(EMB_ERR_INVALID, "%s: offsets is NULL and fixed_pooling is 0", who);
    if (d.grad_ld < t->dim) return fail(EMB_ERR_INVALID, "%s: grad_ld %llu is below the table's dim %u", who, (unsigned long long)d.grad_ld, t->dim);
    const size_t isz = itype == EMB_IDX_I64 ? 8 : 4;
    if ((uintptr_t)d.indices % isz || (uintptr_t)d.offsets % isz || (uintptr_t)d.grad % 4 || (uintptr_t)d.pool.per_sample_weights % 4)
        return fail(EMB_ERR_INVALID, "%s: indices, offsets, grad and weights must be naturally aligned", who);
    return EMB_OK;
}

struct StepSpec {
    int kind = RES_SPARSE;       // ResultKind
    float lr = 0.f, eps = 0.f;
    float *const *masters = nullptr;      // emb_grad_master_step: one fp32 master per descriptor; the kind's master tail runs
    const emb_sr_spec *sr = nullptr;      // emb_grad_sgd_sr / emb_grad_step_sr: the kind's stochastically rounded tail runs
};
struct SparseOut {               // where emb_grad_sparse writes; all NULL for a step (no unique numbering, no output arrays)
    long long *rows = nullptr;
    float *grads = nullptr;
    unsigned long long *n_unique = nullptr;
};

// THE predicate for "this descriptor runs on the lane-group kernel" (for RES_ROWWISE: whether it runs at all).  Evaluated once per
// descriptor, into Planned::lane: the row-wise refusal, emb_grad_multi_shape::lane_group and the chain's kernel all read that.
bool lane_group_path(const emb_grad_desc &d, const TableShape &t, int kind, const float *state, const float *grads_out) {
    return t.dim % 4 == 0 && t.dim <= 512 && d.grad_ld % 4 == 0 && (uintptr_t)d.grad % 16 == 0 &&
           (kind != RES_SPARSE || (uintptr_t)grads_out % 16 == 0) && (kind != RES_ADAGRAD || (uintptr_t)state % 16 == 0);
}

// The lane-group kernels' launch: a lane per 16-byte piece of a row, in groups of a power of two up to 64.
struct LaneGeom {
    uint32_t chunks, lanes, lanes_log2, blocks;
};
LaneGeom lane_geom(uint32_t dim, uint32_t n) {
    LaneGeom l{dim / 4, 1, 0, 0};
    for (; l.lanes < l.chunks && l.lanes < 64; l.lanes <<= 1) l.lanes_log2++;
    l.blocks = (uint32_t)(((uint64_t)n * l.lanes + kBlock - 1) / kBlock);      // (n <= 2^30, 64 lanes: below 2^28)
    return l;
}

// What the kernels take of a descriptor's emb_pool_spec: grad_classify's arguments, RowArgs and MultiDesc are filled from this.
struct PoolArgs {
    uint32_t coef, pad_on;       // CoefMode; 1: padding_idx is in use
    uint64_t pad_idx;
};
PoolArgs pool_args(const emb_grad_desc &d) {
    const bool pad = (d.pool.flags & EMB_POOL_PADDING) != 0;
    const uint32_t coef = d.pool.mode == EMB_POOL_MEAN ? COEF_MEAN : d.pool.per_sample_weights ? COEF_WEIGHTED : COEF_SUM;
    return PoolArgs{coef, pad ? 1u : 0u, pad ? (uint64_t)d.pool.padding_idx : 0ull};
}

// ---- phase one, the plan: no device work, and everything that can refuse a call -------------------------------------------------

// One descriptor of a call, and the launch chain that STARTS at it (k == 0: none does): the cnt memset, classify, the sort, the head
// scan (sparse) and the hot launch over the k non-empty descriptors of [this one, end) -- one, or a group's 2 .. 16.
struct Planned {
    TableShape t;
    bool lane;                   // lane_group_path of this descriptor, and so the chain's kernel (the members of a group all have it)
    bool mean;                   // a member pools by mean: cnt[] is cleared and counted
    uint32_t k, end;
    uint32_t n, n_bags, key_end; // positions, bags and rows summed over the members; key_end is the key of a position that is not good
    LaneGeom geo;                // lane: the hot launch
    uint32_t elem_blocks;        // !lane: its workgroups
};

// Plans the chain of the non-empty descriptors of [first, end): one descriptor, or a group as emb_grad_multi_groups made it.
int plan_chain(const emb_grad *g, const emb_grad_desc *descs, Planned *p, uint32_t first, uint32_t end) {
    Planned &c = p[first];
    uint64_t pos = 0, bags = 0, keys_end = 0;
    bool fusable = true;
    for (uint32_t j = first; j < end; j++) {
        if (descs[j].n_indices == 0) continue;
        c.k++;
        pos += descs[j].n_indices;
        bags += descs[j].n_bags;
        keys_end += p[j].t.nr_rows;
        fusable = fusable && p[j].lane && p[j].t.dim == c.t.dim;
        c.mean = c.mean || pool_args(descs[j]).coef == COEF_MEAN;
    }
    if (c.k > 1 && (c.k > kMultiMax || !fusable || pos > g->max_indices || bags > g->max_bags || keys_end > 0xfffffffeull))
        return fail(EMB_ERR_INVALID, "emb_grad: a group of %u descriptors, %llu indices, %llu bags and %llu rows does not fit", c.k, (unsigned long long)pos,
                    (unsigned long long)bags, (unsigned long long)keys_end);      // (emb_grad_multi_groups makes no such group)
    c.end = end;
    c.n = (uint32_t)pos;         // (one descriptor: check_desc kept these within the context, and nr_rows below 2^32 - 1)
    c.n_bags = (uint32_t)bags;
    c.key_end = (uint32_t)keys_end;
    if (c.lane) {
        c.geo = lane_geom(c.t.dim, c.n);
        return EMB_OK;
    }
    const uint64_t blocks = ((uint64_t)c.n * c.t.dim + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffull)
        return fail(EMB_ERR_UNSUPPORTED, "emb_grad: %u indices of dim %u are more elements than one launch of the element-wise kernel takes", c.n, c.t.dim);
    c.elem_blocks = (uint32_t)blocks;
    return EMB_OK;
}

// The plan of a step call: every descriptor and state checked, in order; then the chains -- one per non-empty descriptor, or one per
// group (ms != NULL: the multi calls; ms and group_of have n_descs entries like `plan`).
int plan_step(emb_grad *g, const emb_grad_desc *descs, float *const *states, uint32_t n_descs, emb_index_type itype, const StepSpec &spec, const char *step,
              const char *who, Planned *plan, emb_grad_multi_shape *ms, uint32_t *group_of) {
    for (uint32_t k = 0; k < n_descs; k++) {
        const emb_grad_desc &d = descs[k];
        Planned &p = plan[k];
        if (int rc = check_desc(g, d, itype, step, who, &p.t)) return rc;
        if (spec.sr && p.t.dtype == kF32)
            return fail(EMB_ERR_UNSUPPORTED, "%s: table %u is EMB_F32: an fp32 step stores its fp32 result, there is nothing to round -- use %s", who,
                        d.table_id, spec.kind == RES_SGD ? "emb_grad_sgd" : "emb_grad_step");
        float *state = d.n_indices && states ? states[k] : nullptr;
        if (d.n_indices && spec.kind != RES_SGD && (!state || (uintptr_t)state % 4))
            return fail(EMB_ERR_INVALID, "%s: the state of table %u is NULL or not 4-byte aligned", who, d.table_id);
        p.lane = lane_group_path(d, p.t, spec.kind, state, nullptr);
        if (d.n_indices && spec.kind == RES_ROWWISE && !p.lane)
            return fail(EMB_ERR_UNSUPPORTED,
                        "%s: row-wise Adagrad needs the lane-group shape (dim %% 4 == 0, dim <= 512, grad 16-byte aligned, grad_ld %% 4 == 0): table %u "
                        "has dim %u, grad %p, grad_ld %llu -- the element-wise kernel has no row-wide view of g", who, d.table_id, p.t.dim,
                        (const void *)d.grad, (unsigned long long)d.grad_ld);
        if (ms) ms[k] = emb_grad_multi_shape{d.table_id, p.t.dim, p.lane ? 1u : 0u, p.t.nr_rows, d.n_indices, d.n_bags};
    }
    if (ms) emb_grad_multi_groups(ms, n_descs, g->max_indices, g->max_bags, group_of);
    for (uint32_t k = 0, end; k < n_descs; k = end) {
        end = k + 1;             // (a group's members are consecutive but for the empty descriptors among them)
        if (descs[k].n_indices == 0) continue;
        while (ms && end < n_descs && (group_of[end] == group_of[k] || descs[end].n_indices == 0)) end++;
        if (int rc = plan_chain(g, descs, plan, k, end)) return rc;
    }
    return EMB_OK;
}

// ---- phase two, the enqueue: from the first launch on, the only possible failure is a HIP error ---------------------------------

struct Scratch {                 // the scratch area as the kernels take it
    uint32_t *keys[2], *vals[2], *bagof, *uidx, *hist, *sums, *cnt;
};
Scratch scratch_of(const emb_grad *g) {
    const Layout &l = g->lay;
    auto at = [g](uint64_t off) { return reinterpret_cast<uint32_t *>(g->scratch + off); };
    return Scratch{{at(l.keys[0]), at(l.keys[1])}, {at(l.vals[0]), at(l.vals[1])}, at(l.bagof), at(l.uidx), at(l.hist), at(l.sums), at(l.cnt)};
}

// The stable sort of the n (key, position) pairs in keys[0] / vals[0], the keys running up to key_end itself: four launches per 8
// bits of key_end.  *cur = which of the two buffers holds the result.
int sort_pairs(const Scratch &sc, uint32_t n, uint32_t key_end, hipStream_t s, int *cur) {
    uint32_t bits = 0;
    while (bits < 32 && ((uint64_t)key_end >> bits) != 0) bits++;
    const uint32_t tiles = (uint32_t)tiles_of(n), hist_len = 256u * tiles, hist_chunks = (uint32_t)tiles_of(hist_len);
    int c = 0;
    for (uint32_t shift = 0; shift < bits; shift += 8, c ^= 1) {
        grad_sort_count<<<dim3(tiles), dim3(kBlock), 0, s>>>(sc.keys[c], n, shift, sc.hist, tiles);
        grad_scan_chunks<false><<<dim3(hist_chunks), dim3(kBlock), 0, s>>>(sc.hist, hist_len, 0u, sc.hist, sc.sums);
        grad_scan_sums<<<dim3(1), dim3(kBlock), 0, s>>>(sc.sums, hist_chunks, (unsigned long long *)nullptr);
        grad_sort_scatter<<<dim3(tiles), dim3(kBlock), 0, s>>>(sc.keys[c], sc.vals[c], sc.keys[c ^ 1], sc.vals[c ^ 1], n, shift, sc.hist, sc.sums, tiles);
        GRAD_HIP(hipGetLastError());
    }
    *cur = c;
    return EMB_OK;
}

// The records of the group planned at descriptor `first`: positions, bags and keys of its members laid end to end.
void fill_multi(MultiArgs &m, const emb_grad_desc *descs, float *const *states, const Planned *p, uint32_t first) {
    const Planned &c = p[first];
    m = MultiArgs{};
    m.k = c.k, m.n = c.n, m.key_end = c.key_end, m.dim = c.t.dim;
    uint32_t pos = 0, bags = 0, key = 0, j = 0;
    for (uint32_t at = first; at < c.end; at++) {
        const emb_grad_desc &d = descs[at];
        if (d.n_indices == 0) continue;
        const TableShape &t = p[at].t;
        const PoolArgs pa = pool_args(d);
        MultiDesc &r = m.d[j++];
        r.ids = d.indices, r.offsets = d.offsets, r.fixed_pooling = d.fixed_pooling;
        r.weights = d.pool.per_sample_weights, r.coef = pa.coef, r.pad_on = pa.pad_on, r.pad_idx = pa.pad_idx;
        r.grad = d.grad, r.ld = d.grad_ld;
        r.table = t.rows, r.stride = t.stride, r.dtype = t.dtype;
        r.state = states ? states[at] : nullptr;
        r.pos_base = pos, r.n = (uint32_t)d.n_indices;
        r.bag_base = bags, r.n_bags = (uint32_t)d.n_bags;
        r.key_base = key, r.nr_rows = (uint32_t)t.nr_rows;
        pos += r.n, bags += r.n_bags, key += r.nr_rows;
    }
}

// Runs the chain planned at descriptor `first`, for a chain of one and for a group alike.
int run_chain(emb_grad *g, const emb_grad_desc *descs, float *const *states, const Planned *p, uint32_t first, bool idx64, const StepSpec &spec,
              const SparseOut &out, hipStream_t s) {
    const Planned &c = p[first];
    const emb_grad_desc &d = descs[first];       // (a chain of one: its descriptor)
    const PoolArgs pa = pool_args(d);
    const Scratch sc = scratch_of(g);
    const LaneGeom &l = c.geo;
    const bool group = c.k > 1;
    const uint32_t n = c.n;
    const dim3 block(kBlock), pos_grid((n + kBlock - 1) / kBlock);
    unsigned long long *bad = &g->counters[0];
    MultiArgs m;                                 // (filled for a group only)
    if (c.mean && c.n_bags && (spec.masters || spec.sr)) pimemb_grad_master_clear(sc.cnt, c.n_bags, s);      // (a kernel: the note at grad_master_clear)
    else if (c.mean && c.n_bags) GRAD_HIP(hipMemsetAsync(sc.cnt, 0, (size_t)c.n_bags * 4, s));
    if (group) {
        fill_multi(m, descs, states, p, first);
        if (idx64) grad_multi_classify<true><<<pos_grid, block, 0, s>>>(m, sc.keys[0], sc.vals[0], sc.bagof, sc.cnt, bad);
        else grad_multi_classify<false><<<pos_grid, block, 0, s>>>(m, sc.keys[0], sc.vals[0], sc.bagof, sc.cnt, bad);
    } else {
        uint32_t *cnt = c.mean ? sc.cnt : nullptr;
        if (idx64)
            grad_classify<true><<<pos_grid, block, 0, s>>>(d.indices, d.offsets, d.fixed_pooling, n, c.n_bags, c.key_end, pa.pad_on, pa.pad_idx, sc.keys[0],
                                                          sc.vals[0], sc.bagof, cnt, bad);
        else
            grad_classify<false><<<pos_grid, block, 0, s>>>(d.indices, d.offsets, d.fixed_pooling, n, c.n_bags, c.key_end, pa.pad_on, pa.pad_idx, sc.keys[0],
                                                           sc.vals[0], sc.bagof, cnt, bad);
    }
    GRAD_HIP(hipGetLastError());
    int cur = 0;
    if (int rc = sort_pairs(sc, n, c.key_end, s, &cur)) return rc;
    const uint32_t *keys = sc.keys[cur], *vals = sc.vals[cur];
    const bool seg = g->segmented();
    SegArgs sg{};                                // (filled for the lane-group kernels of a segmented context only)
    if (seg && c.lane) {
        sg.partials = reinterpret_cast<float4 *>(g->scratch + g->lay.partials);
        sg.S = g->cfg.segment, sg.S_log2 = g->seg_log2;
        sg.n_slots = (uint32_t)seg_slots(g->max_indices, sg.S);      // (l.chunks <= seg_pieces(max_dim): check_desc; max_indices <= 2^30)
    }
    if (group && seg) {
        const dim3 grid(l.blocks);
        grad_seg_multi_partials<<<grid, block, 0, s>>>(m, keys, vals, sc.bagof, sc.cnt, sg, l.lanes, l.lanes_log2, l.chunks);
        if (spec.kind == RES_SGD)
            grad_seg_multi_rows<RES_SGD><<<grid, block, 0, s>>>(m, keys, vals, sc.bagof, sc.cnt, spec.lr, spec.eps, sg, l.lanes, l.lanes_log2, l.chunks);
        else if (spec.kind == RES_ADAGRAD)
            grad_seg_multi_rows<RES_ADAGRAD><<<grid, block, 0, s>>>(m, keys, vals, sc.bagof, sc.cnt, spec.lr, spec.eps, sg, l.lanes, l.lanes_log2, l.chunks);
        else grad_seg_multi_rows<RES_ROWWISE><<<grid, block, 0, s>>>(m, keys, vals, sc.bagof, sc.cnt, spec.lr, spec.eps, sg, l.lanes, l.lanes_log2, l.chunks);
        GRAD_HIP(hipGetLastError());
        return EMB_OK;
    }
    if (group) {
        const dim3 grid(l.blocks);
        if (spec.kind == RES_SGD) grad_multi_rows<RES_SGD><<<grid, block, 0, s>>>(m, keys, vals, sc.bagof, sc.cnt, spec.lr, spec.eps, l.lanes, l.lanes_log2, l.chunks);
        else if (spec.kind == RES_ADAGRAD)
            grad_multi_rows<RES_ADAGRAD><<<grid, block, 0, s>>>(m, keys, vals, sc.bagof, sc.cnt, spec.lr, spec.eps, l.lanes, l.lanes_log2, l.chunks);
        else grad_multi_rows<RES_ROWWISE><<<grid, block, 0, s>>>(m, keys, vals, sc.bagof, sc.cnt, spec.lr, spec.eps, l.lanes, l.lanes_log2, l.chunks);
        GRAD_HIP(hipGetLastError());
        return EMB_OK;
    }
    RowArgs a{};
    a.keys = keys, a.vals = vals, a.bagof = sc.bagof, a.cnt = sc.cnt;
    a.weights = d.pool.per_sample_weights, a.coef = pa.coef;
    a.grad = d.grad, a.ld = d.grad_ld;
    a.n = n, a.n_bags = c.n_bags, a.nr_rows = c.key_end, a.dim = c.t.dim;
    if (spec.kind != RES_SPARSE) {
        a.table = c.t.rows, a.stride = c.t.stride, a.dtype = c.t.dtype;
        a.lr = spec.lr, a.eps = spec.eps, a.state = states ? states[first] : nullptr;
    } else {
        const uint32_t tiles = (uint32_t)tiles_of(n);
        grad_scan_chunks<true><<<dim3(tiles), block, 0, s>>>(keys, n, c.key_end, sc.uidx, sc.sums);
        grad_scan_sums<<<dim3(1), block, 0, s>>>(sc.sums, tiles, out.n_unique);
        GRAD_HIP(hipGetLastError());
        a.uidx = sc.uidx, a.usums = sc.sums, a.rows_out = out.rows, a.grads_out = out.grads;
    }
    if (spec.masters) {
        if (seg && c.lane) grad_seg_partials<<<dim3(l.blocks), block, 0, s>>>(a, sg, l.lanes, l.lanes_log2, l.chunks);
        const MasterArgs ma{spec.masters[first], c.t.dtype, &g->counters[1]};
        pimemb_grad_master_launch(&a, &sg, &ma, spec.kind, seg, c.lane, l.lanes, l.lanes_log2, l.chunks, l.blocks, c.elem_blocks, g->cfg.segment, s);
        GRAD_HIP(hipGetLastError());
        return EMB_OK;
    }
    if (spec.sr) {
        if (seg && c.lane) grad_seg_partials<<<dim3(l.blocks), block, 0, s>>>(a, sg, l.lanes, l.lanes_log2, l.chunks);
        const SrArgs sr{spec.sr->seed, spec.sr->step + first, spec.sr->step_dev};      // (descriptor k of the call: t = step + *step_dev + k, mod 2^64)
        pimemb_grad_sr_launch(&a, &sg, &sr, spec.kind, seg, c.lane, l.lanes, l.lanes_log2, l.chunks, l.blocks, c.elem_blocks, g->cfg.segment, s);
        GRAD_HIP(hipGetLastError());
        return EMB_OK;
    }
    if (seg && c.lane) {
        const dim3 grid(l.blocks);
        grad_seg_partials<<<grid, block, 0, s>>>(a, sg, l.lanes, l.lanes_log2, l.chunks);
        if (spec.kind == RES_SGD) grad_seg_rows_group<RES_SGD><<<grid, block, 0, s>>>(a, sg, l.lanes, l.lanes_log2, l.chunks);
        else if (spec.kind == RES_ADAGRAD) grad_seg_rows_group<RES_ADAGRAD><<<grid, block, 0, s>>>(a, sg, l.lanes, l.lanes_log2, l.chunks);
        else if (spec.kind == RES_ROWWISE) grad_seg_rows_group<RES_ROWWISE><<<grid, block, 0, s>>>(a, sg, l.lanes, l.lanes_log2, l.chunks);
        else grad_seg_rows_group<RES_SPARSE><<<grid, block, 0, s>>>(a, sg, l.lanes, l.lanes_log2, l.chunks);
    } else if (seg) {
        const dim3 grid(c.elem_blocks);
        if (spec.kind == RES_SGD) grad_seg_rows_elem<RES_SGD><<<grid, block, 0, s>>>(a, g->cfg.segment);
        else if (spec.kind == RES_ADAGRAD) grad_seg_rows_elem<RES_ADAGRAD><<<grid, block, 0, s>>>(a, g->cfg.segment);
        else grad_seg_rows_elem<RES_SPARSE><<<grid, block, 0, s>>>(a, g->cfg.segment);
    } else if (c.lane) {
        const dim3 grid(l.blocks);
        if (spec.kind == RES_SGD) grad_rows_group<RES_SGD><<<grid, block, 0, s>>>(a, l.lanes, l.lanes_log2, l.chunks);
        else if (spec.kind == RES_ADAGRAD) grad_rows_group<RES_ADAGRAD><<<grid, block, 0, s>>>(a, l.lanes, l.lanes_log2, l.chunks);
        else if (spec.kind == RES_ROWWISE) grad_rows_group<RES_ROWWISE><<<grid, block, 0, s>>>(a, l.lanes, l.lanes_log2, l.chunks);
        else grad_rows_group<RES_SPARSE><<<grid, block, 0, s>>>(a, l.lanes, l.lanes_log2, l.chunks);
    } else {
        const dim3 grid(c.elem_blocks);
        if (spec.kind == RES_SGD) grad_rows_elem<RES_SGD><<<grid, block, 0, s>>>(a);
        else if (spec.kind == RES_ADAGRAD) grad_rows_elem<RES_ADAGRAD><<<grid, block, 0, s>>>(a);
        else grad_rows_elem<RES_SPARSE><<<grid, block, 0, s>>>(a);      // (RES_ROWWISE never gets here: the plan refused it)
    }
    GRAD_HIP(hipGetLastError());
    return EMB_OK;
}

// The plan of emb_grad_master_step: every descriptor, master and state checked, in order; then one chain per non-empty descriptor.
int plan_master(emb_grad *g, const emb_grad_desc *descs, float *const *masters, float *const *states, uint32_t n_descs, emb_index_type itype,
                const StepSpec &spec, const char *who, Planned *plan) {
    for (uint32_t k = 0; k < n_descs; k++) {
        const emb_grad_desc &d = descs[k];
        Planned &p = plan[k];
        TableShape &t = p.t;
        if (int rc = check_desc(g, d, itype, nullptr, who, &t)) return rc;
        if (t.dtype == kF32)
            return fail(EMB_ERR_UNSUPPORTED, "%s: table %u is EMB_F32: the table is its own master, use emb_grad_sgd / emb_grad_step", who, d.table_id);
        if (t.dtype != kMasterF16 && t.dtype != kMasterBF16 && t.dtype != kMasterE4M3 && t.dtype != kMasterE5M2 && t.dtype != kMasterMXFP4)
            return fail(EMB_ERR_UNSUPPORTED, "%s: table %u has dtype %d, which no master step encodes", who, d.table_id, t.dtype);
        uint32_t n_hot = 0;
        if (int rc = emb_table_hot_count(g->e, d.table_id, &n_hot)) return fail_engine(rc, who);
        if (n_hot)
            return fail(EMB_ERR_UNSUPPORTED,
                        "%s: table %u has a hot set of %u rows staged, a copy taken when it was set that lookups would go on serving: "
                        "clear the set (emb_set_hot_rows with n_rows = 0), step, then set it again", who, d.table_id, n_hot);
        const bool mx = t.dtype == kMasterMXFP4;
        if (mx && t.dim > 512) return fail(EMB_ERR_UNSUPPORTED, "%s: table %u is MXFP4 of dim %u, the master step takes MXFP4 rows up to dim 512", who, d.table_id, t.dim);
        t.stride = mx ? EMB_MXFP4_ROW_STRIDE(t.dim) : t.dim * (t.dtype == kMasterF16 || t.dtype == kMasterBF16 ? 2u : 1u);
        float *master = d.n_indices ? masters[k] : nullptr;
        if (d.n_indices && (!master || (uintptr_t)master % 4))
            return fail(EMB_ERR_INVALID, "%s: the master of table %u is NULL or not 4-byte aligned", who, d.table_id);
        float *state = d.n_indices && states ? states[k] : nullptr;
        if (d.n_indices && spec.kind != RES_SGD && (!state || (uintptr_t)state % 4))
            return fail(EMB_ERR_INVALID, "%s: the state of table %u is NULL or not 4-byte aligned", who, d.table_id);
        p.lane = lane_group_path(d, t, spec.kind, state, nullptr) && (uintptr_t)master % 16 == 0;
        if (d.n_indices && !p.lane && (spec.kind == RES_ROWWISE || mx))
            return fail(EMB_ERR_UNSUPPORTED,
                        "%s: %s needs the lane-group shape (dim %% 4 == 0, dim <= 512, grad and master 16-byte aligned, grad_ld %% 4 == 0): table %u has "
                        "dim %u, grad %p, grad_ld %llu, master %p -- the element-wise kernel has no row-wide or block-wide view", who,
                        mx ? "an MXFP4 table" : "row-wise Adagrad", d.table_id, t.dim, (const void *)d.grad, (unsigned long long)d.grad_ld, (const void *)master);
    }
    for (uint32_t k = 0; k < n_descs; k++)
        if (descs[k].n_indices)
            if (int rc = plan_chain(g, descs, plan, k, k + 1)) return rc;
    return EMB_OK;
}

// What emb_grad_sgd(_multi) and emb_grad_step(_multi) share once their arguments are checked: the plan of the whole call, then chain
// after chain enqueued.
int step_call(emb_grad *g, const emb_grad_desc *descs, float *const *states, uint32_t n_descs, emb_index_type itype, const StepSpec &spec,
              const char *step, const char *who, bool multi, void *stream) {
    const bool sgd = spec.kind == RES_SGD;       // (no states)
    if (!g) return fail(EMB_ERR_INVALID, "%s: context is NULL", who);
    if (n_descs && (!descs || (!sgd && !states))) return fail(EMB_ERR_INVALID, "%s: %s is NULL", who, sgd ? "descs" : "descs or states");
    if (itype != EMB_IDX_U32 && itype != EMB_IDX_I64) return fail(EMB_ERR_INVALID, "%s: bad index type", who);
    std::vector<Planned> plan(n_descs);
    std::vector<emb_grad_multi_shape> ms(multi ? n_descs : 0);
    std::vector<uint32_t> group_of(multi ? n_descs : 0);
    if (int rc = plan_step(g, descs, states, n_descs, itype, spec, step, who, plan.data(), multi ? ms.data() : nullptr, group_of.data())) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(g->device);
    for (uint32_t k = 0; k < n_descs; k++)
        if (plan[k].k)
            if (int rc = run_chain(g, descs, states, plan.data(), k, itype == EMB_IDX_I64, spec, SparseOut{}, s)) return rc;
    return EMB_OK;
}

}  // namespace

extern "C" {

uint32_t emb_grad_multi_groups(const emb_grad_multi_shape *shapes, uint32_t n, uint64_t max_indices, uint64_t max_bags, uint32_t *group_of) {
    uint32_t groups = 0, first = 0, members = 0;      // the open group: its number is groups - 1, it began at `first`
    uint64_t idx = 0, bags = 0, rows = 0;
    bool open_fusable = false;
    for (uint32_t k = 0; shapes && k < n; k++) {
        const emb_grad_multi_shape &c = shapes[k];
        if (c.n_indices == 0) {
            if (group_of) group_of[k] = 0xffffffffu;
            continue;
        }
        bool join = members > 0 && open_fusable && c.lane_group && c.dim == shapes[first].dim && members < EMB_GRAD_MULTI_MAX &&
                    idx + c.n_indices <= max_indices && bags + c.n_bags <= max_bags && rows + c.nr_rows <= 0xfffffffeull;
        for (uint32_t j = first; join && j < k; j++)
            if (shapes[j].n_indices != 0 && shapes[j].table_id == c.table_id) join = false;
        if (!join) {
            groups++;
            first = k;
            members = 0;
            idx = bags = rows = 0;
            open_fusable = c.lane_group != 0;
        }
        members++;
        idx += c.n_indices;
        bags += c.n_bags;
        rows += c.nr_rows;
        if (group_of) group_of[k] = groups - 1;
    }
    return groups;
}

int emb_grad_sparse(emb_grad *g, const emb_grad_desc *desc, emb_index_type itype, int64_t *rows_out, float *grads_out, uint64_t capacity,
                    uint64_t *n_unique_dev, void *stream) {
    if (!g || !desc) return fail(EMB_ERR_INVALID, "emb_grad_sparse: context or descriptor is NULL");
    if (itype != EMB_IDX_U32 && itype != EMB_IDX_I64) return fail(EMB_ERR_INVALID, "emb_grad_sparse: bad index type");
    if (!n_unique_dev || (uintptr_t)n_unique_dev % 8) return fail(EMB_ERR_INVALID, "emb_grad_sparse: n_unique_dev is NULL or not 8-byte aligned");
    Planned p{};                                 // the plan: a chain of one, with the unique numbering switched on
    if (int rc = check_desc(g, *desc, itype, nullptr, "emb_grad_sparse", &p.t)) return rc;
    if (capacity < desc->n_indices)
        return fail(EMB_ERR_INVALID, "emb_grad_sparse: room for %llu rows, %llu indices may name as many", (unsigned long long)capacity,
                    (unsigned long long)desc->n_indices);
    if (desc->n_indices && (!rows_out || !grads_out || (uintptr_t)rows_out % 8 || (uintptr_t)grads_out % 4))
        return fail(EMB_ERR_INVALID, "emb_grad_sparse: rows_out or grads_out is NULL or not naturally aligned");
    p.lane = lane_group_path(*desc, p.t, RES_SPARSE, nullptr, grads_out);
    if (desc->n_indices)
        if (int rc = plan_chain(g, desc, &p, 0, 1)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(g->device);
    if (desc->n_indices == 0) {
        GRAD_HIP(hipMemsetAsync(n_unique_dev, 0, 8, s));
        return EMB_OK;
    }
    const SparseOut out{reinterpret_cast<long long *>(rows_out), grads_out, reinterpret_cast<unsigned long long *>(n_unique_dev)};
    return run_chain(g, desc, nullptr, &p, 0, itype == EMB_IDX_I64, StepSpec{}, out, s);
}

}  // extern "C"

namespace {

// Everything that can be refused about an emb_sr_spec; NULL text: it is fine.
const char *sr_fault(const emb_sr_spec *sr) {
    if (!sr) return "the stochastic-rounding spec is NULL";
    if (sr->reserved != 0) return "the stochastic-rounding spec's reserved field must be 0";
    if ((uintptr_t)sr->step_dev % 8) return "step_dev is not 8-byte aligned";
    return nullptr;
}

int opt_call(emb_grad *g, const emb_grad_desc *descs, float *const *states, uint32_t n_descs, emb_index_type itype, const emb_opt_spec *opt,
             void *stream, bool multi, const emb_sr_spec *sr = nullptr) {
    const char *who = sr ? "emb_grad_step_sr" : multi ? "emb_grad_step_multi" : "emb_grad_step";
    if (!opt) return fail(EMB_ERR_INVALID, "%s: the optimizer spec is NULL", who);
    if (opt->kind != EMB_OPT_ADAGRAD && opt->kind != EMB_OPT_ROWWISE_ADAGRAD) return fail(EMB_ERR_INVALID, "%s: unknown optimizer kind %u", who, opt->kind);
    if (opt->reserved != 0) return fail(EMB_ERR_INVALID, "%s: the spec's reserved field must be 0, got %u", who, opt->reserved);
    if (!(opt->eps >= 0.f)) return fail(EMB_ERR_INVALID, "%s: eps must not be negative or NaN, got %g", who, (double)opt->eps);
    StepSpec st{opt->kind == EMB_OPT_ROWWISE_ADAGRAD ? RES_ROWWISE : RES_ADAGRAD, opt->lr, opt->eps};
    st.sr = sr;
    return step_call(g, descs, states, n_descs, itype, st, "an Adagrad", who, multi, stream);
}

}  // namespace

extern "C" {

int emb_grad_sgd(emb_grad *g, const emb_grad_desc *descs, uint32_t n_descs, emb_index_type itype, float lr, void *stream) {
    return step_call(g, descs, nullptr, n_descs, itype, StepSpec{RES_SGD, lr, 0.f}, "an SGD", "emb_grad_sgd", false, stream);
}

int emb_grad_sgd_multi(emb_grad *g, const emb_grad_desc *descs, uint32_t n_descs, emb_index_type itype, float lr, void *stream) {
    return step_call(g, descs, nullptr, n_descs, itype, StepSpec{RES_SGD, lr, 0.f}, "an SGD", "emb_grad_sgd_multi", true, stream);
}

uint64_t emb_opt_state_floats(uint32_t kind, uint64_t nr_rows, uint32_t dim) {
    if (kind == EMB_OPT_ADAGRAD) return nr_rows * dim;
    if (kind == EMB_OPT_ROWWISE_ADAGRAD) return nr_rows;
    return 0;
}

int emb_grad_step(emb_grad *g, const emb_grad_desc *descs, float *const *states, uint32_t n_descs, emb_index_type itype, const emb_opt_spec *opt,
                  void *stream) {
    return opt_call(g, descs, states, n_descs, itype, opt, stream, false);
}

int emb_grad_step_multi(emb_grad *g, const emb_grad_desc *descs, float *const *states, uint32_t n_descs, emb_index_type itype,
                        const emb_opt_spec *opt, void *stream) {
    return opt_call(g, descs, states, n_descs, itype, opt, stream, true);
}

int emb_grad_sgd_sr(emb_grad *g, const emb_grad_desc *descs, uint32_t n_descs, emb_index_type itype, float lr, const emb_sr_spec *sr, void *stream) {
    if (const char *fault = sr_fault(sr)) return fail(EMB_ERR_INVALID, "emb_grad_sgd_sr: %s", fault);
    StepSpec st{RES_SGD, lr, 0.f};
    st.sr = sr;
    return step_call(g, descs, nullptr, n_descs, itype, st, "an SGD", "emb_grad_sgd_sr", false, stream);
}

int emb_grad_step_sr(emb_grad *g, const emb_grad_desc *descs, float *const *states, uint32_t n_descs, emb_index_type itype, const emb_opt_spec *opt,
                     const emb_sr_spec *sr, void *stream) {
    if (const char *fault = sr_fault(sr)) return fail(EMB_ERR_INVALID, "emb_grad_step_sr: %s", fault);
    return opt_call(g, descs, states, n_descs, itype, opt, stream, false, sr);
}

int emb_grad_weights(emb_grad *g, const emb_grad_desc *descs, float *const *dw_out, uint32_t n_descs, emb_index_type itype, void *stream) {
    const char *who = "emb_grad_weights";
    if (!descs || !dw_out) return fail(EMB_ERR_INVALID, "%s: descs or dw_out is NULL", who);
    if (itype != EMB_IDX_U32 && itype != EMB_IDX_I64) return fail(EMB_ERR_INVALID, "%s: bad index type", who);
    if (!g) return fail(EMB_ERR_INVALID, "%s: context is NULL", who);
    std::vector<TableShape> shapes(n_descs);
    for (uint32_t k = 0; k < n_descs; k++) {     // the plan: every descriptor checked before anything is enqueued
        const emb_grad_desc &d = descs[k];
        TableShape &t = shapes[k];
        if (int rc = check_desc(g, d, itype, nullptr, who, &t)) return rc;
        if (d.pool.mode != EMB_POOL_SUM)
            return fail(EMB_ERR_UNSUPPORTED, "%s: per_sample_weights go with EMB_POOL_SUM only, table %u pools by mode %u", who, d.table_id, d.pool.mode);
        if (t.dtype != kF32 && t.dtype != kF16 && t.dtype != kBF16)
            return fail(EMB_ERR_UNSUPPORTED, "%s: table %u is fp8 or MXFP4: this call decodes fp32, fp16 and bf16 rows only", who, d.table_id);
        if (d.n_indices && (!dw_out[k] || (uintptr_t)dw_out[k] % 4))
            return fail(EMB_ERR_INVALID, "%s: the output of table %u is NULL or not 4-byte aligned", who, d.table_id);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(g->device);
    for (uint32_t k = 0; k < n_descs; k++) {     // the enqueue: one launch per non-empty descriptor
        const emb_grad_desc &d = descs[k];
        const TableShape &t = shapes[k];
        if (d.n_indices == 0) continue;
        const PoolArgs pa = pool_args(d);
        PswArgs a{};
        a.ids = d.indices, a.offsets = d.offsets, a.fixed_pooling = d.fixed_pooling;
        a.grad = d.grad, a.ld = d.grad_ld;
        a.table = t.rows, a.stride = t.stride, a.dtype = t.dtype;
        a.dw = dw_out[k], a.bad = &g->counters[0];
        a.pad_on = pa.pad_on, a.pad_idx = pa.pad_idx;
        a.n = (uint32_t)d.n_indices, a.n_bags = (uint32_t)d.n_bags, a.nr_rows = (uint32_t)t.nr_rows, a.dim = t.dim;
        const bool idx64 = itype == EMB_IDX_I64;
        if (lane_group_path(d, t, RES_SGD, nullptr, nullptr)) {
            const LaneGeom l = lane_geom(t.dim, a.n_bags ? a.n_bags : 1u);      // a group per bag (n_bags <= 2^31 - 1, 64 lanes: below 2^29 workgroups)
            if (idx64) grad_psw_group<true><<<dim3(l.blocks), dim3(kBlock), 0, s>>>(a, l.lanes, l.lanes_log2, l.chunks);
            else grad_psw_group<false><<<dim3(l.blocks), dim3(kBlock), 0, s>>>(a, l.lanes, l.lanes_log2, l.chunks);
        } else {
            const uint32_t lanes = dot_lanes(t.dim);
            uint32_t lanes_log2 = 0;
            while ((1u << lanes_log2) < lanes) lanes_log2++;
            const uint32_t blocks = (uint32_t)(((uint64_t)a.n * lanes + kBlock - 1) / kBlock);      // a group per position (n <= 2^30: below 2^28)
            if (idx64) grad_psw_elem<true><<<dim3(blocks), dim3(kBlock), 0, s>>>(a, lanes, lanes_log2);
            else grad_psw_elem<false><<<dim3(blocks), dim3(kBlock), 0, s>>>(a, lanes, lanes_log2);
        }
        GRAD_HIP(hipGetLastError());
    }
    return EMB_OK;
}

int emb_grad_master_step(emb_grad *g, const emb_grad_desc *descs, float *const *masters, float *const *states, uint32_t n_descs, emb_index_type itype,
                         const emb_master_spec *spec, void *stream) {
    const char *who = "emb_grad_master_step";
    if (!spec) return fail(EMB_ERR_INVALID, "%s: the master spec is NULL", who);
    if (spec->kind != EMB_MASTER_SGD && spec->kind != EMB_MASTER_ADAGRAD && spec->kind != EMB_MASTER_ROWWISE_ADAGRAD)
        return fail(EMB_ERR_INVALID, "%s: unknown master step kind %u", who, spec->kind);
    if (spec->reserved != 0) return fail(EMB_ERR_INVALID, "%s: the spec's reserved field must be 0, got %u", who, spec->reserved);
    if (!(spec->eps >= 0.f)) return fail(EMB_ERR_INVALID, "%s: eps must not be negative or NaN, got %g", who, (double)spec->eps);
    if (!g) return fail(EMB_ERR_INVALID, "%s: context is NULL", who);
    const bool sgd = spec->kind == EMB_MASTER_SGD;
    if (n_descs && (!descs || !masters || (!sgd && !states))) return fail(EMB_ERR_INVALID, "%s: descs, masters or states is NULL", who);
    if (itype != EMB_IDX_U32 && itype != EMB_IDX_I64) return fail(EMB_ERR_INVALID, "%s: bad index type", who);
    StepSpec st{sgd ? RES_SGD : spec->kind == EMB_MASTER_ADAGRAD ? RES_ADAGRAD : RES_ROWWISE, spec->lr, sgd ? 0.f : spec->eps};
    st.masters = masters;
    std::vector<Planned> plan(n_descs);
    if (int rc = plan_master(g, descs, masters, states, n_descs, itype, st, who, plan.data())) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DeviceGuard guard(g->device);
    for (uint32_t k = 0; k < n_descs; k++)
        if (plan[k].k)
            if (int rc = run_chain(g, descs, states, plan.data(), k, itype == EMB_IDX_I64, st, SparseOut{}, s)) return rc;
    return EMB_OK;
}

int emb_grad_master_report(emb_grad *g, uint64_t *n_unencodable) {
    if (!g) return fail(EMB_ERR_INVALID, "emb_grad_master_report: context is NULL");
    DeviceGuard guard(g->device);
    unsigned long long n = 0;
    GRAD_HIP(hipDeviceSynchronize());
    GRAD_HIP(hipMemcpy(&n, &g->counters[1], 8, hipMemcpyDeviceToHost));
    GRAD_HIP(hipMemset(&g->counters[1], 0, 8));
    if (n_unencodable) *n_unencodable = n;
    return EMB_OK;
}

int emb_grad_report(emb_grad *g, uint64_t *n_bad) {
    if (!g) return fail(EMB_ERR_INVALID, "emb_grad_report: context is NULL");
    DeviceGuard guard(g->device);
    unsigned long long bad = 0;
    GRAD_HIP(hipDeviceSynchronize());
    GRAD_HIP(hipMemcpy(&bad, &g->counters[0], 8, hipMemcpyDeviceToHost));
    GRAD_HIP(hipMemset(&g->counters[0], 0, 8));
    if (n_bad) *n_bad = bad;
    return EMB_OK;
}

}  // extern "C"

#else
}  // namespace
#endif  // !PIMEMB_GRAD_KERNEL_UNIT
