// pimemb_bag_kernels.h -- device code of the hot path (gfx950 / MI355X, CDNA4), as templates so the
// library (pimemb_kernels.hip) and the tuning tool (tools/tune_bag_kernels.hip) compile the very
// same source with different compile-time knobs.
//
// Replaces the UPMEM DPU program upmem/src/dpu/emb_dpu_lookup.c:36-138 (one DPU per (table,
// column), 14 tasklets striding over bags, one 8-byte MRAM read per (index, column)) and the host
// post-process upmem/include/emb_host.h:186-222 with ONE fused launch over all tables:
//
//   out[t][b][:] = sum_{p = off_t[b]}^{end-1} W_t[idx_t[p]][:]      end = off_t[b+1] | n_idx_t
//
// Mapping to the machine (bandwidth/latency-bound indexing; no MFMA -- there is no contraction):
//   * rows stay row-major [nr_rows][dim] in HBM; a row is read as 16-byte pieces, one per lane,
//     so the LPR = row_bytes/16 lanes of a "lane group" fetch a whole row with one coalesced
//     16-byte-per-lane load -- flat_load_dwordx4 in the shipped code object (PIMEMB_GLOBAL_AS 0, below) --
//     (64 B for dim 16 fp32, 512 B for dim 128 fp32);
//   * a 64-lane wavefront owns 64 consecutive bags per step ("wave batch"): lane l first loads the
//     bounds of bag l (two coalesced 256-B loads instead of 64/LPR scattered ones), then the
//     wavefront walks the batch in LPR rounds of 64/LPR bags, lane groups picking their bag's
//     bounds / index out of the owning lane with a wavefront shuffle (ds_bpermute);
//   * one-hot batches (every bag <= 1 index: the Criteo-Kaggle shape) take a fast path that
//     issues all rounds' row gathers before the first store, so a lane keeps up to 8 independent
//     16-byte gathers in flight; longer bags keep kUnroll gathers in flight inside the bag;
//   * every output element is accumulated by ONE lane in index order starting from +0, the order
//     of a sequential CPU EmbeddingBag: fp32 results are bit-identical to the oracle for any
//     pooling factor (no cross-lane reduction tree whose rounding would differ);
//   * the fixed-point mode keeps the reference arithmetic: int32 wrap-around accumulate
//     (emb_dpu_lookup.c:114) and out = (float)acc / 1e9 through double (emb_host.h:210).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "pimemb.h"

namespace pimemb {

// The 32 bytes behind the fixed fields of a DevDesc mean what the launch needs them to mean; each launch kind reads ONE of
// these views.
struct RangedView {         // ranged launch (bag_sum_wavebatch_kernel<..., RANGED>; launch_bag_sum(..., ranged))
    uint64_t row_lo;        // first row of the range this descriptor serves | kRangeOpenEnd
    uint32_t *served;       // counter in HBM the launch adds the number of bags it served to, or nullptr
};
struct PoolView {           // pooled launch (bag_pool_*: pool_args)
    const float *weights;   // per-sample weights, or nullptr
    uint64_t padding_row;   // padding row id, ~0: none
    uint64_t op;            // pooling op (kPoolOp*) | kPoolMean
};

// One table's share of a fused launch as the kernel sees it (HBM-resident array, 128 B each: a
// workgroup fetches its descriptor with scalar loads).
struct alignas(64) DevDesc {
    const void *weights;    // row-major [nr_rows][dim] of the table dtype
    const void *indices;    // IdxT[n_idx]
    const void *offsets;    // IdxT[n_bags] bag starts, or nullptr when fixed_pooling > 0
    float *out;             // float[n_bags][dim]
    uint64_t n_idx;
    uint64_t n_bags;
    uint64_t nr_rows;       // row ids are clamped to nr_rows-1 (kClamp); also read by the validation kernel
    uint32_t fixed_pooling; // L > 0: offsets[b] = b*L (load_generator.c:88)
    uint32_t n_tiles;       // ceil(n_bags / bags_per_tile) for this launch geometry
    // hot rows of this table (bag_sum_hot_kernel only; n_hot == 0 switches the LDS path off)
    const void *hot_rows;     // compact copy [n_hot][dim] of the hot rows, staged into LDS
    const uint64_t *hot_hash; // open-addressing table: entry = (slot << 32) | row id, empty = ~0
    uint32_t n_hot;
    uint32_t hot_log2;        // log2 of the hash table size
    union {                   // (words first: `DevDesc d{}` zeroes all of it)
        uint64_t words[4];    // raw: a plain launch leaves them zero; the plan signature and the tuners' own kernels read them
        RangedView ranged;
        PoolView pool;
    };
};
// words[3], which neither view reaches: the row stride of a STRIDED descriptor's output, in floats (emb_lookup_strided; read by
// the bag_strided_* twins only).  Zero in every other launch -- dense, ranged, hot-row, queue flush: `DevDesc d{}`.
constexpr int kOutStrideWord = 3;
static_assert(sizeof(DevDesc) == 128, "DevDesc is two 64-byte lines");
static_assert(offsetof(DevDesc, words) == 88 && offsetof(DevDesc, ranged.row_lo) == 88 && offsetof(DevDesc, ranged.served) == 96 &&
              offsetof(DevDesc, pool.weights) == 88 && offsetof(DevDesc, pool.padding_row) == 96 && offsetof(DevDesc, pool.op) == 104 &&
              sizeof(RangedView) <= 8 * kOutStrideWord && sizeof(PoolView) <= 8 * kOutStrideWord &&
              offsetof(DevDesc, words) + 8 * kOutStrideWord == 112,
              "the views overlay words[0..2], the strided output's row stride is words[3] (byte 112): engine, kernels, tuners and "
              "the host-side stub agree on these offsets");

using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x8 = __attribute__((ext_vector_type(8))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

// The fp8 table dtypes as template arguments and case labels: pimemb.h spells EMB_F8_E4M3 / EMB_F8_E5M2 as casts to emb_dtype
// outside the enum's range, which C++ does not take as constant expressions -- the same values as plain ints.
constexpr int kF8E4M3 = 8, kF8E5M2 = 9;
template <int DT>
inline constexpr bool kIsF8 = DT == kF8E4M3 || DT == kF8E5M2;

// Bytes of one table element of dtype `dt` (a public emb_dtype value): THE place that knows it -- geometry_for, the engine's
// and the shard's byte counts and the any-dim kernels all ask here.
__host__ __device__ constexpr uint32_t elem_bytes(int dt) {
    return (dt == kF8E4M3 || dt == kF8E5M2) ? 1u : (dt == EMB_F16 || dt == EMB_BF16) ? 2u : 4u;
}

// MXFP4 tables (EMB_MXFP4, the same way an int).  A row is no run of like elements: chunks = dim / 32 16-byte pieces of 32
// E2M1 elements each, then one E8M0 scale byte per piece, padded to a 16-byte multiple (pimemb.h has the layout).
constexpr int kMXFP4 = 10;
using f32x32 = __attribute__((ext_vector_type(32))) float;
// Bytes from one row of a table to the next: THE place that knows it -- table sizes, a plan's algorithmic bytes and the MXFP4
// kernels ask here (elem_bytes cannot say it for MXFP4).
__host__ __device__ constexpr uint64_t row_stride_bytes(int dt, uint32_t dim) {
    return dt == kMXFP4 ? (uint64_t)EMB_MXFP4_ROW_STRIDE(dim) : (uint64_t)dim * elem_bytes(dt);
}

// Compile-time knobs of the bag kernels.
template <int BLOCK = 256, int UNROLL = 8, bool NT_STORE = false, bool NT_META = false,
          int ONEHOT_INFLIGHT = 8, int MIN_WAVES = 1, int BATCHES = 1, bool NT_ROW = false,
          bool SPECULATE = false, bool IDX_SHUFFLE = false, bool CLAMP = false>
struct BagCfg {
    static constexpr bool kClamp = CLAMP;         // clamp row ids to the table and bag ends to n_idx: malformed
                                                  // input gives garbage rows, never an out-of-bounds access
    static constexpr bool kIdxShuffle = IDX_SHUFFLE; // lane group loads a window of indices coalesced, broadcasts by shuffle
    static constexpr bool kSpeculate = SPECULATE; // prefetch indices[bag] before the bounds arrive
    static constexpr int kMinWaves = MIN_WAVES;   // __launch_bounds__ 2nd arg: waves per SIMD wanted
    static constexpr int kBatches = BATCHES;      // 64-bag batches a wavefront takes per step
    static constexpr bool kNtRow = NT_ROW;        // non-temporal row gathers
    static constexpr int kBlock = BLOCK;          // threads per workgroup (multiple of 64)
    static constexpr int kUnroll = UNROLL;        // row gathers in flight per lane inside a bag
    static constexpr bool kNtStore = NT_STORE;    // non-temporal pooled-row stores
    static constexpr bool kNtMeta = NT_META;      // non-temporal index / offset loads
    static constexpr int kOneHot = ONEHOT_INFLIGHT;  // rounds batched on the one-hot fast path
};

// ---- per-dtype accumulate / store -----------------------------------------------------------
template <int DT>
struct RowOps;

// Address space of row / index / pooled-row accesses.  Pointers that come out of a descriptor in memory are generic
// ("flat"), and the SHIPPED build keeps them so (PIMEMB_GLOBAL_AS 0): its row gathers are flat_load_dwordx4, its pooled-row
// stores flat_store_dwordx4 ... nt.  Every buffer this library touches is GPU-visible memory (HBM, or pinned host memory on
// the zero-copy host path), never LDS or scratch, so they COULD be accessed as GLOBAL (address space 1, -DPIMEMB_GLOBAL_AS=1):
// global_load / global_store skip the aperture check and count on vmcnt alone.  Measured A/B on MI355X: no difference on any
// shape (profiles/r02/tune_address_space_flat_vs_global.log), so the default stays the plain one.
#ifndef PIMEMB_GLOBAL_AS
#define PIMEMB_GLOBAL_AS 0
#endif
#if PIMEMB_GLOBAL_AS
#define PIMEMB_AS __attribute__((address_space(1)))
#else
#define PIMEMB_AS
#endif

template <bool NT>
__device__ __forceinline__ void store_f32x4(float *dst, f32x4 v) {
    typedef f32x4 PIMEMB_AS *ptr_t;
    if constexpr (NT)
        __builtin_nontemporal_store(v, (ptr_t)(reinterpret_cast<f32x4 *>(dst)));
    else
        *(ptr_t)(reinterpret_cast<f32x4 *>(dst)) = v;
}

template <>
struct RowOps<EMB_F32> {
    using Acc = f32x4;
    static constexpr uint32_t kFloatsPerLane = 4;
    static constexpr bool kGroupStore = false;
    static __device__ __forceinline__ Acc zero() { return Acc{0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ void add(Acc &a, u32x4 raw) { a += __builtin_bit_cast(f32x4, raw); }
    template <bool NT>
    static __device__ __forceinline__ void store(const Acc &a, float *dst) {
        store_f32x4<NT>(dst, a);
    }
};

template <>
struct RowOps<EMB_F16> {
    using Acc = f32x8;
    static constexpr uint32_t kFloatsPerLane = 8;
    // A lane holds 8 consecutive output floats (32 B): storing them as two 16-byte pieces per lane makes
    // every store instruction hit alternate 16-byte pieces (32-B lane stride), which non-temporal stores
    // cannot combine -- measured 3.5 TB/s on one-hot fp16 lookups against ~7 for fp32.  store_row()
    // therefore re-deals the pieces inside the lane group so that each instruction writes a contiguous run
    // (rows of >= 8 lanes; narrower rows use plain stores and leave the merging to the L2).
    static constexpr bool kGroupStore = true;
    static __device__ __forceinline__ Acc zero() { return Acc{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ void add(Acc &a, u32x4 raw) {
        a += __builtin_convertvector(__builtin_bit_cast(f16x8, raw), f32x8);
    }
    template <bool NT>
    static __device__ __forceinline__ void store(const Acc &a, float *dst) {
        store_f32x4<NT>(dst, f32x4{a[0], a[1], a[2], a[3]});
        store_f32x4<NT>(dst + 4, f32x4{a[4], a[5], a[6], a[7]});
    }
};

// bfloat16 rows: a bf16 is the upper half of an fp32, so widening is integer work on the raw dwords and exact for every bit
// pattern (denormals, NaN payloads).  Dword i of a piece holds elements 2i (low half: v_lshlrev_b32 16) and 2i + 1 (high half:
// v_and_b32 0xffff0000), and the accumulator takes them in row order (store_row relies on it).  Written as ONE vector conversion,
// which the backend lowers to exactly those shifts and masks: spelled out as shifts, masks and a re-ordering shuffle the machine
// work is the same, but it is five IR operations where the fp16 conversion is one, too many for the compiler to speculate, and
// the one-hot paths then keep a branch around every gathered row (+2..4 % per launch: profiles/bf16/README.md).
__device__ __forceinline__ f32x8 widen_bf16x8(u32x4 raw) {
    return __builtin_convertvector(__builtin_bit_cast(bf16x8, raw), f32x8);
}

template <>
struct RowOps<EMB_BF16> {
    using Acc = f32x8;
    static constexpr uint32_t kFloatsPerLane = 8;
    static constexpr bool kGroupStore = true;      // 32 B of output per lane, as fp16 rows: see RowOps<EMB_F16>
    static __device__ __forceinline__ Acc zero() { return Acc{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ void add(Acc &a, u32x4 raw) { a += widen_bf16x8(raw); }
    template <bool NT>
    static __device__ __forceinline__ void store(const Acc &a, float *dst) {
        store_f32x4<NT>(dst, f32x4{a[0], a[1], a[2], a[3]});
        store_f32x4<NT>(dst + 4, f32x4{a[4], a[5], a[6], a[7]});
    }
};

// FP8 rows (OCP e4m3fn / e5m2): a lane's 16-byte piece is 16 elements, widened by the packed hardware conversions
// v_cvt_pk_f32_fp8 / v_cvt_pk_f32_bf8 -- two elements per instruction, low and high word of each dword (SDWA word select), eight
// instructions per piece, exact for every non-NaN bit pattern (subnormals, signed zeros, e5m2 infinities).  e5m2 could also be
// widened as the upper byte of an fp16 (zero-extend, shift, v_cvt_f32_f16): four v_perm_b32 and sixteen conversions per piece
// against eight, so the hardware conversion it is.  The accumulator takes the elements in row order (store_row relies on it).
template <int DT> struct F8Widen;
template <> struct F8Widen<kF8E4M3> {
    static __device__ __forceinline__ f32x2 two(uint32_t w, bool hi) { return hi ? __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true) : __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false); }
    static __device__ __forceinline__ float one(uint8_t b) { return __builtin_amdgcn_cvt_f32_fp8((int)b, 0); }
};
template <> struct F8Widen<kF8E5M2> {
    static __device__ __forceinline__ f32x2 two(uint32_t w, bool hi) { return hi ? __builtin_amdgcn_cvt_pk_f32_bf8((int)w, true) : __builtin_amdgcn_cvt_pk_f32_bf8((int)w, false); }
    static __device__ __forceinline__ float one(uint8_t b) { return __builtin_amdgcn_cvt_f32_bf8((int)b, 0); }
};
template <int DT>
__device__ __forceinline__ f32x16 widen_f8x16(u32x4 raw) {
    using W = F8Widen<DT>;
    const f32x4 q0 = __builtin_shufflevector(W::two(raw[0], false), W::two(raw[0], true), 0, 1, 2, 3);
    const f32x4 q1 = __builtin_shufflevector(W::two(raw[1], false), W::two(raw[1], true), 0, 1, 2, 3);
    const f32x4 q2 = __builtin_shufflevector(W::two(raw[2], false), W::two(raw[2], true), 0, 1, 2, 3);
    const f32x4 q3 = __builtin_shufflevector(W::two(raw[3], false), W::two(raw[3], true), 0, 1, 2, 3);
    const f32x8 h0 = __builtin_shufflevector(q0, q1, 0, 1, 2, 3, 4, 5, 6, 7), h1 = __builtin_shufflevector(q2, q3, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
}

// Wide fp8 rows (>= 8 lanes): a lane owns 64 B of output, four 16-byte pieces at a 64-byte lane stride.  1: store_row re-deals
// the pieces inside the lane group (16 ds_bpermute per store instruction) so that every instruction writes a contiguous run,
// non-temporally, as for fp16 rows; 0: four plain stores per lane, merged by the L2.  Measured on MI355X (profiles/fp8/README.md),
// us per launch, plain -> re-dealt: one-hot dim 128 177.6 -> 108.5, dim 256 330.7 -> 213.2, pooled dim 128 14.6 -> 12.6.
#ifndef PIMEMB_F8_WIDE_REDEAL
#define PIMEMB_F8_WIDE_REDEAL 1
#endif
// Narrow fp8 rows (<= 4 lanes) store plainly, four 16-byte pieces per lane.  1: those stores are non-temporal (an A/B of the
// one-hot launches' store pattern, profiles/fp8/README.md); 0, the default: ordinary stores that the L2 merges, as fp16's narrow rows.
#ifndef PIMEMB_F8_NARROW_NT
#define PIMEMB_F8_NARROW_NT 0
#endif

template <int DT>
struct F8RowOps {
    using Acc = f32x16;
    static constexpr uint32_t kFloatsPerLane = 16;
    static constexpr bool kGroupStore = true;       // 64 B of output per lane: store_row decides how they leave
    static constexpr bool kGroupRedeal = PIMEMB_F8_WIDE_REDEAL != 0;
    static constexpr bool kNarrowNt = PIMEMB_F8_NARROW_NT != 0;
    static __device__ __forceinline__ Acc zero() { return Acc{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ void add(Acc &a, u32x4 raw) { a += widen_f8x16<DT>(raw); }
    template <bool NT>
    static __device__ __forceinline__ void store(const Acc &a, float *dst) {
#pragma unroll
        for (int c = 0; c < 16; c += 4) store_f32x4<NT>(dst + c, f32x4{a[c], a[c + 1], a[c + 2], a[c + 3]});
    }
};
template <> struct RowOps<kF8E4M3> : F8RowOps<kF8E4M3> {};
template <> struct RowOps<kF8E5M2> : F8RowOps<kF8E5M2> {};

// MXFP4 rows: a lane's 16-byte piece is exactly one MX block -- 32 E2M1 elements -- and comes with the block's E8M0 scale byte
// from the row's tail.  Widened by v_cvt_scalef32_pk_f32_fp4: two elements (one byte) per instruction, the byte picked by op_sel,
// sixteen instructions per piece.
// PIMEMB_MX4_HW_SCALE 1: the scale travels as the instruction's scale operand, s << 23 (the fp32 whose exponent field is s).
// 0: the instruction widens with scale 1.0 and the element is multiplied by 2^(s - 127) in fp32 (exact: an E2M1 value has two
// significant bits; 2^-127 is the fp32 denormal 0x00400000, s = 0xFF a NaN) -- for hardware whose scale operand departs from
// the contract somewhere.  MI355X does not: over all 16 nibbles x 256 scale bytes (tests/test_gpu_mxfp4.py) the instruction takes
// the exponent field alone (s = 0 is 2^-127), keeps results that are fp32 denormals, reads the low nibble first and gives NaN
// for s = 0xFF, so 1 ships.
#ifndef PIMEMB_MX4_HW_SCALE
#define PIMEMB_MX4_HW_SCALE 1
#endif
// 1: the pooled row leaves by non-temporal stores; 0, the default: ordinary stores.  A lane owns 128 contiguous bytes of output,
// a whole line.  Measured on MI355X (profiles/mxfp4/README.md), us per launch, ordinary -> non-temporal: pooled dim 128 16.7 -> 26.8,
// one-hot dim 32 48 -> 226, dim 128 182 -> 952.
#ifndef PIMEMB_MX4_NT_STORE
#define PIMEMB_MX4_NT_STORE 0
#endif
struct Mx4Piece {
    u32x4 raw;      // 32 elements, element 2j in the low nibble of byte j
    uint32_t s;     // the block's E8M0 scale byte
};
__device__ __forceinline__ uint32_t load_mx4_scale(const char *p) {
    typedef const uint8_t PIMEMB_AS *ptr_t;
    return (uint32_t)*(ptr_t)(reinterpret_cast<const uint8_t *>(p));
}
__device__ __forceinline__ f32x32 widen_mx4x32(const Mx4Piece &pc) {
#if PIMEMB_MX4_HW_SCALE
    const float scale = __builtin_bit_cast(float, pc.s << 23);
#else
    const float scale = 1.0f;
    const float mul = __builtin_bit_cast(float, pc.s == 0u ? 0x00400000u : pc.s == 0xffu ? 0x7fc00000u : pc.s << 23);
#endif
    f32x32 out;
#define PIMEMB_MX4_BYTE(d, b)                                                                              \
    {                                                                                                      \
        const f32x2 v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(pc.raw[d], scale, b);                     \
        out[8 * (d) + 2 * (b)] = v[0];                                                                     \
        out[8 * (d) + 2 * (b) + 1] = v[1];                                                                 \
    }
#define PIMEMB_MX4_DWORD(d) PIMEMB_MX4_BYTE(d, 0) PIMEMB_MX4_BYTE(d, 1) PIMEMB_MX4_BYTE(d, 2) PIMEMB_MX4_BYTE(d, 3)
    PIMEMB_MX4_DWORD(0) PIMEMB_MX4_DWORD(1) PIMEMB_MX4_DWORD(2) PIMEMB_MX4_DWORD(3)
#undef PIMEMB_MX4_DWORD
#undef PIMEMB_MX4_BYTE
#if !PIMEMB_MX4_HW_SCALE
    out *= mul;
#endif
    return out;
}
template <>
struct RowOps<kMXFP4> {
    using Acc = f32x32;
    static constexpr uint32_t kFloatsPerLane = 32;
    static constexpr bool kGroupStore = true;       // 128 B of output per lane ...
    static constexpr bool kGroupRedeal = false;     // ... a whole line of its own: eight plain 16-byte stores, no re-deal
    static constexpr bool kNarrowNt = PIMEMB_MX4_NT_STORE != 0;
    static __device__ __forceinline__ Acc zero() {
        Acc a;
#pragma unroll
        for (int c = 0; c < 32; c++) a[c] = 0.f;
        return a;
    }
    static __device__ __forceinline__ void add(Acc &a, const Mx4Piece &pc) { a += widen_mx4x32(pc); }
    template <bool NT>
    static __device__ __forceinline__ void store(const Acc &a, float *dst) {
#pragma unroll
        for (int c = 0; c < 32; c += 4) store_f32x4<NT>(dst + c, f32x4{a[c], a[c + 1], a[c + 2], a[c + 3]});
    }
};

template <>
struct RowOps<EMB_FIXED32> {
    using Acc = u32x4;  // unsigned add == int32 two's-complement wrap (emb_dpu_lookup.c:114)
    static constexpr uint32_t kFloatsPerLane = 4;
    static constexpr bool kGroupStore = false;
    static __device__ __forceinline__ Acc zero() { return Acc{0u, 0u, 0u, 0u}; }
    static __device__ __forceinline__ void add(Acc &a, u32x4 raw) { a += raw; }
    static __device__ __forceinline__ float conv(uint32_t acc) {
        // emb_host.h:210: (float)tmp / pow(10,9): int32 -> float, divide in double, round to float
        return (float)((double)(float)(int32_t)acc / 1.0e9);
    }
    template <bool NT>
    static __device__ __forceinline__ void store(const Acc &a, float *dst) {
        store_f32x4<NT>(dst, f32x4{conv(a[0]), conv(a[1]), conv(a[2]), conv(a[3])});
    }
};

// ---- half-width pooled output (EMB_POOL_OUT_TABLE_DTYPE): the pooled row leaves in the table's own 2-byte dtype ----------
// An INTERNAL dtype value, EMB_F16 / EMB_BF16 with the kHalfOutDT bit, names the half-output twin of a kernel: the sum kernels
// derive everything from RowOps<DT> / ElemOps<DT>, so `fp16, half out` instantiates them under a mangling of its own and the
// fp32-out instantiations keep their machine code.  The value never leaves the library (launch_bag_sum maps to it).
// The fp32 accumulator is rounded ONCE, to nearest even: v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32, one per two elements, which is
// what the vector conversion lowers to on gfx950.
constexpr int kHalfOutDT = 16;
template <int DT>
inline constexpr bool kIsHalfOut = (DT & kHalfOutDT) != 0;

template <int BASE> struct HalfRound;      // fp32 -> the 2-byte dtype BASE, as raw bits
template <> struct HalfRound<EMB_F16> {
    static __device__ __forceinline__ u32x4 pack(f32x8 a) { return __builtin_bit_cast(u32x4, __builtin_convertvector(a, f16x8)); }
    static __device__ __forceinline__ uint16_t one(float x) { return __builtin_bit_cast(uint16_t, (_Float16)x); }
};
template <> struct HalfRound<EMB_BF16> {
    static __device__ __forceinline__ u32x4 pack(f32x8 a) { return __builtin_bit_cast(u32x4, __builtin_convertvector(a, bf16x8)); }
    static __device__ __forceinline__ uint16_t one(float x) { return __builtin_bit_cast(uint16_t, (__bf16)x); }
};

// A lane's 8 consecutive elements are 16 B of output: one dwordx4 store per lane, already contiguous across the lane group,
// so no group store.  The kernels address the output as float *: kFloatsPerLane is therefore the lane's output in FLOATS'
// WORTH of bytes (4), which makes out_stride = chunks * 4 floats = dim * 2 bytes.
template <int BASE>
struct HalfOutRowOps : RowOps<BASE> {
    static constexpr uint32_t kFloatsPerLane = 4;
    static constexpr bool kGroupStore = false;
    template <bool NT>
    static __device__ __forceinline__ void store(const f32x8 &a, float *dst) {
        store_f32x4<NT>(dst, __builtin_bit_cast(f32x4, HalfRound<BASE>::pack(a)));
    }
};
template <> struct RowOps<EMB_F16 | kHalfOutDT> : HalfOutRowOps<EMB_F16> {};
template <> struct RowOps<EMB_BF16 | kHalfOutDT> : HalfOutRowOps<EMB_BF16> {};

template <bool NT, typename T>
__device__ __forceinline__ T load_meta(const T *p) {
    typedef const T PIMEMB_AS *ptr_t;
    if constexpr (NT)
        return __builtin_nontemporal_load((ptr_t)p);
    else
        return *(ptr_t)p;
}

// Row id -> row id inside the table.  A 64-bit row id that came from a uint32 index is clamped with
// one 32-bit min (the high half is known to be zero); int64 indices (negative = huge unsigned) take
// the 64-bit compare.
template <bool CLAMP, typename IdxT = int64_t>
__device__ __forceinline__ uint64_t clamp_row(uint64_t r, uint64_t last_row) {
    if constexpr (!CLAMP) {
        return r;
    } else if constexpr (sizeof(IdxT) == 4) {
        const uint32_t last32 = last_row > 0xffffffffull ? 0xffffffffu : (uint32_t)last_row;
        const uint32_t r32 = (uint32_t)r;
        return (uint64_t)(r32 < last32 ? r32 : last32);
    } else {
        return r < last_row ? r : last_row;
    }
}

template <bool NT>
__device__ __forceinline__ u32x4 load_row(const char *p) {
    typedef const u32x4 PIMEMB_AS *ptr_t;
    if constexpr (NT)
        return __builtin_nontemporal_load((ptr_t)(reinterpret_cast<const u32x4 *>(p)));
    else
        return *(ptr_t)(reinterpret_cast<const u32x4 *>(p));
}

__device__ __forceinline__ uint32_t shfl_u32(uint32_t v, uint32_t src) {
    return (uint32_t)__shfl((int)v, (int)src, 64);
}
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, uint32_t src) {
    uint32_t lo = shfl_u32((uint32_t)v, src), hi = shfl_u32((uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}
template <typename IdxT>
__device__ __forceinline__ uint64_t shfl_index(IdxT v, uint32_t src) {
    if constexpr (sizeof(IdxT) == 8)
        return shfl_u64((uint64_t)v, src);
    else
        return (uint64_t)shfl_u32((uint32_t)v, src);
}

__device__ __forceinline__ float shfl_f32(float v, uint32_t src) {
    return __builtin_bit_cast(float, shfl_u32(__builtin_bit_cast(uint32_t, v), src));
}

// Store one pooled row held by a lane group.  `row` = out + bag * out_stride (the row's first float);
// `valid`: this lane owns a piece of a real bag.  Ops without kGroupStore: every lane stores its own
// 16 bytes (already contiguous across the group).  kGroupStore (2-byte tables: 32 B of output per lane, PPL = 2 pieces;
// fp8 tables: 64 B, PPL = 4): the row is PPL*chunks 16-byte pieces, lane s holds pieces PPL*s .. PPL*s + PPL-1; instruction i
// lets lane j write piece i*LPR + j, fetched from the owning lane with ds_bpermute -- EVERY lane
// of the group must call this (the shuffles read the neighbours' registers).
template <class Ops, class = void>
struct GroupRedeal { static constexpr bool value = true; };      // (Ops that say nothing re-deal: the 2-byte tables)
template <class Ops>
struct GroupRedeal<Ops, std::void_t<decltype(Ops::kGroupRedeal)>> { static constexpr bool value = Ops::kGroupRedeal; };

template <class Ops, class = void>
struct NarrowNt { static constexpr bool value = false; };
template <class Ops>
struct NarrowNt<Ops, std::void_t<decltype(Ops::kNarrowNt)>> { static constexpr bool value = Ops::kNarrowNt; };

template <class Ops, class Cfg, int LPR>
__device__ __forceinline__ void store_row(const typename Ops::Acc &acc, float *__restrict__ row, uint32_t sub,
                                          uint32_t grp, uint32_t chunks, bool valid) {
    if constexpr (!Ops::kGroupStore) {
        if (valid) Ops::template store<Cfg::kNtStore>(acc, row + sub * Ops::kFloatsPerLane);
    } else if constexpr (LPR <= 4 || !GroupRedeal<Ops>::value) {
        // narrow rows: the shuffles cost more than they save (fp16 dim 16 one-hot: 42 us with them, 21 us
        // without); plain 16-byte stores per lane instead, which the L2 merges into full lines
        if (valid) Ops::template store<NarrowNt<Ops>::value && Cfg::kNtStore>(acc, row + sub * Ops::kFloatsPerLane);
    } else if constexpr (Ops::kFloatsPerLane == 8) {
        const uint32_t pieces = 2u * chunks;
#pragma unroll
        for (uint32_t inst = 0; inst < 2; inst++) {
            const uint32_t p = inst * LPR + sub;               // piece this lane writes
            const uint32_t src = grp * LPR + (p >> 1);         // lane that holds it
            const bool hi = (p & 1u) != 0u;
            f32x4 v;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const float lo_c = shfl_f32(acc[c], src), hi_c = shfl_f32(acc[4 + c], src);
                v[c] = hi ? hi_c : lo_c;
            }
            // (validity is uniform over a lane group except for lanes beyond `chunks`, whose own
            // `valid` is false but which still write pieces of the row when p < pieces)
            const bool bag_ok = __shfl((int)valid, (int)(grp * LPR), 64) != 0;
            if (bag_ok && p < pieces) store_f32x4<Cfg::kNtStore>(row + 4u * p, v);
        }
    } else {
        // any number of pieces per lane (a power of two; the 2-piece case above keeps its own text, and with it the machine code
        // of the fp16 / bf16 kernels): LPR is a multiple of PPL here, so a lane wants the SAME piece number p % PPL of its
        // source lane in every instruction
        constexpr uint32_t PPL = Ops::kFloatsPerLane / 4u;
        static_assert((PPL & (PPL - 1u)) == 0u && LPR % PPL == 0u, "pieces per lane: a power of two that divides the lane group");
        const uint32_t pieces = PPL * chunks;
#pragma unroll
        for (uint32_t inst = 0; inst < PPL; inst++) {
            const uint32_t p = inst * LPR + sub;               // piece this lane writes
            const uint32_t src = grp * LPR + p / PPL;          // lane that holds it
            const uint32_t which = p % PPL;
            f32x4 v;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                float x = shfl_f32(acc[c], src);
#pragma unroll
                for (uint32_t k = 1; k < PPL; k++) {
                    const float y = shfl_f32(acc[4 * k + c], src);
                    x = (which == k) ? y : x;
                }
                v[c] = x;
            }
            // (validity is uniform over a lane group except for lanes beyond `chunks`, whose own
            // `valid` is false but which still write pieces of the row when p < pieces)
            const bool bag_ok = __shfl((int)valid, (int)(grp * LPR), 64) != 0;
            if (bag_ok && p < pieces) store_f32x4<Cfg::kNtStore>(row + 4u * p, v);
        }
    }
}

// Workgroup -> (descriptor, tile).  xmap == nullptr: 2-D grid (x = tile, y = descriptor).
// Otherwise the 1-D XCD-aware map built by pimemb_xcd_map.h: residue class blockIdx.x % 8 owns a
// contiguous share of the (table, tile) list, so a table's rows stay in ONE XCD's L2.
struct XcdSegDev {
    uint32_t desc, tile0, slot_begin, slot_end;
};
constexpr uint32_t kXmapDirect = 0x80000000u;   // flag in the `chunks` kernel argument: xmap is a per-workgroup table
constexpr uint64_t kRangeOpenEnd = 1ull << 63;  // flag in RangedView::row_lo (EMB_RANGE_OPEN_END, pimemb.h)

__device__ __forceinline__ bool decode_block(const uint32_t *__restrict__ xmap, uint32_t direct,
                                             uint32_t *desc_i, uint32_t *tile) {
    if (xmap == nullptr) {
        *desc_i = blockIdx.y;
        *tile = blockIdx.x;
        return true;
    }
    if (direct) {   // one 8-byte scalar load: {descriptor, tile} of this workgroup (0xffffffff = idle slot)
        const uint2 ent = reinterpret_cast<const uint2 *>(xmap)[blockIdx.x];
        *desc_i = ent.x;
        *tile = ent.y;
        return ent.x != 0xffffffffu;
    }
    const uint32_t cls = blockIdx.x & 7u, slot = blockIdx.x >> 3;
    const uint32_t ns = xmap[cls];
    const XcdSegDev *segs = reinterpret_cast<const XcdSegDev *>(xmap + 16) + xmap[8 + cls];
    // first segment whose slot_end exceeds `slot` (segments are sorted by slot): binary search, so a
    // launch over hundreds of tables costs ~log2 scalar loads per workgroup, not a linear walk
    uint32_t lo = 0, hi = ns;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (slot < segs[mid].slot_end)
            hi = mid;
        else
            lo = mid + 1;
    }
    if (lo >= ns) return false;
    const XcdSegDev sg = segs[lo];
    *desc_i = sg.desc;
    *tile = sg.tile0 + (slot - sg.slot_begin);
    return true;
}

// Walk one bag [p, e) in index order, adding the rows `fetch(row)` returns.  Two ways to get at the
// indices: (a) every lane of the group loads indices[p+k] itself (same address in all LPR lanes),
// kUnroll at a time; (b) kIdxShuffle: the group loads a WINDOW of indices coalesced -- lane `sub`
// holds indices[p + sub + i*LPR] -- and broadcasts them with ds_bpermute, one vector-memory
// instruction per LPR*IPL indices instead of one per index.  Every lane of the wavefront must call
// this (the shuffles need the whole lane group active); `live` lanes own a 16-byte piece of the row.
template <typename IdxT, int LPR, class Cfg, class Ops, class Probe, class Fetch>
__device__ __forceinline__ void walk_bag(const IdxT *__restrict__ indices, uint64_t p, uint64_t e, uint32_t sub,
                                         uint32_t grp, bool live, typename Ops::Acc &acc, Probe &&probe,
                                         Fetch &&fetch) {
    // probe(row) -> 32-bit token computed ONCE per index (e.g. the LDS slot of a hot row);
    // fetch(row, token) -> the lane's 16-byte piece of that row (whatever Ops::add takes).
    constexpr int U = Cfg::kUnroll;
    using Piece = decltype(fetch(uint64_t{}, uint32_t{}));   // u32x4: 16 bytes of a row; MXFP4: with the block's scale (Mx4Piece)
    constexpr bool kProbe = std::remove_reference_t<Probe>::kUsed;
    if constexpr (!Cfg::kIdxShuffle) {
        if (!live) return;
        for (; p + U <= e; p += U) {
            uint64_t r[U];
#pragma unroll
            for (int k = 0; k < U; k++) r[k] = (uint64_t)load_meta<Cfg::kNtMeta>(indices + p + k);
            Piece v[U];
#pragma unroll
            for (int k = 0; k < U; k++) v[k] = fetch(r[k], probe(r[k]));
#pragma unroll
            for (int k = 0; k < U; k++) Ops::add(acc, v[k]);
        }
        for (; p < e; p++) {
            const uint64_t r = (uint64_t)load_meta<Cfg::kNtMeta>(indices + p);
            Ops::add(acc, fetch(r, probe(r)));
        }
    } else {
        constexpr uint32_t IPL = (U + LPR - 1) / LPR;      // indices held per lane
        constexpr uint32_t W = IPL * LPR;                  // window
        while (p < e) {
            const uint32_t cnt = (e - p < W) ? (uint32_t)(e - p) : W;
            IdxT mine[IPL];
            uint32_t tok[IPL];
#pragma unroll
            for (uint32_t i = 0; i < IPL; i++) {
                mine[i] = 0;
                if (sub + i * LPR < cnt) mine[i] = load_meta<Cfg::kNtMeta>(indices + p + sub + i * LPR);
                tok[i] = probe((uint64_t)mine[i]);         // LPR different probes per instruction
            }
            uint32_t k = 0;
            for (; k + U <= cnt; k += U) {
                uint64_t r[U];
                uint32_t t[U];
#pragma unroll
                for (int j = 0; j < U; j++) {
                    const uint32_t q = k + j, src = grp * LPR + q % LPR;   // position in the window
                    r[j] = shfl_index<IdxT>(mine[(IPL == 1) ? 0 : q / LPR], src);
                    t[j] = kProbe ? shfl_u32(tok[(IPL == 1) ? 0 : q / LPR], src) : 0u;
                }
                if (live) {
                    Piece v[U];
#pragma unroll
                    for (int j = 0; j < U; j++) v[j] = fetch(r[j], t[j]);
#pragma unroll
                    for (int j = 0; j < U; j++) Ops::add(acc, v[j]);
                }
            }
            for (; k < cnt; k++) {
                const uint32_t src = grp * LPR + k % LPR;
                const uint64_t r = shfl_index<IdxT>(mine[(IPL == 1) ? 0 : k / LPR], src);
                const uint32_t t = kProbe ? shfl_u32(tok[(IPL == 1) ? 0 : k / LPR], src) : 0u;
                if (live) Ops::add(acc, fetch(r, t));
            }
            p += cnt;
        }
    }
}

struct NoProbe {
    static constexpr bool kUsed = false;
    __device__ __forceinline__ uint32_t operator()(uint64_t) const { return 0u; }
};

// ---- what the bag kernels share below their entry points -------------------------------------------------------------------
// Each piece is used where it leaves the kernel's machine code as it was (the counter profiles are tied to it, and the
// kernels are tuned to the register: DESIGN.md section 3.2b); a site that keeps its own text says so.

// One descriptor as a kernel's locals: typed pointers and the counts, fetched once per workgroup (scalar loads).
// (bag_pool_wavebatch_kernel and the three any-dim kernels spell these out: built from a DescView their code object changes.)
template <typename IdxT>
struct DescView {
    const char *__restrict__ weights;
    const IdxT *__restrict__ indices;
    const IdxT *__restrict__ offsets;
    float *__restrict__ out;
    uint64_t n_idx, n_bags, last_row;
    uint32_t fixed_pooling, n_tiles;
    __device__ __forceinline__ explicit DescView(const DevDesc *dp)
        : weights(static_cast<const char *>(dp->weights)), indices(static_cast<const IdxT *>(dp->indices)),
          offsets(static_cast<const IdxT *>(dp->offsets)), out(dp->out), n_idx(dp->n_idx), n_bags(dp->n_bags),
          last_row(dp->nr_rows - 1), fixed_pooling(dp->fixed_pooling), n_tiles(dp->n_tiles) {}
};

// Where a thread sits among the LPR-lane groups of its wavefront, and what a row of `chunks` 16-byte pieces means to it.
// (The two wave-batch kernels; the three lane-group kernels -- sum, hot, pooled -- spell it out: with a LaneGeom the code
// object of some of their instantiations changes.)
template <int LPR, class Ops>
struct LaneGeom {
    uint32_t lane, wave;             // lane of the wavefront, wavefront of the workgroup
    uint32_t sub, grp;               // piece of the row this lane owns, lane group of the wavefront
    uint32_t row_bytes, out_stride;  // bytes of a table row, floats of a pooled row
    const char *__restrict__ wsub;   // this lane's piece of row 0
    __device__ __forceinline__ LaneGeom(const char *weights, uint32_t chunks)
        : lane(threadIdx.x & 63u), wave(threadIdx.x >> 6), sub(lane & (LPR - 1)), grp(lane / LPR), row_bytes(chunks * 16u),
          out_stride(chunks * Ops::kFloatsPerLane), wsub(weights + sub * 16u) {}
};

// Bounds [p, e) of bag `bag` < n_bags: from the offsets array (the last bag ends at n_idx), else bag * fixed_pooling.
// (Plain arguments, not a DescView: the any-dim kernels have none.  bag_sum_group_kernel spells it out.)
template <bool NT, bool CLAMP, typename IdxT>
__device__ __forceinline__ void bag_range(const IdxT *__restrict__ offsets, uint64_t n_bags, uint64_t n_idx, uint32_t fixed_pooling,
                                          uint64_t bag, uint64_t &p, uint64_t &e) {
    if (offsets != nullptr) {
        p = (uint64_t)load_meta<NT>(offsets + bag);
        e = (bag + 1 < n_bags) ? (uint64_t)load_meta<NT>(offsets + bag + 1) : n_idx;
    } else {
        p = bag * fixed_pooling;
        e = p + fixed_pooling;
    }
    if (CLAMP && e > n_idx) e = n_idx;
}

// ---- any row width: one thread per output element --------------------------------------------
// Rows whose byte size is not a multiple of 16 (dim 2, 3, 10, 100 ... -- nn.EmbeddingBag takes any
// dim, dlrm_s_pytorch.py's default sparse feature size is 2) or exceeds 1 KiB cannot use the 16-byte
// lane pieces above.  `lanes` (power of two, <= 256) consecutive threads own one bag and stride over
// its columns; each output element is still summed by one thread in index order from +0, so results
// are bit-identical to the vector kernels and the oracle.  Generality path, not a tuned one.
template <int DT> struct ElemOps;
template <> struct ElemOps<EMB_F32> {
    using Elem = float; using Acc = float; using Out = float;
    static __device__ __forceinline__ void add(Acc &a, Elem v) { a = a + v; }
    static __device__ __forceinline__ float out(Acc a) { return a; }
};
template <> struct ElemOps<EMB_F16> {
    using Elem = _Float16; using Acc = float; using Out = float;
    static __device__ __forceinline__ void add(Acc &a, Elem v) { a = a + (float)v; }
    static __device__ __forceinline__ float out(Acc a) { return a; }
};
template <> struct ElemOps<EMB_BF16> {
    using Elem = uint16_t; using Acc = float; using Out = float;      // (Elem: the raw bits)
    static __device__ __forceinline__ float widen(Elem v) { return __builtin_bit_cast(float, (uint32_t)v << 16); }
    static __device__ __forceinline__ void add(Acc &a, Elem v) { a = a + widen(v); }
    static __device__ __forceinline__ float out(Acc a) { return a; }
};
template <int DT> struct F8ElemOps {
    using Elem = uint8_t; using Acc = float; using Out = float;       // (Elem: the raw byte)
    static __device__ __forceinline__ float widen(Elem v) { return F8Widen<DT>::one(v); }
    static __device__ __forceinline__ void add(Acc &a, Elem v) { a = a + widen(v); }
    static __device__ __forceinline__ float out(Acc a) { return a; }
};
template <> struct ElemOps<kF8E4M3> : F8ElemOps<kF8E4M3> {};
template <> struct ElemOps<kF8E5M2> : F8ElemOps<kF8E5M2> {};
template <> struct ElemOps<EMB_FIXED32> {
    using Elem = uint32_t; using Acc = uint32_t; using Out = float;
    static __device__ __forceinline__ void add(Acc &a, Elem v) { a += v; }
    static __device__ __forceinline__ float out(Acc a) { return RowOps<EMB_FIXED32>::conv(a); }
};

template <int BASE> struct HalfOutElemOps : ElemOps<BASE> {       // half-width output: Out is the raw bits of the table's dtype
    using Out = uint16_t;
    static __device__ __forceinline__ Out out(float a) { return HalfRound<BASE>::one(a); }
};
template <> struct ElemOps<EMB_F16 | kHalfOutDT> : HalfOutElemOps<EMB_F16> {};
template <> struct ElemOps<EMB_BF16 | kHalfOutDT> : HalfOutElemOps<EMB_BF16> {};

template <typename IdxT, int DT, bool CLAMP>
__global__ void __launch_bounds__(256)
bag_sum_anydim_kernel(const DevDesc *__restrict__ descs, uint32_t dim, uint32_t lanes) {
    using E = ElemOps<DT>;
    const DevDesc *dp = descs + blockIdx.y;
    const typename E::Elem *__restrict__ weights = static_cast<const typename E::Elem *>(dp->weights);
    const IdxT *__restrict__ indices = static_cast<const IdxT *>(dp->indices);
    const IdxT *__restrict__ offsets = static_cast<const IdxT *>(dp->offsets);
    typename E::Out *__restrict__ out = reinterpret_cast<typename E::Out *>(dp->out);     // (float, or the halves of a half-output twin)
    const uint64_t n_idx = dp->n_idx, n_bags = dp->n_bags, last_row = dp->nr_rows - 1;
    const uint64_t bag = (uint64_t)blockIdx.x * (256u / lanes) + threadIdx.x / lanes;
    if (blockIdx.x >= dp->n_tiles || bag >= n_bags) return;
    uint64_t p0, e;
    bag_range<false, CLAMP>(offsets, n_bags, n_idx, dp->fixed_pooling, bag, p0, e);
    for (uint32_t col = threadIdx.x & (lanes - 1); col < dim; col += lanes) {
        typename E::Acc acc = 0;
        for (uint64_t p = p0; p < e; p++) {
            const uint64_t r = clamp_row<CLAMP, IdxT>((uint64_t)indices[p], last_row);
            E::add(acc, weights[r * dim + col]);
        }
        out[bag * dim + col] = E::out(acc);
    }
}

// Rows whose byte size is a multiple of 4 (every fp32 / fixed-point dim, even fp16 dims) but not of 16:
// one thread per 16-byte PIECE instead of per element.  A piece of an unpadded row starts at a 4-byte
// aligned address, which global_load/store_dwordx4 accept on gfx950, so full pieces move as vectors and
// only the last, partial piece of a row goes element by element.  Same summation order, same bits.
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

template <typename IdxT, int DT, bool CLAMP>
__global__ void __launch_bounds__(256)
bag_sum_anydim_vec_kernel(const DevDesc *__restrict__ descs, uint32_t dim, uint32_t lanes) {
    using Ops = RowOps<DT>;
    constexpr uint32_t ESZ = elem_bytes(DT & ~kHalfOutDT);
    constexpr uint32_t EP = 16u / ESZ;                       // elements per 16-byte piece (4, 8 halves or 16 bytes)
    constexpr int U = 4;
    const DevDesc *dp = descs + blockIdx.y;
    const char *__restrict__ weights = static_cast<const char *>(dp->weights);
    const IdxT *__restrict__ indices = static_cast<const IdxT *>(dp->indices);
    const IdxT *__restrict__ offsets = static_cast<const IdxT *>(dp->offsets);
    float *__restrict__ out = dp->out;
    const uint64_t n_idx = dp->n_idx, n_bags = dp->n_bags, last_row = dp->nr_rows - 1;
    const uint64_t bag = (uint64_t)blockIdx.x * (256u / lanes) + threadIdx.x / lanes;
    if (blockIdx.x >= dp->n_tiles || bag >= n_bags) return;
    uint64_t p0, e;
    bag_range<false, CLAMP>(offsets, n_bags, n_idx, dp->fixed_pooling, bag, p0, e);
    const uint32_t row_bytes = dim * ESZ, pieces = (dim + EP - 1) / EP;
    for (uint32_t piece = threadIdx.x & (lanes - 1); piece < pieces; piece += lanes) {
        const uint32_t n_el = (dim - piece * EP < EP) ? dim - piece * EP : EP;
        const char *__restrict__ wp = weights + piece * 16u;
        auto fetch = [&](uint64_t r) -> u32x4 {
            const char *src = wp + clamp_row<CLAMP, IdxT>(r, last_row) * row_bytes;
            if (n_el == EP) return *reinterpret_cast<const u32x4_a4 *>(src);
            u32x4 v = {0u, 0u, 0u, 0u};                     // partial last piece: whole dwords only
            const uint32_t n_dw = n_el * ESZ / 4u;
            for (uint32_t d = 0; d < n_dw; d++) v[d] = reinterpret_cast<const uint32_t *>(src)[d];
            return v;
        };
        typename Ops::Acc acc = Ops::zero();
        uint64_t p = p0;      // (walk_bag's non-shuffle loop, spelled out: a call of walk_bag changes the code object of 2 of 6 instantiations)
        for (; p + U <= e; p += U) {
            uint64_t r[U];
#pragma unroll
            for (int k = 0; k < U; k++) r[k] = (uint64_t)indices[p + k];
            u32x4 v[U];
#pragma unroll
            for (int k = 0; k < U; k++) v[k] = fetch(r[k]);
#pragma unroll
            for (int k = 0; k < U; k++) Ops::add(acc, v[k]);
        }
        for (; p < e; p++) Ops::add(acc, fetch((uint64_t)indices[p]));
        if constexpr (kIsHalfOut<DT>) {
            // half-width output: the piece is 16 B of halves at a 4-byte aligned address (dim is even here)
            uint16_t *o = reinterpret_cast<uint16_t *>(out) + bag * dim + piece * EP;
            const u32x4 h = HalfRound<DT & ~kHalfOutDT>::pack(acc);
            if (n_el == EP) {
                *reinterpret_cast<u32x4_a4 *>(o) = h;
            } else {
#pragma unroll
                for (uint32_t c = 0; c < EP; c++)
                    if (c < n_el) o[c] = (uint16_t)(h[c / 2] >> (16u * (c & 1u)));
            }
        } else {
            float *o = out + bag * dim + piece * EP;
            float res[EP];
            if constexpr (DT == EMB_FIXED32) {
#pragma unroll
                for (uint32_t c = 0; c < EP; c++) res[c] = RowOps<EMB_FIXED32>::conv(acc[c]);
            } else {
#pragma unroll
                for (uint32_t c = 0; c < EP; c++) res[c] = acc[c];
            }
            if (n_el == EP) {
#pragma unroll
                for (uint32_t c = 0; c < EP; c += 4)
                    *reinterpret_cast<f32x4_a4 *>(o + c) = f32x4{res[c], res[c + 1], res[c + 2], res[c + 3]};
            } else {
                for (uint32_t c = 0; c < n_el; c++) o[c] = res[c];
            }
        }
    }
}

// Rounds of the one-hot fast path a wavefront keeps in flight for 1-KiB rows (LPR = 64: one bag per round).  Eight -- what every
// narrower row width uses -- needs two registers more than the 64-VGPR cap holds there (12 bytes of scratch per lane); four leaves one.
// 26 Kaggle-sized tables, dim 256 fp32, B = 39 292, us per launch (tools/wide_row_onehot_probe.py, profiles/r06/wide_rows_*.log):
// 8 in flight 270.4, 4 in flight 257.0-259.6 (-4 %), 2 in flight 267.4; dim 128 (LPR = 32, untouched) 122.6-125.2 in the same runs.
#ifndef PIMEMB_LPR64_ONEHOT_INFLIGHT
#define PIMEMB_LPR64_ONEHOT_INFLIGHT 4
#endif
// ... and for 512-byte rows (LPR = 32: dim 128 fp32, the Terabyte shape): tools/onehot_inflight_sweep.sh
#ifndef PIMEMB_LPR32_ONEHOT_INFLIGHT
#define PIMEMB_LPR32_ONEHOT_INFLIGHT 8
#endif

// (1-KiB rows, LPR = 64: eight rounds in flight = 8 KiB per wavefront and two registers more than the 64-VGPR cap of the
// fp32 configurations holds -- 12 bytes of scratch per lane; PIMEMB_LPR64_ONEHOT_INFLIGHT picks the depth for that row width)
template <int LPR, class Cfg>
constexpr uint32_t onehot_rounds_in_flight() {      // of the LPR rounds of a 64-bag wave batch (both wave-batch kernels)
    constexpr uint32_t depth = (LPR == 64) ? (uint32_t)PIMEMB_LPR64_ONEHOT_INFLIGHT : (LPR == 32) ? (uint32_t)PIMEMB_LPR32_ONEHOT_INFLIGHT : (uint32_t)Cfg::kOneHot;
    return ((uint32_t)LPR < depth) ? (uint32_t)LPR : depth;
}

// The lane-group kernel (v1) and the wave-batch kernel (v2) themselves: pimemb_sum_kernels.inc, compiled under two sets of
// names.  bag_sum_* here write dense pooled rows; the strided twins bag_strided_sum_* are at the end of this header.
// PIMEMB_OUT_STRIDE(dp, dense): floats from one bag's pooled row to the next -- `dense` for every kernel but the strided twins.
#define PIMEMB_OUT_STRIDE(dp, dense) (dense)
#define PIMEMB_SUM_KERNEL(path) bag_sum_##path##_kernel
#include "pimemb_sum_kernels.inc"
#undef PIMEMB_SUM_KERNEL

// ---- v3: lane-group kernel with the table's HOT ROWS staged in LDS -------------------------------
// For skewed (Zipf-like) pooled workloads.  The engine keeps, per table, a compact copy of up to a
// few hundred hot rows plus a small open-addressing hash (row id -> slot).  A persistent workgroup
// stages both into LDS once, then walks its share of the table's bags: every index is probed in the
// LDS hash (two ds_read_b64); a hit reads the row piece from LDS (ds_read_b128), a miss goes to
// L2/HBM as before.  The hot copy holds the same bits as the table, and the adds stay in index
// order, so results are bit-identical to the other kernels.
constexpr uint32_t kHotEmpty = 0xffffffffu;
constexpr uint32_t kHotProbes = 2;   // the host builder places a row within this many probes or drops it

__device__ __forceinline__ uint32_t hot_hash_pos(uint32_t key, uint32_t log2size) {
    return (key * 0x9E3779B1u) >> (32u - log2size);
}

struct HotProbe {
    static constexpr bool kUsed = true;
    const uint64_t *lhash;
    uint32_t n_hot, log2, mask;
    __device__ __forceinline__ uint32_t operator()(uint64_t r) const {
        if (n_hot == 0 || r >= 0xffffffffull) return 0u;
        const uint32_t key = (uint32_t)r, pos = hot_hash_pos(key, log2);
        const uint64_t e0 = lhash[pos], e1 = lhash[(pos + 1) & mask];
        if ((uint32_t)e0 == key) return 0x80000000u | (uint32_t)(e0 >> 32);
        if ((uint32_t)e1 == key) return 0x80000000u | (uint32_t)(e1 >> 32);
        return 0u;
    }
};

template <typename IdxT, int DT, int LPR, class Cfg>
__global__ void __launch_bounds__(Cfg::kBlock)
bag_sum_hot_kernel(const DevDesc *__restrict__ descs, uint32_t chunks) {
    using Ops = RowOps<DT>;
    constexpr uint32_t kWaves = Cfg::kBlock / 64;
    constexpr uint32_t BPW = 64 / LPR;
    constexpr uint32_t BAGS_PER_TILE = BPW * kWaves;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];

    const DevDesc *dp = descs + blockIdx.y;
    const DescView<IdxT> t(dp);
    const uint32_t n_hot = dp->n_hot, hot_log2 = dp->hot_log2;

    // (a LaneGeom here changes the code object of 8 of this kernel's 42 instantiations)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t sub = lane & (LPR - 1), grp = lane / LPR;
    const uint32_t row_bytes = chunks * 16u;
    const uint32_t out_stride = chunks * Ops::kFloatsPerLane;
    const char *__restrict__ wsub = t.weights + sub * 16u;

    // stage hot rows + hash into LDS (rows first: 16-byte aligned pieces)
    u32x4 *lrows = reinterpret_cast<u32x4 *>(lds_raw);
    uint64_t *lhash = reinterpret_cast<uint64_t *>(lds_raw + (size_t)n_hot * row_bytes);
    const uint32_t hash_mask = (1u << hot_log2) - 1u;
    if (n_hot) {
        const u32x4 *src = static_cast<const u32x4 *>(dp->hot_rows);
        for (uint32_t i = threadIdx.x; i < n_hot * chunks; i += Cfg::kBlock) lrows[i] = src[i];
        for (uint32_t i = threadIdx.x; i <= hash_mask; i += Cfg::kBlock) lhash[i] = dp->hot_hash[i];
    }
    __syncthreads();
    const u32x4 *lsub = lrows + sub;

    // probe: token = 0x80000000 | LDS slot if the row is hot, 0 otherwise (one probe per INDEX: with
    // kIdxShuffle each lane probes its own index of the window, 32 probes per instruction pair)
    HotProbe probe{lhash, n_hot, hot_log2, hash_mask};
    // one gathered row piece: LDS if the row is hot, L2/HBM otherwise
    auto fetch = [&](uint64_t r, uint32_t tok) -> u32x4 {
        if (tok & 0x80000000u) return lsub[(tok & 0x7fffffffu) * chunks];
        return load_row<Cfg::kNtRow>(wsub + clamp_row<Cfg::kClamp, IdxT>(r, t.last_row) * row_bytes);
    };

    const bool live = sub < chunks;
    for (uint32_t tile = blockIdx.x; tile < t.n_tiles; tile += gridDim.x) {
        const uint64_t bag = (uint64_t)tile * BAGS_PER_TILE + wave * BPW + grp;
        if (bag < t.n_bags) {                          // (no `continue`: lane groups stay whole for the shuffles)
            uint64_t p, e;
            bag_range<Cfg::kNtMeta, Cfg::kClamp>(t.offsets, t.n_bags, t.n_idx, t.fixed_pooling, bag, p, e);
            typename Ops::Acc acc = Ops::zero();
            walk_bag<IdxT, LPR, Cfg, Ops>(t.indices, p, e, sub, grp, live, acc, probe, fetch);
            store_row<Ops, Cfg, LPR>(acc, t.out + bag * out_stride, sub, grp, chunks, live);
        }
    }
}

// ---- pooled lookups: mean / max pooling, per-sample weights, padding_idx (emb_lookup_pooled) -------------------------
// A family of its own (bag_pool_*), so that every bag_sum_* kernel above keeps its machine code.  Each output element is
// still owned by ONE lane that takes the bag's entries in index order, and the arithmetic is spelled out so that the result
// equals torch's CPU EmbeddingBag bit for bit (fp16 and bf16 rows are widened to fp32 first):
//   sum              acc = +0; acc = acc + x
//   weighted sum     acc = fma(w, x, acc)                         (no padding_idx: torch's fused per-sample-weight kernel)
//   ... + padding    acc = acc + round(w * x)                     (padding_idx given: torch takes the unfused path)
//   mean             acc = sum as above; out = acc / count        (a true division; count = non-padding entries; 0 -> +0)
//   max              acc = first row; acc = (x > acc) ? x : acc  (strict compare: the first of equal values stays, +0 vs -0
//                                                                  included -- v_max_f32 would not keep it; empty -> +0)
// Padding entries are skipped before their row is gathered.  hipcc contracts a * b + c into an FMA by default, so the
// unfused rule lives under `fp contract(off)` and the fused one is an explicit fma.
// The pooling spec of a descriptor rides in DevDesc::pool (PoolView).
constexpr uint32_t kPoolOpAdd = 0, kPoolOpFma = 1, kPoolOpMulAdd = 2, kPoolOpMax = 3;
constexpr uint32_t kPoolMean = 0x100u;

struct PoolArgs {
    const float *psw;   // per-sample weights, or nullptr
    uint64_t pad;       // padding row id, ~0 for none
    uint32_t op;        // kPoolOp*: uniform over a descriptor, so every branch on it is a scalar one
    bool mean;
};

__device__ __forceinline__ PoolArgs pool_args(const DevDesc *dp) {
    PoolArgs a;
    a.psw = dp->pool.weights;
    a.pad = dp->pool.padding_row;
    a.op = (uint32_t)dp->pool.op & 0xffu;
    a.mean = (dp->pool.op & kPoolMean) != 0;
    return a;
}

// One entry into one accumulator element.  `first`: no entry of this bag was taken yet (max starts at the first row).
__device__ __forceinline__ float pool_op1(float acc, float x, float w, uint32_t op, bool first) {
#pragma clang fp contract(off)
    if (op == kPoolOpAdd) return acc + x;
    if (op == kPoolOpFma) return __builtin_fmaf(w, x, acc);
    if (op == kPoolOpMulAdd) return acc + w * x;          // the product rounded on its own (contract off)
    return (first || x > acc) ? x : acc;
}

// count taken entries -> the pooled value (sum / max: acc as it is; +0 for an empty bag, which acc still is)
__device__ __forceinline__ float pool_finish1(float acc, uint32_t cnt, bool mean) {
    return (mean && cnt > 1u) ? __fdiv_rn(acc, (float)cnt) : acc;    // (x / 1 == x: one-entry bags skip the division)
}

// A lane's 16-byte piece of a row as fp32 accumulator elements (RowOps<DT>::Acc: the layout store_row expects).
template <int DT> struct PoolRow;
template <> struct PoolRow<EMB_F32> {
    static constexpr int K = 4;
    static __device__ __forceinline__ f32x4 widen(u32x4 raw) { return __builtin_bit_cast(f32x4, raw); }
};
template <> struct PoolRow<EMB_F16> {
    static constexpr int K = 8;
    static __device__ __forceinline__ f32x8 widen(u32x4 raw) {
        return __builtin_convertvector(__builtin_bit_cast(f16x8, raw), f32x8);
    }
};
template <> struct PoolRow<EMB_BF16> {
    static constexpr int K = 8;
    static __device__ __forceinline__ f32x8 widen(u32x4 raw) { return widen_bf16x8(raw); }
};

template <int DT> struct F8PoolRow {
    static constexpr int K = 16;
    static __device__ __forceinline__ f32x16 widen(u32x4 raw) { return widen_f8x16<DT>(raw); }
};
template <> struct PoolRow<kF8E4M3> : F8PoolRow<kF8E4M3> {};
template <> struct PoolRow<kF8E5M2> : F8PoolRow<kF8E5M2> {};

template <int DT, class Acc>
__device__ __forceinline__ void pool_combine(Acc &acc, u32x4 raw, float w, uint32_t op, bool first) {
    const auto x = PoolRow<DT>::widen(raw);
#pragma unroll
    for (int c = 0; c < PoolRow<DT>::K; c++) acc[c] = pool_op1(acc[c], x[c], w, op, first);
}

template <int DT, class Acc>
__device__ __forceinline__ void pool_finish(Acc &acc, uint32_t cnt, bool mean) {
    if (!mean || cnt <= 1u) return;
#pragma unroll
    for (int c = 0; c < PoolRow<DT>::K; c++) acc[c] = pool_finish1(acc[c], cnt, mean);
}

// Walk one bag [p, e) in index order for a lane that owns a 16-byte piece of the row: kUnroll indices (and weights) are
// loaded, padding entries dropped, the remaining rows gathered together, then taken in order.
// (bag_pool_anydim_kernel has its own copy of the load / drop-padding step: as a function of U entries, or of one, shared by
// the two, it changes the code object of all 64 pooled kernels.)
template <typename IdxT, int DT, class Cfg>
__device__ __forceinline__ void pool_walk(const IdxT *__restrict__ indices, const PoolArgs &a, uint64_t p, uint64_t e,
                                          const char *__restrict__ wsub, uint32_t row_bytes, uint64_t last_row,
                                          typename RowOps<DT>::Acc &acc, uint32_t &cnt) {
    constexpr int U = Cfg::kUnroll;
    for (; p < e; p += U) {
        const uint64_t left = e - p;
        uint64_t r[U];
        float w[U];
        bool use[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            use[k] = (uint64_t)k < left;
            r[k] = 0;
            w[k] = 1.f;
            if (use[k]) {
                r[k] = (uint64_t)load_meta<Cfg::kNtMeta>(indices + p + k);
                if (a.psw != nullptr) w[k] = load_meta<Cfg::kNtMeta>(a.psw + p + k);
            }
            use[k] = use[k] && r[k] != a.pad;
        }
        u32x4 v[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            v[k] = u32x4{0u, 0u, 0u, 0u};
            if (use[k]) v[k] = load_row<Cfg::kNtRow>(wsub + clamp_row<Cfg::kClamp, IdxT>(r[k], last_row) * row_bytes);
        }
#pragma unroll
        for (int k = 0; k < U; k++)
            if (use[k]) {
                pool_combine<DT>(acc, v[k], w[k], a.op, cnt == 0u);
                cnt++;
            }
    }
}

// The kernels themselves: pimemb_pool_kernels.inc, compiled under two sets of names.  bag_pool_* are the fp32 and fp16
// instantiations.  bf16 tables enter through bag_bf16pool_*, the same text with the same template arguments:
// tests/test_pooling_abi.py pins the SET of bag_pool_* kernels in the code object (64: index width x fp32 / fp16 x row widths
// x paths, plus the any-dim ones) and is not a file that adding a dtype may edit, so that set stays what the test pins;
// launch_bag_pool (pimemb_kernels.hip) and codeobj.symbol_fragments know both names.  fp8 tables the same way: bag_f8pool_*.
// Half-width output (EMB_POOL_OUT_TABLE_DTYPE): a third set, bag_hpool_*, for fp16 and bf16 tables alike -- the same text with
// PIMEMB_POOL_HALF_OUT 1, which swaps in the half-output RowOps (one 16-byte store per lane) and the any-dim kernel's 2-byte
// store tail.  DT stays the table's public dtype there; the name tells the twins apart (and is not one the tests above pin).
#define PIMEMB_POOL_KERNEL(path) bag_pool_##path##_kernel
#define PIMEMB_POOL_HALF_OUT 0
#define PIMEMB_POOL_ROWOPS(DT) RowOps<DT>
#include "pimemb_pool_kernels.inc"
#undef PIMEMB_POOL_KERNEL
#define PIMEMB_POOL_KERNEL(path) bag_bf16pool_##path##_kernel
#include "pimemb_pool_kernels.inc"
#undef PIMEMB_POOL_KERNEL
#define PIMEMB_POOL_KERNEL(path) bag_f8pool_##path##_kernel       // fp8 tables (both encodings), fp32 out: as bag_bf16pool_*
#include "pimemb_pool_kernels.inc"
#undef PIMEMB_POOL_KERNEL
#undef PIMEMB_POOL_HALF_OUT
#undef PIMEMB_POOL_ROWOPS
#define PIMEMB_POOL_KERNEL(path) bag_hpool_##path##_kernel
#define PIMEMB_POOL_HALF_OUT 1
#define PIMEMB_POOL_ROWOPS(DT) RowOps<(DT) | kHalfOutDT>
#include "pimemb_pool_kernels.inc"
#undef PIMEMB_POOL_KERNEL
#undef PIMEMB_POOL_HALF_OUT
#undef PIMEMB_POOL_ROWOPS

// ---- MXFP4 tables: the lane-group kernels, sum and pooled ------------------------------------------------------------------
// Kernels of their own, not instantiations of the ones above: a row is `chunks` 16-byte pieces FOLLOWED by `chunks` scale bytes,
// so the row stride is not chunks * 16, a gather is a 16-byte load plus a byte load (lane `sub`: row + 16 * sub and
// row + 16 * chunks + sub -- for dims <= 224 inside the cache lines the pieces bring in anyway), and a lane accumulates 32 floats.
// Everything else is the lane-group kernels': one lane group per bag, indices loaded as a window and broadcast by shuffle, each
// output element summed by one lane in index order from +0.  The lanes of a group beyond `chunks` (dim 96: 3 of 4) gather nothing.
__host__ __device__ constexpr uint32_t mx4_row_stride(uint32_t chunks) { return (chunks * 17u + 15u) & ~15u; }
static_assert(mx4_row_stride(1) == EMB_MXFP4_ROW_STRIDE(32u) && mx4_row_stride(4) == EMB_MXFP4_ROW_STRIDE(128u) &&
              mx4_row_stride(64) == EMB_MXFP4_ROW_STRIDE(2048u), "the kernels' row stride is the header's");

// pool_walk for MXFP4 rows: kUnroll indices (and weights) loaded, padding entries dropped, the remaining blocks and scales
// gathered together, then taken in order.
template <typename IdxT, class Cfg>
__device__ __forceinline__ void mx4_pool_walk(const IdxT *__restrict__ indices, const PoolArgs &a, uint64_t p, uint64_t e,
                                              const char *__restrict__ wsub, const char *__restrict__ ssub, uint32_t row_stride,
                                              uint64_t last_row, f32x32 &acc, uint32_t &cnt) {
    constexpr int U = Cfg::kUnroll;
    for (; p < e; p += U) {
        const uint64_t left = e - p;
        uint64_t r[U];
        float w[U];
        bool use[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            use[k] = (uint64_t)k < left;
            r[k] = 0;
            w[k] = 1.f;
            if (use[k]) {
                r[k] = (uint64_t)load_meta<Cfg::kNtMeta>(indices + p + k);
                if (a.psw != nullptr) w[k] = load_meta<Cfg::kNtMeta>(a.psw + p + k);
            }
            use[k] = use[k] && r[k] != a.pad;
        }
        Mx4Piece v[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            v[k] = Mx4Piece{u32x4{0u, 0u, 0u, 0u}, 0u};
            if (use[k]) {
                const uint64_t at = clamp_row<Cfg::kClamp, IdxT>(r[k], last_row) * row_stride;
                v[k] = Mx4Piece{load_row<Cfg::kNtRow>(wsub + at), load_mx4_scale(ssub + at)};
            }
        }
#pragma unroll
        for (int k = 0; k < U; k++)
            if (use[k]) {
                const f32x32 x = widen_mx4x32(v[k]);
#pragma unroll
                for (int c = 0; c < 32; c++) acc[c] = pool_op1(acc[c], x[c], w[k], a.op, cnt == 0u);
                cnt++;
            }
    }
}

// The two kernels themselves: pimemb_mx4_kernels.inc, under the names tests/test_mxfp4_cpu.py pins (28 kernels with `mx4`).
#define PIMEMB_MX4_KERNEL(op) bag_mx4##op##_group_kernel
#include "pimemb_mx4_kernels.inc"
#undef PIMEMB_MX4_KERNEL
#undef PIMEMB_OUT_STRIDE

// ---- strided pooled output (emb_lookup_strided / emb_plan_create_strided): the twins -----------------------------------------
// A strided descriptor's pooled rows are DevDesc::words[kOutStrideWord] floats apart instead of back to back -- one table's columns of a
// [B, T * dim] buffer.  Every store path above addresses a row as out + bag * out_stride and stores relative to it, so the twins
// are the SAME text with the stride read from the descriptor (wave-uniform: a scalar load next to the other fields) instead of
// computed from `chunks`.  New instantiations under names of their own, not a runtime branch: the kernels above keep their machine
// code, and the names hold none of the fragments the tests pin kernel sets by (bag_sum_, bag_pool_, bag_bf16pool_, bag_f8pool_,
// bag_hpool_, mx4).  One pooled set serves every dtype.  No ranged, hot-row, any-dim or half-output twin.
#define PIMEMB_OUT_STRIDE(dp, dense) ((uint32_t)(dp)->words[kOutStrideWord])
#define PIMEMB_SUM_KERNEL(path) bag_strided_sum_##path##_kernel
#include "pimemb_sum_kernels.inc"
#undef PIMEMB_SUM_KERNEL
#define PIMEMB_POOL_KERNEL(path) bag_strided_pool_##path##_kernel
#define PIMEMB_POOL_HALF_OUT 0
#define PIMEMB_POOL_ROWOPS(DT) RowOps<DT>
#include "pimemb_pool_kernels.inc"
#undef PIMEMB_POOL_KERNEL
#undef PIMEMB_POOL_HALF_OUT
#undef PIMEMB_POOL_ROWOPS
#define PIMEMB_MX4_KERNEL(op) bag_strided_e2m1##op##_group_kernel
#include "pimemb_mx4_kernels.inc"
#undef PIMEMB_MX4_KERNEL
#undef PIMEMB_OUT_STRIDE

}  // namespace pimemb
