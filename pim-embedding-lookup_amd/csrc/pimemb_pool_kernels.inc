// pimemb_pool_kernels.inc -- the three kernels of the pooled family (mean / max pooling, per-sample weights, padding_idx).
// Included by pimemb_bag_kernels.h, inside namespace pimemb, ONCE PER SET OF ENTRY-POINT NAMES: PIMEMB_POOL_KERNEL(path) names
// the kernel of a path (group, wavebatch, anydim); PIMEMB_POOL_ROWOPS(DT) is the accumulate / store trait and
// PIMEMB_POOL_HALF_OUT says whether the set stores fp32 rows (0) or rows of the table's 2-byte dtype (1).  PIMEMB_OUT_STRIDE(dp,
// dense) is the distance in floats between two bags' pooled rows: `dense` everywhere but in the strided set, which reads it from
// the descriptor (DevDesc::words[3]; the group and wave-batch paths only: the set's any-dim kernel is never instantiated).
// The same text compiled under five sets of names -- bag_pool_* (fp32, fp16), bag_bf16pool_* (bf16), bag_f8pool_* (fp8),
// bag_hpool_* (half-width output of fp16 and bf16 tables), bag_strided_pool_* (strided fp32 output, every dtype) -- so that
// the kernels of the first set keep their machine code to the byte (as bodies
// shared by thin kernels they do not: inlined, 50 of the 64 fp32 / fp16 pooled kernels change, some by up to 4 VGPRs).

// Lane-group path (ragged bags, rows of 16-byte multiples up to 1 KiB): one lane group per bag, as bag_sum_group_kernel.
template <typename IdxT, int DT, int LPR, class Cfg>
__global__ void __launch_bounds__(Cfg::kBlock)
PIMEMB_POOL_KERNEL(group)(const DevDesc *__restrict__ descs, uint32_t chunks_arg, const uint32_t *__restrict__ xmap) {
    using Ops = PIMEMB_POOL_ROWOPS(DT);
    constexpr uint32_t kWaves = Cfg::kBlock / 64;
    constexpr uint32_t BPW = 64 / LPR;
    constexpr uint32_t BAGS_PER_TILE = BPW * kWaves;

    uint32_t desc_i, tile;
    if (!decode_block(xmap, chunks_arg & kXmapDirect, &desc_i, &tile)) return;
    const uint32_t chunks = chunks_arg & ~kXmapDirect;
    const DevDesc *dp = descs + desc_i;
    const DescView<IdxT> t(dp);
    const PoolArgs a = pool_args(dp);

    // (a LaneGeom here changes the code object of this kernel's 4 one-lane-per-row instantiations)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t sub = lane & (LPR - 1), grp = lane / LPR;
    const uint32_t row_bytes = chunks * 16u;
    const uint32_t out_stride = PIMEMB_OUT_STRIDE(dp, chunks * Ops::kFloatsPerLane);
    const char *__restrict__ wsub = t.weights + sub * 16u;

    if (tile < t.n_tiles) {
        const uint64_t bag = (uint64_t)tile * BAGS_PER_TILE + wave * BPW + grp;
        const bool live = sub < chunks;
        if (bag >= t.n_bags) return;                   // whole lane group leaves together
        uint64_t p, e;
        bag_range<Cfg::kNtMeta, Cfg::kClamp>(t.offsets, t.n_bags, t.n_idx, t.fixed_pooling, bag, p, e);
        typename Ops::Acc acc = Ops::zero();
        uint32_t cnt = 0;
        if (live) pool_walk<IdxT, DT, Cfg>(t.indices, a, p, e, wsub, row_bytes, t.last_row, acc, cnt);
        pool_finish<DT>(acc, cnt, a.mean);
        store_row<Ops, Cfg, LPR>(acc, t.out + bag * out_stride, sub, grp, chunks, live);
    }
}

// Wave-batch path (big batches): 64 bags per wavefront with coalesced bounds, as bag_sum_wavebatch_kernel (one batch per
// step).  One-hot steps -- DLRM's weighted pooling on Criteo shapes -- load the bag's index AND its weight coalesced (both
// speculatively, in the shadow of the bounds), issue every round's gather before the first store and store non-temporally;
// a padding entry makes its bag empty.  Longer bags: each round a lane group walks its bag (pool_walk).
template <typename IdxT, int DT, int LPR, class Cfg>
__global__ void __launch_bounds__(Cfg::kBlock, Cfg::kMinWaves)
PIMEMB_POOL_KERNEL(wavebatch)(const DevDesc *__restrict__ descs, uint32_t chunks_arg, const uint32_t *__restrict__ xmap) {
    using Ops = PIMEMB_POOL_ROWOPS(DT);
    constexpr uint32_t kWaves = Cfg::kBlock / 64;
    constexpr uint32_t BPR = 64 / LPR;      // bags per round
    constexpr uint32_t ROUNDS = LPR;        // rounds per 64-bag wave batch
    constexpr uint32_t RU = onehot_rounds_in_flight<LPR, Cfg>();

    uint32_t desc_i, tile;
    if (!decode_block(xmap, chunks_arg & kXmapDirect, &desc_i, &tile)) return;
    const uint32_t chunks = chunks_arg & ~kXmapDirect;
    const DevDesc *dp = descs + desc_i;
    // (a DescView here changes the code object of the two fp32 two-lanes-per-row instantiations)
    const char *__restrict__ weights = static_cast<const char *>(dp->weights);
    const IdxT *__restrict__ indices = static_cast<const IdxT *>(dp->indices);
    const IdxT *__restrict__ offsets = static_cast<const IdxT *>(dp->offsets);
    float *__restrict__ out = dp->out;
    const uint64_t n_idx = dp->n_idx, n_bags = dp->n_bags, last_row = dp->nr_rows - 1;
    const uint32_t fixed_pooling = dp->fixed_pooling, n_tiles = dp->n_tiles;
    const PoolArgs a = pool_args(dp);
    const LaneGeom<LPR, Ops> ln(weights, chunks);
    const bool lane_live = ln.sub < chunks;
    const uint32_t out_stride = PIMEMB_OUT_STRIDE(dp, ln.out_stride);    // floats between two bags' pooled rows: read ONCE, with the descriptor's other fields

    if (tile >= n_tiles) return;
    const uint64_t step_base = ((uint64_t)tile * kWaves + ln.wave) * 64u;
    if (step_base >= n_bags) return;  // wave-uniform

    // lane l holds the bounds of bag step_base + l (past-the-end = empty)
    const uint64_t mb = step_base + ln.lane;
    IdxT spec = 0;
    float spec_w = 1.f;
    if (mb < n_idx) {
        spec = load_meta<Cfg::kNtMeta>(indices + mb);
        if (a.psw != nullptr) spec_w = load_meta<Cfg::kNtMeta>(a.psw + mb);
    }
    uint64_t st, en;    // (shared with bag_sum_wavebatch_kernel's block as a function: every instantiation changes)
    if (offsets != nullptr) {
        st = (mb < n_bags) ? (uint64_t)load_meta<Cfg::kNtMeta>(offsets + mb) : n_idx;
        en = (mb + 1 < n_bags) ? (uint64_t)load_meta<Cfg::kNtMeta>(offsets + mb + 1) : n_idx;
    } else {
        st = (mb < n_bags ? mb : n_bags) * fixed_pooling;
        en = (mb + 1 < n_bags ? mb + 1 : n_bags) * fixed_pooling;
    }
    if (Cfg::kClamp) {
        if (en > n_idx) en = n_idx;
        if (st > en) st = en;
    }
    uint32_t len = (uint32_t)(en - st);

    if (__all(len <= 1u)) {
        IdxT my = 0;
        float my_w = 1.f;
        if (len) {
            const bool at_spec = st == mb;
            my = at_spec ? spec : load_meta<Cfg::kNtMeta>(indices + st);
            if (a.psw != nullptr) my_w = at_spec ? spec_w : load_meta<Cfg::kNtMeta>(a.psw + st);
            if ((uint64_t)my == a.pad) len = 0;     // the bag's only entry is padding: an empty bag
        }
#pragma unroll
        for (uint32_t j0 = 0; j0 < ROUNDS; j0 += RU) {
            u32x4 v[RU];
            bool has[RU];
#pragma unroll
            for (uint32_t jj = 0; jj < RU; jj++) {
                const uint32_t src = (j0 + jj) * BPR + ln.grp;
                const uint64_t r = clamp_row<Cfg::kClamp, IdxT>(shfl_index<IdxT>(my, src), last_row);
                has[jj] = shfl_u32(len, src) != 0u;
                v[jj] = u32x4{0u, 0u, 0u, 0u};
                if (has[jj] && lane_live) v[jj] = load_row<Cfg::kNtRow>(ln.wsub + r * ln.row_bytes);
            }
#pragma unroll
            for (uint32_t jj = 0; jj < RU; jj++) {
                const uint32_t src = (j0 + jj) * BPR + ln.grp;
                const uint64_t bag = step_base + src;
                const float w = shfl_f32(my_w, src);
                typename Ops::Acc acc = Ops::zero();
                if (has[jj] && lane_live) pool_combine<DT>(acc, v[jj], w, a.op, true);
                // (all lanes take part in a group store's shuffles)
                store_row<Ops, Cfg, LPR>(acc, out + bag * out_stride, ln.sub, ln.grp, chunks, bag < n_bags && lane_live);
            }
        }
        return;
    }

    // general step: each round, a lane group walks its bag in index order
#pragma unroll 1
    for (uint32_t j = 0; j < ROUNDS; j++) {
        const uint32_t src = j * BPR + ln.grp;
        const uint64_t p = shfl_u64(st, src);
        const uint64_t e = p + shfl_u32(len, src);
        const uint64_t bag = step_base + src;
        // (no early `continue`: every lane must reach the next round's shuffles)
        typename Ops::Acc acc = Ops::zero();
        uint32_t cnt = 0;
        if (bag < n_bags && lane_live) pool_walk<IdxT, DT, Cfg>(indices, a, p, e, ln.wsub, ln.row_bytes, last_row, acc, cnt);
        pool_finish<DT>(acc, cnt, a.mean);
        store_row<Ops, Cfg, LPR>(acc, out + bag * out_stride, ln.sub, ln.grp, chunks, bag < n_bags && lane_live);
    }
}

// Any-dim path: rows that are not 16-byte multiples or wider than 1 KiB, as bag_sum_anydim[_vec]_kernel.  VEC: one thread
// per 16-byte piece of a 4-byte-multiple row (a partial last piece dword by dword), else one thread per element.
template <typename IdxT, int DT, bool VEC, bool CLAMP>
__global__ void __launch_bounds__(256)
PIMEMB_POOL_KERNEL(anydim)(const DevDesc *__restrict__ descs, uint32_t dim, uint32_t lanes) {
    constexpr uint32_t EP = VEC ? (uint32_t)PoolRow<DT>::K : 1u;    // elements per unit
    constexpr uint32_t ESZ = elem_bytes(DT);
    constexpr int U = 4;
    const DevDesc *dp = descs + blockIdx.y;
    const char *__restrict__ weights = static_cast<const char *>(dp->weights);
    const IdxT *__restrict__ indices = static_cast<const IdxT *>(dp->indices);
    const IdxT *__restrict__ offsets = static_cast<const IdxT *>(dp->offsets);
    float *__restrict__ out = dp->out;
    const uint64_t n_idx = dp->n_idx, n_bags = dp->n_bags, last_row = dp->nr_rows - 1;
    const uint64_t bag = (uint64_t)blockIdx.x * (256u / lanes) + threadIdx.x / lanes;
    if (blockIdx.x >= dp->n_tiles || bag >= n_bags) return;
    const PoolArgs a = pool_args(dp);
    uint64_t p0, e;
    bag_range<false, CLAMP>(offsets, n_bags, n_idx, dp->fixed_pooling, bag, p0, e);
    const uint32_t row_bytes = dim * ESZ, units = (dim + EP - 1) / EP;
    for (uint32_t unit = threadIdx.x & (lanes - 1); unit < units; unit += lanes) {
        const uint32_t n_el = (dim - unit * EP < EP) ? dim - unit * EP : EP;
        const char *__restrict__ wp = weights + unit * EP * ESZ;
        float acc[EP];
#pragma unroll
        for (uint32_t c = 0; c < EP; c++) acc[c] = 0.f;
        uint32_t cnt = 0;
        for (uint64_t p = p0; p < e; p += U) {
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
                    r[k] = (uint64_t)indices[p + k];
                    if (a.psw != nullptr) w[k] = a.psw[p + k];
                }
                use[k] = use[k] && r[k] != a.pad;
            }
            float x[U][EP];
#pragma unroll
            for (int k = 0; k < U; k++) {
                const char *src = wp + clamp_row<CLAMP, IdxT>(r[k], last_row) * row_bytes;
                if constexpr (VEC) {
                    u32x4 v = {0u, 0u, 0u, 0u};
                    if (use[k]) {
                        if (n_el == EP) {
                            v = *reinterpret_cast<const u32x4_a4 *>(src);
                        } else {                         // partial last piece: whole dwords only
                            const uint32_t n_dw = n_el * ESZ / 4u;
                            for (uint32_t d = 0; d < n_dw; d++) v[d] = reinterpret_cast<const uint32_t *>(src)[d];
                        }
                    }
                    const auto f = PoolRow<DT>::widen(v);
#pragma unroll
                    for (uint32_t c = 0; c < EP; c++) x[k][c] = f[c];
                } else {
                    x[k][0] = 0.f;
                    if (use[k]) {
                        if constexpr (DT == EMB_F16) x[k][0] = (float)*reinterpret_cast<const _Float16 *>(src);
                        else if constexpr (DT == EMB_BF16) x[k][0] = ElemOps<EMB_BF16>::widen(*reinterpret_cast<const uint16_t *>(src));
                        else if constexpr (kIsF8<DT>) x[k][0] = ElemOps<DT>::widen(*reinterpret_cast<const uint8_t *>(src));
                        else x[k][0] = *reinterpret_cast<const float *>(src);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < U; k++)
                if (use[k]) {
#pragma unroll
                    for (uint32_t c = 0; c < EP; c++) acc[c] = pool_op1(acc[c], x[k][c], w[k], a.op, cnt == 0u);
                    cnt++;
                }
        }
#pragma unroll
        for (uint32_t c = 0; c < EP; c++) acc[c] = pool_finish1(acc[c], cnt, a.mean);
#if PIMEMB_POOL_HALF_OUT    // rounded once to the table's dtype: a full piece is 16 B of halves at a 4-byte aligned address
        uint16_t *o = reinterpret_cast<uint16_t *>(out) + bag * dim + unit * EP;
        if constexpr (VEC) {
            f32x8 a8;
#pragma unroll
            for (uint32_t c = 0; c < EP; c++) a8[c] = acc[c];
            const u32x4 h = HalfRound<DT>::pack(a8);
            if (n_el == EP) {
                *reinterpret_cast<u32x4_a4 *>(o) = h;
            } else {
#pragma unroll
                for (uint32_t c = 0; c < EP; c++)
                    if (c < n_el) o[c] = (uint16_t)(h[c / 2] >> (16u * (c & 1u)));
            }
        } else {
            o[0] = HalfRound<DT>::one(acc[0]);
        }
#else
        float *o = out + bag * dim + unit * EP;
        bool stored = false;
        if constexpr (VEC) {
            if (n_el == EP) {
#pragma unroll
                for (uint32_t c = 0; c < EP; c += 4)
                    *reinterpret_cast<f32x4_a4 *>(o + c) = f32x4{acc[c], acc[c + 1], acc[c + 2], acc[c + 3]};
                stored = true;
            }
        }
        if (!stored)
            for (uint32_t c = 0; c < n_el; c++) o[c] = acc[c];
#endif
    }
}
