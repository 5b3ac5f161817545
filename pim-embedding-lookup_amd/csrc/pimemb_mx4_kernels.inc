// pimemb_mx4_kernels.inc -- the two MXFP4 lane-group kernels, sum and pooled.  Included by pimemb_bag_kernels.h, inside namespace
// pimemb, once per set of entry-point names: PIMEMB_MX4_KERNEL(op) names the kernel of op (sum, pool) and PIMEMB_OUT_STRIDE(dp,
// dense) is the distance in floats between two bags' pooled rows -- `dense` for bag_mx4sum_* / bag_mx4pool_*, the descriptor's
// DevDesc::words[3] for the strided twins bag_strided_e2m1sum_* / bag_strided_e2m1pool_*.

template <typename IdxT, int LPR, class Cfg>
__global__ void __launch_bounds__(Cfg::kBlock)
PIMEMB_MX4_KERNEL(sum)(const DevDesc *__restrict__ descs, uint32_t chunks_arg, const uint32_t *__restrict__ xmap) {
    using Ops = RowOps<kMXFP4>;
    constexpr uint32_t kWaves = Cfg::kBlock / 64;
    constexpr uint32_t BPW = 64 / LPR;
    constexpr uint32_t BAGS_PER_TILE = BPW * kWaves;

    uint32_t desc_i, tile;
    if (!decode_block(xmap, chunks_arg & kXmapDirect, &desc_i, &tile)) return;
    const uint32_t chunks = chunks_arg & ~kXmapDirect;
    const DescView<IdxT> t(descs + desc_i);

    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t sub = lane & (LPR - 1), grp = lane / LPR;
    const uint32_t row_stride = mx4_row_stride(chunks);
    const uint32_t out_stride = PIMEMB_OUT_STRIDE(descs + desc_i, chunks * Ops::kFloatsPerLane);
    const char *__restrict__ wsub = t.weights + sub * 16u;              // this lane's block of row 0 ...
    const char *__restrict__ ssub = t.weights + chunks * 16u + sub;     // ... and that block's scale

    if (tile < t.n_tiles) {
        const uint64_t bag = (uint64_t)tile * BAGS_PER_TILE + wave * BPW + grp;
        const bool live = sub < chunks;
        if (bag >= t.n_bags) return;                   // whole lane group leaves together
        uint64_t p, e;
        bag_range<Cfg::kNtMeta, Cfg::kClamp>(t.offsets, t.n_bags, t.n_idx, t.fixed_pooling, bag, p, e);
        typename Ops::Acc acc = Ops::zero();
        walk_bag<IdxT, LPR, Cfg, Ops>(t.indices, p, e, sub, grp, live, acc, NoProbe{}, [&](uint64_t r, uint32_t) -> Mx4Piece {
            const uint64_t at = clamp_row<Cfg::kClamp, IdxT>(r, t.last_row) * row_stride;
            return Mx4Piece{load_row<Cfg::kNtRow>(wsub + at), load_mx4_scale(ssub + at)};
        });
        store_row<Ops, Cfg, LPR>(acc, t.out + bag * out_stride, sub, grp, chunks, live);
    }
}

template <typename IdxT, int LPR, class Cfg>
__global__ void __launch_bounds__(Cfg::kBlock)
PIMEMB_MX4_KERNEL(pool)(const DevDesc *__restrict__ descs, uint32_t chunks_arg, const uint32_t *__restrict__ xmap) {
    using Ops = RowOps<kMXFP4>;
    constexpr uint32_t kWaves = Cfg::kBlock / 64;
    constexpr uint32_t BPW = 64 / LPR;
    constexpr uint32_t BAGS_PER_TILE = BPW * kWaves;

    uint32_t desc_i, tile;
    if (!decode_block(xmap, chunks_arg & kXmapDirect, &desc_i, &tile)) return;
    const uint32_t chunks = chunks_arg & ~kXmapDirect;
    const DevDesc *dp = descs + desc_i;
    const DescView<IdxT> t(dp);
    const PoolArgs a = pool_args(dp);

    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t sub = lane & (LPR - 1), grp = lane / LPR;
    const uint32_t row_stride = mx4_row_stride(chunks);
    const uint32_t out_stride = PIMEMB_OUT_STRIDE(dp, chunks * Ops::kFloatsPerLane);
    const char *__restrict__ wsub = t.weights + sub * 16u;
    const char *__restrict__ ssub = t.weights + chunks * 16u + sub;

    if (tile < t.n_tiles) {
        const uint64_t bag = (uint64_t)tile * BAGS_PER_TILE + wave * BPW + grp;
        const bool live = sub < chunks;
        if (bag >= t.n_bags) return;                   // whole lane group leaves together
        uint64_t p, e;
        bag_range<Cfg::kNtMeta, Cfg::kClamp>(t.offsets, t.n_bags, t.n_idx, t.fixed_pooling, bag, p, e);
        typename Ops::Acc acc = Ops::zero();
        uint32_t cnt = 0;
        if (live) mx4_pool_walk<IdxT, Cfg>(t.indices, a, p, e, wsub, ssub, row_stride, t.last_row, acc, cnt);
        if (a.mean && cnt > 1u) {
#pragma unroll
            for (int c = 0; c < 32; c++) acc[c] = pool_finish1(acc[c], cnt, true);
        }
        store_row<Ops, Cfg, LPR>(acc, t.out + bag * out_stride, sub, grp, chunks, live);
    }
}
