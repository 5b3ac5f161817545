// pimemb_sum_kernels.inc -- the lane-group and the wave-batch kernel of the plain-sum family.
// Included by pimemb_bag_kernels.h, inside namespace pimemb, ONCE PER SET OF ENTRY-POINT NAMES: PIMEMB_SUM_KERNEL(path) names the
// kernel of a path (group, wavebatch) and PIMEMB_OUT_STRIDE(dp, dense) is the distance in floats from one bag's pooled row to the
// next: `dense` (chunks * kFloatsPerLane, rows back to back) for bag_sum_*, the descriptor's DevDesc::words[3] for the strided
// twins bag_strided_sum_* (emb_lookup_strided).  The same text under two sets of names, as pimemb_pool_kernels.inc, so that the
// bag_sum_* kernels keep their machine code to the byte: the macro leaves them the expression they always had.

// ---- v1: one lane group per bag, no cross-lane traffic (kept as the A/B baseline) -------------
template <typename IdxT, int DT, int LPR, class Cfg>
__global__ void __launch_bounds__(Cfg::kBlock)
PIMEMB_SUM_KERNEL(group)(const DevDesc *__restrict__ descs, uint32_t chunks_arg,
                     const uint32_t *__restrict__ xmap) {
    using Ops = RowOps<DT>;
    constexpr uint32_t kWaves = Cfg::kBlock / 64;
    constexpr uint32_t BPW = 64 / LPR;
    constexpr uint32_t BAGS_PER_TILE = BPW * kWaves;

    uint32_t desc_i, tile;
    if (!decode_block(xmap, chunks_arg & kXmapDirect, &desc_i, &tile)) return;
    const uint32_t chunks = chunks_arg & ~kXmapDirect;
    const DescView<IdxT> t(descs + desc_i);

    // (a LaneGeom here changes the code object of 30 of this kernel's 42 instantiations)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t sub = lane & (LPR - 1), grp = lane / LPR;
    const uint32_t row_bytes = chunks * 16u;
    const uint32_t out_stride = PIMEMB_OUT_STRIDE(descs + desc_i, chunks * Ops::kFloatsPerLane);
    const char *__restrict__ wsub = t.weights + sub * 16u;

    if (tile < t.n_tiles) {
        const uint64_t bag = (uint64_t)tile * BAGS_PER_TILE + wave * BPW + grp;
        const bool live = sub < chunks;
        if (bag >= t.n_bags) return;                   // whole lane group leaves together
        uint64_t p, e;
        // (bag_range() spelled out: calling it changes the code object of 28 of the 42 instantiations, same registers, no spill)
        if (t.offsets != nullptr) {
            p = (uint64_t)load_meta<Cfg::kNtMeta>(t.offsets + bag);
            e = (bag + 1 < t.n_bags) ? (uint64_t)load_meta<Cfg::kNtMeta>(t.offsets + bag + 1) : t.n_idx;
        } else {
            p = bag * t.fixed_pooling;
            e = p + t.fixed_pooling;
        }
        if (Cfg::kClamp && e > t.n_idx) e = t.n_idx;
        typename Ops::Acc acc = Ops::zero();
        walk_bag<IdxT, LPR, Cfg, Ops>(t.indices, p, e, sub, grp, live, acc, NoProbe{},
                                      [&](uint64_t r, uint32_t) -> u32x4 {
                                          return load_row<Cfg::kNtRow>(wsub + clamp_row<Cfg::kClamp, IdxT>(r, t.last_row) * row_bytes);
                                      });
        store_row<Ops, Cfg, LPR>(acc, t.out + bag * out_stride, sub, grp, chunks, live);
    }
}

// ---- v2: wave batches of 64 bags, coalesced bounds, shuffle-distributed, one-hot fast path -------
// RANGED (the sharded lookup's direct path, pimemb_shard.cpp): one index per bag, and a descriptor serves only the bags
// whose row falls into [row_lo, row_lo + nr_rows) (DevDesc::ranged.row_lo): out[b] = W[idx[b] - row_lo]; the other bags
// are left untouched -- another shard of the table writes them, straight into the same output (DevDesc::ranged.served, if not null: a
// uint32 counter in HBM the launch adds the number of bags it served to).  A shard scans the
// requester's RAW index array (its own, or a peer's through its mapping): no router, no counts, no un-router.  A whole
// table is the range [0, nr_rows), so replicated tables and shards share ONE launch of the tuned kernel.
// (The strided twin is instantiated with RANGED = false only: ranged launches stay dense.)
template <typename IdxT, int DT, int LPR, class Cfg, bool RANGED = false>
__global__ void __launch_bounds__(Cfg::kBlock, Cfg::kMinWaves)
PIMEMB_SUM_KERNEL(wavebatch)(const DevDesc *__restrict__ descs, uint32_t chunks_arg,
                         const uint32_t *__restrict__ xmap) {
    using Ops = RowOps<DT>;
    constexpr uint32_t kWaves = Cfg::kBlock / 64;
    constexpr uint32_t BPR = 64 / LPR;      // bags per round
    constexpr uint32_t ROUNDS = LPR;        // rounds per 64-bag wave batch
    constexpr uint32_t NB = Cfg::kBatches;  // wave batches per step
    constexpr int U = Cfg::kUnroll;
    constexpr uint32_t RU = onehot_rounds_in_flight<LPR, Cfg>();

    uint32_t desc_i, tile;
    if (!decode_block(xmap, chunks_arg & kXmapDirect, &desc_i, &tile)) return;
    const uint32_t chunks = chunks_arg & ~kXmapDirect;
    const DevDesc *dp = descs + desc_i;
    const DescView<IdxT> t(dp);

    const LaneGeom<LPR, Ops> ln(t.weights, chunks);
    const bool lane_live = ln.sub < chunks;
    const uint32_t out_stride = PIMEMB_OUT_STRIDE(dp, ln.out_stride);    // floats between two bags' pooled rows: read ONCE, with the descriptor's other fields
    uint64_t row_lo = 0;
    bool open_end = false;               // RANGED: ids at or beyond the end of this range are this descriptor's to ZERO (EMB_RANGE_OPEN_END)
    uint32_t *served_ctr = nullptr;      // RANGED: where this descriptor's launch adds the number of bags it served (or null)
    if constexpr (RANGED) {
        row_lo = dp->ranged.row_lo & ~kRangeOpenEnd;
        open_end = (dp->ranged.row_lo & kRangeOpenEnd) != 0;
        served_ctr = dp->ranged.served;
    }

    if (tile < t.n_tiles) {
        const uint64_t step_base = ((uint64_t)tile * kWaves + ln.wave) * (64u * NB);
        if (step_base >= t.n_bags) return;  // wave-uniform

        // lane l of batch q holds the bounds of bag step_base + 64q + l (past-the-end = empty)
        uint64_t st[NB];
        uint32_t len[NB];
        bool small = true;
        // Speculation: in a one-hot batch with contiguous bags offsets[b] == b, so bag b's only index
        // sits at indices[b].  Fetch it NOW, in the shadow of the bounds loads, and keep it only if
        // the bounds agree -- one memory round trip less on the critical path of the Kaggle shape.
        IdxT spec[NB];
        if constexpr (Cfg::kSpeculate) {
#pragma unroll
            for (uint32_t q = 0; q < NB; q++) {
                const uint64_t mb = step_base + 64u * q + ln.lane;
                spec[q] = 0;
                if (mb < t.n_idx) spec[q] = load_meta<Cfg::kNtMeta>(t.indices + mb);
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < NB; q++) {
            const uint64_t mb = step_base + 64u * q + ln.lane;
            uint64_t en;    // (this block as a function shared with bag_pool_wavebatch_kernel: 18 instantiations here, 28 there change)
            if (t.offsets != nullptr) {
                st[q] = (mb < t.n_bags) ? (uint64_t)load_meta<Cfg::kNtMeta>(t.offsets + mb) : t.n_idx;
                en = (mb + 1 < t.n_bags) ? (uint64_t)load_meta<Cfg::kNtMeta>(t.offsets + mb + 1) : t.n_idx;
            } else {
                st[q] = (mb < t.n_bags ? mb : t.n_bags) * t.fixed_pooling;
                en = (mb + 1 < t.n_bags ? mb + 1 : t.n_bags) * t.fixed_pooling;
            }
            if (Cfg::kClamp) {                       // malformed offsets: keep [st, en) inside [0, n_idx]
                if (en > t.n_idx) en = t.n_idx;
                if (st[q] > en) st[q] = en;
            }
            len[q] = (uint32_t)(en - st[q]);
            small = small && (len[q] <= 1u);
        }

        if (__all(small)) {
            // one-hot step: lane l fetches its bag's only index (coalesced), groups pull theirs and
            // every gather of the step is issued before the first store.
            IdxT my[NB];
#pragma unroll
            for (uint32_t q = 0; q < NB; q++) {
                my[q] = 0;
                if constexpr (Cfg::kSpeculate) {
                    const uint64_t mb = step_base + 64u * q + ln.lane;
                    if (len[q]) my[q] = (st[q] == mb) ? spec[q] : load_meta<Cfg::kNtMeta>(t.indices + st[q]);
                } else {
                    if (len[q]) my[q] = load_meta<Cfg::kNtMeta>(t.indices + st[q]);
                }
                if constexpr (RANGED) {     // row ids relative to this shard; a bag of another shard counts as empty
                    const uint64_t id = (uint64_t)my[q];               // (a negative int64 id: huge, beyond every range)
                    const uint64_t r = id - row_lo;                    // (wraps far out of range below row_lo)
                    // len: 1 = served here; 2 = an id no range holds, and this descriptor answers for the open end: the bag's
                    // pooled row is written as zeros (not served, not counted); 0 = some other shard's bag, left alone
                    if (r > t.last_row) len[q] = (len[q] && open_end && id >= row_lo) ? 2u : 0u;
                    my[q] = (IdxT)r;
                }
            }
            if constexpr (RANGED) {
                // Counted launch (a checked shard's direct path): the bags this wavefront serves, one atomic per wavefront,
                // no return value.  The requester adds the counts of all shards up: a sum short of its bag count means an
                // index no shard holds -- a bag left untouched (pimemb_shard.cpp: stage_unroute).
                // A counter is EMB_SERVED_LANES words EMB_SERVED_STRIDE bytes apart, a workgroup adds to lane blockIdx % LANES:
                // agent-scope atomics on ONE line retire one by one (~5.5 ns each: 8 000 wavefronts of the Kaggle launch on 26
                // neighbouring words took 44 us against the lookup's 20), spread over lines they cost nothing measurable.
                if (served_ctr != nullptr) {     // wave-uniform (a scalar load of the descriptor)
                    uint32_t n = 0;
#pragma unroll
                    for (uint32_t q = 0; q < NB; q++) n += (uint32_t)__popcll(__ballot(len[q] == 1u));
                    uint32_t *slot = served_ctr + (size_t)(blockIdx.x % EMB_SERVED_LANES) * (EMB_SERVED_STRIDE / 4u);
                    if (ln.lane == 0 && n) (void)__hip_atomic_fetch_add(slot, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
#pragma unroll
            for (uint32_t j0 = 0; j0 < ROUNDS; j0 += RU) {
                u32x4 v[NB][RU];
                bool has[NB][RU];
                bool zero_it[NB][RU];      // (RANGED only: the open end's bags)
#pragma unroll
                for (uint32_t q = 0; q < NB; q++)
#pragma unroll
                    for (uint32_t jj = 0; jj < RU; jj++) {
                        const uint32_t src = (j0 + jj) * BPR + ln.grp;
                        const uint64_t r = clamp_row<Cfg::kClamp, IdxT>(shfl_index<IdxT>(my[q], src), t.last_row);
                        const uint32_t l = shfl_u32(len[q], src);
                        has[q][jj] = RANGED ? l == 1u : l != 0u;
                        zero_it[q][jj] = RANGED && l == 2u;
                        v[q][jj] = u32x4{0u, 0u, 0u, 0u};
                        if (has[q][jj] && lane_live) v[q][jj] = load_row<Cfg::kNtRow>(ln.wsub + r * ln.row_bytes);
                    }
#pragma unroll
                for (uint32_t q = 0; q < NB; q++)
#pragma unroll
                    for (uint32_t jj = 0; jj < RU; jj++) {
                        const uint64_t bag = step_base + 64u * q + (j0 + jj) * BPR + ln.grp;
                        // (RANGED: only the bags this shard holds the row of are written)
                        const bool wr = RANGED ? (has[q][jj] || zero_it[q][jj]) : bag < t.n_bags;
                        // (store_row alone, which covers both cases, changes the code object of 50 instantiations)
                        if constexpr (!Ops::kGroupStore) {
                            if (wr && lane_live) {
                                typename Ops::Acc acc = Ops::zero();
                                if (has[q][jj]) Ops::add(acc, v[q][jj]);
                                Ops::template store<Cfg::kNtStore>(
                                    acc, t.out + bag * out_stride + ln.sub * Ops::kFloatsPerLane);
                            }
                        } else {   // all lanes take part in the group store's shuffles
                            typename Ops::Acc acc = Ops::zero();
                            // (fp8: a piece that was not gathered is all zero bytes, which widen to +0, and +0 + +0 = +0 --
                            // added without the test, the eight conversions stay out of a branch per gathered row)
                            if constexpr (kIsF8<DT>) Ops::add(acc, v[q][jj]);
                            else if (has[q][jj] && lane_live) Ops::add(acc, v[q][jj]);
                            store_row<Ops, Cfg, LPR>(acc, t.out + bag * out_stride, ln.sub, ln.grp, chunks,
                                                     wr && lane_live);
                        }
                    }
            }
            return;
        }
        if constexpr (RANGED) return;      // (the host hands a ranged launch fixed_pooling 1 only: every step is one-hot)

        // general step: each round, a lane group walks its bag in index order (walk_bag's non-shuffle loop, spelled out: a call of
        // walk_bag changes the code object of 46 instantiations)
#pragma unroll 1
        for (uint32_t q = 0; q < NB; q++) {
#pragma unroll 1
            for (uint32_t j = 0; j < ROUNDS; j++) {
                const uint32_t src = j * BPR + ln.grp;
                uint64_t p = shfl_u64(st[q], src);
                const uint64_t e = p + shfl_u32(len[q], src);
                const uint64_t bag = step_base + 64u * q + src;
                // (no early `continue`: every lane must reach the next round's shuffles)
                typename Ops::Acc acc = Ops::zero();
                if (bag < t.n_bags && lane_live) {
                    for (; p + U <= e; p += U) {
                        uint64_t r[U];
#pragma unroll
                        for (int k = 0; k < U; k++) r[k] = (uint64_t)load_meta<Cfg::kNtMeta>(t.indices + p + k);
                        u32x4 v[U];
#pragma unroll
                        for (int k = 0; k < U; k++)
                            v[k] = load_row<Cfg::kNtRow>(ln.wsub + clamp_row<Cfg::kClamp, IdxT>(r[k], t.last_row) * ln.row_bytes);
#pragma unroll
                        for (int k = 0; k < U; k++) Ops::add(acc, v[k]);
                    }
                    for (; p < e; p++) {
                        const uint64_t r = clamp_row<Cfg::kClamp, IdxT>((uint64_t)load_meta<Cfg::kNtMeta>(t.indices + p), t.last_row);
                        Ops::add(acc, load_row<Cfg::kNtRow>(ln.wsub + r * ln.row_bytes));
                    }
                    if constexpr (!Ops::kGroupStore)
                        Ops::template store<Cfg::kNtStore>(acc, t.out + bag * out_stride + ln.sub * Ops::kFloatsPerLane);
                }
                if constexpr (Ops::kGroupStore)
                    store_row<Ops, Cfg, LPR>(acc, t.out + bag * out_stride, ln.sub, ln.grp, chunks, bag < t.n_bags && lane_live);
            }
        }
    }
}
