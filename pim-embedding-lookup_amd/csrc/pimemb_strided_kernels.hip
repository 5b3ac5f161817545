// pimemb_strided_kernels.hip -- instantiates and launches the strided twins of the bag kernels (bag_strided_*,
// pimemb_bag_kernels.h; emb_lookup_strided / emb_plan_create_strided): the kernels that take the distance between two bags'
// pooled rows from their descriptor, so that a lookup writes one table's columns of a [B, T * dim] buffer.  gfx950 only.
// A translation unit of its own: its 338 kernels compile next to pimemb_kernels.hip's, and that unit's code object stays what it
// was.  Configurations and dispatch are pimemb_kernels.hip's own, word for word -- a twin runs under its dense kernel's: that file
// is included up to the end of them (PIMEMB_CONFIGURATIONS_ONLY).
#define PIMEMB_CONFIGURATIONS_ONLY
#include "pimemb_kernels.hip"

namespace pimemb {
namespace {

// One exception to "its dense kernel's configuration": 1-KiB fp32 rows under uint32 indices.  bag_sum_wavebatch_kernel<uint32_t,
// EMB_F32, 64, WaveCfg> is one register over its 64-VGPR cap (1 VGPR spilled, 8 bytes of scratch) and its twin inherits that; asked
// for 7 waves per SIMD instead of 8 the twin lands at 64 VGPRs without the spill -- and still fits 8 waves.
using WaveCfgStrided64 = BagCfg<64, 8, true, false, 8, 7, 1, false, true, false, kClampInputs>;

// The twins of launch_sum's three kernels (pimemb_kernels.hip): same grid, same arguments.  Never ranged.
template <typename IdxT, int DT, int L>
void launch_strided_sum(const DevDesc *d, dim3 grid, uint32_t chunks, KernelKind kind, const uint32_t *xmap, hipStream_t s) {
    using One = std::conditional_t<DT == EMB_F32 && L == 64 && sizeof(IdxT) == 4, WaveCfgStrided64, typename WaveCfgOf<DT>::One>;
    using Two = typename WaveCfgOf<DT>::Two;
    if (kind == KERNEL_WAVEBATCH)
        hipLaunchKernelGGL((bag_strided_sum_wavebatch_kernel<IdxT, DT, L, One, false>), grid, dim3(One::kBlock), 0, s, d, chunks, xmap);
    else if (kind == KERNEL_WAVEBATCH2) {
        if constexpr (L <= 4)       // (as launch_sum: choose_kernel hands the two-batch geometry out for narrow rows only)
            hipLaunchKernelGGL((bag_strided_sum_wavebatch_kernel<IdxT, DT, L, Two, false>), grid, dim3(Two::kBlock), 0, s, d, chunks, xmap);
    } else
        hipLaunchKernelGGL((bag_strided_sum_group_kernel<IdxT, DT, L, GroupCfg>), grid, dim3(GroupCfg::kBlock), 0, s, d, chunks, xmap);
}

}  // namespace

hipError_t launch_bag_strided(const DevDesc *d_descs, dim3 grid, uint32_t chunks_arg, int dtype, emb_index_type itype, const LaunchGeom &g,
                              KernelKind kind, const uint32_t *d_xmap, hipStream_t stream, bool pooled) {
    if (g.scalar_lanes) return hipErrorInvalidValue;                  // no any-dim twin
    if (pooled ? (kind != KERNEL_WAVEBATCH && kind != KERNEL_GROUP) : (kind != KERNEL_WAVEBATCH && kind != KERNEL_WAVEBATCH2 && kind != KERNEL_GROUP))
        return hipErrorInvalidValue;
    if (dtype == kMXFP4) {      // the lane-group pair only
        if (kind != KERNEL_GROUP) return hipErrorInvalidValue;
        return with_lanes_per_row(g.lanes_per_row, [&](auto l) {
            constexpr int L = decltype(l)::value;
            if (pooled) {
                if (itype == EMB_IDX_U32)
                    hipLaunchKernelGGL((bag_strided_e2m1pool_group_kernel<uint32_t, L, Mx4GroupCfg>), grid, dim3(Mx4GroupCfg::kBlock), 0, stream, d_descs, chunks_arg, d_xmap);
                else
                    hipLaunchKernelGGL((bag_strided_e2m1pool_group_kernel<int64_t, L, Mx4GroupCfg>), grid, dim3(Mx4GroupCfg::kBlock), 0, stream, d_descs, chunks_arg, d_xmap);
            } else if (itype == EMB_IDX_U32)
                hipLaunchKernelGGL((bag_strided_e2m1sum_group_kernel<uint32_t, L, Mx4GroupCfg>), grid, dim3(Mx4GroupCfg::kBlock), 0, stream, d_descs, chunks_arg, d_xmap);
            else
                hipLaunchKernelGGL((bag_strided_e2m1sum_group_kernel<int64_t, L, Mx4GroupCfg>), grid, dim3(Mx4GroupCfg::kBlock), 0, stream, d_descs, chunks_arg, d_xmap);
        });
    }
    // (with_types<false>: no fixed-point twin.)  Pooled: ONE set for every dtype, bag_strided_pool_*.
    return with_types<false>(itype, dtype, [&](auto idx, auto dt) {
        using IdxT = decltype(idx);
        constexpr int DT = decltype(dt)::value;
        return with_lanes_per_row(g.lanes_per_row, [&](auto l) {
            constexpr int L = decltype(l)::value;
            if (!pooled) {
                launch_strided_sum<IdxT, DT, L>(d_descs, grid, chunks_arg, kind, d_xmap, stream);
                return;
            }
            using One = typename PoolWaveCfgOf<DT>::One;
            if (kind == KERNEL_WAVEBATCH)
                hipLaunchKernelGGL((bag_strided_pool_wavebatch_kernel<IdxT, DT, L, One>), grid, dim3(One::kBlock), 0, stream, d_descs, chunks_arg, d_xmap);
            else
                hipLaunchKernelGGL((bag_strided_pool_group_kernel<IdxT, DT, L, GroupCfg>), grid, dim3(GroupCfg::kBlock), 0, stream, d_descs, chunks_arg, d_xmap);
        });
    });
}

}  // namespace pimemb
