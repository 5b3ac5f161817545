// pimemb_grad_segments.h -- where the partial sums of EMB_GRAD_ORDER_SEGMENTED live (include/pimemb_grad.h): the numbering of the
// segments of long runs, and the size of the buffer that holds their sums.
//
// After the sort a run of k equal keys lies at the sorted places head .. head + k - 1 in position order.  With segment length S
// (a power of two) its segments start at head, head + S, head + 2S, ...; only runs LONGER than S -- long runs -- keep partial sums.
// Take any S-aligned block of sorted places [bS, bS + S).  A long run has at most one segment start in it (its starts lie S
// apart), and at most two long runs reach into it with a start: a second one can only BEGIN in the block, a third would need the
// second to end inside the block it began in, and that one is longer than the block.  So where two starts share a block, the first
// is no run head and the second is one, and
//     slot(start) = 2 * (start / S) + (start is the head of its run ? 1 : 0)
// gives every segment of every long run a slot of its own below 2 * ceil(n / S) -- from the start's place alone, with no scan.
// A slot holds `pieces` 16-byte pieces: one float4 per four elements of a row of the call's table.
// `__host__ __device__` like pimemb_grad_step.h: the kernels of pimemb_grad.hip and the host-side check
// (tests/cpp/grad_segments_check.cpp, which enumerates run layouts) compile the same text.
#pragma once

#include <stdint.h>

#include "pimemb_rows_encode.h"

namespace pimemb_grad {

constexpr uint32_t kSegMin = 8, kSegMax = 1024;       // S: a power of two in this range
constexpr uint32_t kSegLaneDim = 512;                 // the widest row the lane-group kernels take: wider tables need no buffer

PIMEMB_ROWS_HD bool seg_length_ok(uint32_t S) { return S >= kSegMin && S <= kSegMax && (S & (S - 1)) == 0; }

PIMEMB_ROWS_HD uint32_t seg_log2(uint32_t S) {
    uint32_t l = 0;
    while ((1u << l) < S) l++;
    return l;
}

// The slot of the segment that starts at sorted place `start`.
PIMEMB_ROWS_HD uint32_t seg_slot(uint32_t start, uint32_t S_log2, bool is_head) { return 2u * (start >> S_log2) + (is_head ? 1u : 0u); }

// Slots a batch of n positions can use.
PIMEMB_ROWS_HD uint64_t seg_slots(uint64_t n, uint32_t S) { return 2u * ((n + S - 1) / S); }

// 16-byte pieces of one slot for tables of up to max_dim elements a row.
PIMEMB_ROWS_HD uint32_t seg_pieces(uint32_t max_dim) { return ((max_dim < kSegLaneDim ? max_dim : kSegLaneDim) + 3u) / 4u; }

// Bytes of the partial-sum buffer of a context of max_indices positions.
PIMEMB_ROWS_HD uint64_t seg_buffer_bytes(uint64_t max_indices, uint32_t S, uint32_t max_dim) {
    return seg_slots(max_indices, S) * seg_pieces(max_dim) * 16u;
}

}  // namespace pimemb_grad
