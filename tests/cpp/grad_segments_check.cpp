// grad_segments_check.cpp -- the slot numbering of the segmented order's partial sums (csrc/pimemb_grad_segments.h, the text the
// kernels compile) on the HOST.
//   grad_segments_check
// Enumerates layouts of runs over the sorted places -- every composition of n <= 18 places for S = 2 and S = 4 (the claim holds for
// any power of two), and for S = 8, 16 and 32 every sequence of up to six runs with lengths on both sides of S, 2S and 3S -- and
// asserts for each that the segments of the runs longer than S get slots that are unique and below seg_slots(n, S) = 2 * ceil(n / S).
// Prints the number of layouts and of segments it checked; tests/test_grad_segmented_cpu.py runs it.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "pimemb_grad_segments.h"

using namespace pimemb_grad;

static uint64_t g_layouts = 0, g_segments = 0;

// One layout: runs[k] places each, laid end to end.  Returns false on a collision or a slot out of range.
static bool check_layout(const std::vector<uint32_t> &runs, uint32_t S) {
    uint32_t n = 0;
    for (uint32_t L : runs) n += L;
    const uint32_t S_log2 = seg_log2(S);
    const uint64_t slots = seg_slots(n, S);
    if (slots != 2ull * ((n + S - 1) / S)) return false;
    std::vector<char> used(slots, 0);
    uint32_t head = 0;
    for (uint32_t L : runs) {
        if (L > S) {                                    // a long run: its segments start at head, head + S, ...
            for (uint32_t start = head; start < head + L; start += S) {
                const uint32_t slot = seg_slot(start, S_log2, start == head);
                if (slot >= slots || used[slot]) {
                    fprintf(stderr, "S %u n %u: run at %u of %u, segment at %u: slot %u of %llu %s\n", S, n, head, L, start, slot,
                            (unsigned long long)slots, slot >= slots ? "is out of range" : "is taken");
                    return false;
                }
                used[slot] = 1;
                g_segments++;
            }
        }
        head += L;
    }
    g_layouts++;
    return true;
}

static bool compositions(std::vector<uint32_t> &runs, uint32_t left, uint32_t S) {
    if (left == 0) return check_layout(runs, S);
    for (uint32_t L = 1; L <= left; L++) {
        runs.push_back(L);
        const bool ok = compositions(runs, left - L, S);
        runs.pop_back();
        if (!ok) return false;
    }
    return true;
}

static bool sequences(std::vector<uint32_t> &runs, const std::vector<uint32_t> &parts, uint32_t depth, uint32_t S) {
    if (!runs.empty() && !check_layout(runs, S)) return false;
    if (depth == 0) return true;
    for (uint32_t L : parts) {
        runs.push_back(L);
        const bool ok = sequences(runs, parts, depth - 1, S);
        runs.pop_back();
        if (!ok) return false;
    }
    return true;
}

int main() {
    std::vector<uint32_t> runs;
    for (uint32_t S : {2u, 4u})
        for (uint32_t n = 1; n <= 18; n++)
            if (!compositions(runs, n, S)) return 1;
    for (uint32_t S : {8u, 16u, 32u}) {
        if (!seg_length_ok(S)) return 2;
        const std::vector<uint32_t> parts = {1, 3, S - 1, S, S + 1, S + 3, 2 * S, 2 * S + 1, 2 * S + 3, 3 * S + 5};
        if (!sequences(runs, parts, 6, S)) return 1;
    }
    // the lengths the ABI takes, and the size of the buffer
    for (uint32_t S = 0; S <= 2048; S++) {
        const bool want = S == 8 || S == 16 || S == 32 || S == 64 || S == 128 || S == 256 || S == 512 || S == 1024;
        if (seg_length_ok(S) != want) return 2;
        if (want && (1u << seg_log2(S)) != S) return 2;
    }
    if (seg_pieces(1) != 1 || seg_pieces(4) != 1 || seg_pieces(5) != 2 || seg_pieces(512) != 128 || seg_pieces(513) != 128 || seg_pieces(0xffffffffu) != 128) return 3;
    if (seg_buffer_bytes(4097, 8, 320) != 2ull * 513 * 80 * 16) return 3;
    if (seg_buffer_bytes(1ull << 30, 8, 512) != (1ull << 28) * 128 * 16) return 3;
    printf("ok %llu layouts %llu segments\n", (unsigned long long)g_layouts, (unsigned long long)g_segments);
    return 0;
}
