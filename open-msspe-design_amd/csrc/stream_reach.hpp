// stream_reach.hpp -- from the stable-site bit planes to per-record reach (include/msspe_hip.h msspe_stream_reach*):
// tile summaries and their scans, the reach masks with the per-strand counts and gaps, the either-strand gaps.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/msspe_hip.h"

namespace msspe {

// One lane per 64-column word, one wave per tile: the carry works in tiles of this many columns.
constexpr int kReachTileWords = 64;
constexpr int kReachTileColumns = 64 * kReachTileWords;

// What the kernels keep per record: the six counts, then one key len << 32 | ~pos per gap (0: no run closed).
struct ReachAccum {
    uint32_t sites_plus, sites_minus, reached_plus, reached_minus, reached_either, reached_both;
    unsigned long long gap_plus, gap_minus, gap_either;
};

inline size_t reach_plane_words(size_t total_len) { return (total_len + 63) / 64; }
inline size_t reach_tiles(size_t total_len)
{
    return (reach_plane_words(total_len) + kReachTileWords - 1) / kReachTileWords;
}

// (a) per tile: the last set bit of the plus plane (position + 1, 0 without one) and the first set bit of the minus
// END plane -- the minus plane moved up by k - 1, a minus site at q reaches down from its last column q + k - 1 --
// (position, 0xffffffff without one); then the exclusive running maximum from the left / minimum from the right, in
// place, one block.
hipError_t launch_reach_tiles(const uint64_t *d_plus, const uint64_t *d_minus, size_t total_len, int k,
                              uint32_t *d_tile_plus, uint32_t *d_tile_minus, hipStream_t stream);
hipError_t launch_reach_scan(uint32_t *d_tile_max, uint32_t *d_tile_min, size_t n_tiles, hipStream_t stream);

// (b) per word: the plus-reached and minus-reached masks cut at the record boundaries, the four column counts, the two
// site counts and the per-strand gaps of every record into d_acc (zeroed by the caller), and the plane "in a record and
// reached on neither strand" into d_neither.  d_starts: n_records record starts, d_starts[0] == 0; record r ends
// before the separator at d_starts[r + 1] - 1, the last record at total_len.
hipError_t launch_reach_masks(const uint64_t *d_plus, const uint64_t *d_minus, size_t total_len, int k, uint64_t reach,
                              const uint64_t *d_starts, int n_records, const uint32_t *d_tile_plus,
                              const uint32_t *d_tile_minus, ReachAccum *d_acc, uint64_t *d_neither,
                              hipStream_t stream);

// (c) the same carry on d_neither: per tile the last ZERO bit (position + 1), scanned with launch_reach_scan(max only),
// then every maximal run of ones -- it lies in one record, a separator is never in the plane -- folds its length and
// start into gap_either of its record.
hipError_t launch_reach_gap_tiles(const uint64_t *d_neither, size_t total_len, uint32_t *d_tile_zero,
                                  hipStream_t stream);
hipError_t launch_reach_gaps(const uint64_t *d_neither, size_t total_len, const uint64_t *d_starts, int n_records,
                             const uint32_t *d_tile_zero, ReachAccum *d_acc, hipStream_t stream);

}  // namespace msspe
