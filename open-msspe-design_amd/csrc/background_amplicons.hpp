// background_amplicons.hpp -- off-target amplicons from the stable sites of a background screen
// (include/msspe_hip.h msspe_background_amplicons*): sort of the stable keys, their record ids, the join.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/msspe_hip.h"

namespace msspe {

// A stable key is pos << 32 | strand << 31 | primer (k_site_fold_keys writes them).  rocPRIM's temporary storage for
// a sort of m keys over their low end_bit bits.
size_t amplicon_sort_temp_bytes(size_t m, unsigned end_bit);

// d_sorted[0 .. m) = d_keys[0 .. m) ascending on bits [0, end_bit) (position is the major key, then the strand, then
// the primer, so the plus-strand keys of a position come before its minus-strand keys).
hipError_t sort_amplicon_keys(const uint64_t *d_keys, uint64_t *d_sorted, size_t m, unsigned end_bit, void *d_temp,
                              size_t temp_bytes, hipStream_t stream);

// d_rec[i] = the record of sorted key i: the last r with d_starts[r] <= pos (0xffffffff before d_starts[0]).
hipError_t launch_key_records(const uint64_t *d_sorted, uint32_t m, const uint64_t *d_starts, int n_records,
                              uint32_t *d_rec, hipStream_t stream);

// The join over the sorted keys: every (plus key of primer f at p, minus key of primer r at q) with q >= p,
// min_len <= q + k - p <= max_len and equal record ids is one amplicon: counts[2 f] += 1, counts[2 r + 1] += 1, and
// with d_out one msspe_amplicon is appended (at most capacity are stored, *d_count runs on).
hipError_t launch_amplicon_join(const uint64_t *d_sorted, const uint32_t *d_rec, uint32_t m, int k, uint32_t min_len,
                                uint32_t max_len, unsigned long long *counts, msspe_amplicon *d_out,
                                uint64_t capacity, uint64_t *d_count, hipStream_t stream);

}  // namespace msspe
