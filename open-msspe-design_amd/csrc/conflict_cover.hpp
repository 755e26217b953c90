// conflict_cover.hpp -- the greedy minimum vertex cover of the conflict graph on the device
// (replaces the host loop of od-msspe/src/main.rs:754-798).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

namespace msspe {

// Largest pool the cover takes: its symmetrised bitmap is n^2 / 8 bytes (8 GB here).
constexpr int kCoverMaxN = 262144;

class CoverStage {
public:
    // d_pool: n packed oligos of k bases (distinct); d_bitmap: n x ceil(n/64) words, bit j of row i = (i, j) conflicts
    // (read only).  d_deleted[n] (device bytes): 1 = removed by the cover.  Returns an msspe_status; err says why.
    int run(const uint64_t *d_pool, int n, int k, const uint64_t *d_bitmap, bool drop_self_pairs, uint8_t *d_deleted,
            int *n_deleted, int n_cu, hipStream_t stream, std::string &err);
    void release();
    // The phases the tube split shares (csrc/tube_split.hip): begin() sizes the buffers for n oligos and starts the
    // clock; prepare() ranks the oligos, refuses duplicates and bits above 2 k (MSSPE_ERR_ARG), and leaves S = B | B^T
    // (self pairs dropped on request) in symmetrised() and the lexicographic ranks in ranks().  It synchronises the
    // stream once, for the key check.  prepare_us(): device time of the two phases, once the stream has drained.
    int begin(int n, int k, hipStream_t stream, std::string &err);
    int prepare(const uint64_t *d_pool, int n, int k, const uint64_t *d_bitmap, bool drop_self_pairs,
                hipStream_t stream, std::string &err);
    void prepare_us(long long &keys_us, long long &symmetrise_us) const;
    const uint64_t *symmetrised() const { return (const uint64_t *)buf_[0]; }
    const uint32_t *ranks() const { return (const uint32_t *)buf_[6]; }
    // buffers of the rounds, free between two calls: 8 n bytes of keys, two lists of n nodes, n counters
    uint64_t *round_keys() const { return (uint64_t *)buf_[7]; }
    uint32_t *round_lists() const { return (uint32_t *)buf_[8]; }
    uint32_t *round_counters() const { return (uint32_t *)buf_[10]; }
    // the last run: rounds that deleted nodes, and device time of its phases in microseconds (sort and keys,
    // symmetrise, rounds)
    long long rounds() const { return rounds_; }
    const long long *phase_us() const { return phase_us_; }

private:
    void *buf_[11] = {};
    size_t cap_[11] = {};
    hipEvent_t ev_[5] = {};
    size_t sort_tmp_ = 0;
    long long rounds_ = 0;
    long long phase_us_[3] = {};
    int ensure(int slot, size_t bytes, std::string &err);
};

}  // namespace msspe
