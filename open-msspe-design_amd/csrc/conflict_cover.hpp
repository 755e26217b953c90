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
    // the last run: rounds that deleted nodes, and device time of its phases in microseconds (sort and keys,
    // symmetrise, rounds)
    long long rounds() const { return rounds_; }
    const long long *phase_us() const { return phase_us_; }

private:
    void *buf_[11] = {};
    size_t cap_[11] = {};
    hipEvent_t ev_[5] = {};
    long long rounds_ = 0;
    long long phase_us_[3] = {};
    int ensure(int slot, size_t bytes, std::string &err);
};

}  // namespace msspe
