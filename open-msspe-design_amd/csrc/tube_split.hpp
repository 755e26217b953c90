// tube_split.hpp -- the conflict graph split into reaction tubes on the device: a largest-degree-first greedy colouring
// with at most max_tubes colours (engine extension, no reference counterpart).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "conflict_cover.hpp"

namespace msspe {

constexpr int kTubeMax = 64;   // one 64-bit mask per node holds its forbidden tubes

class TubeStage {
public:
    // d_pool, d_bitmap, drop_self_pairs as CoverStage::run (the graph is the cover's, built by the cover's phases in
    // the cover's buffers).  d_tube[n] (device bytes): the tube of each oligo in [0, max_tubes), or MSSPE_TUBE_NONE.
    // Returns an msspe_status; err says why.
    int run(CoverStage &cover, const uint64_t *d_pool, int n, int k, const uint64_t *d_bitmap, bool drop_self_pairs,
            int max_tubes, uint8_t *d_tube, int *n_tubes_used, int *n_unplaced, int n_cu, hipStream_t stream,
            std::string &err);
    void release();
    // the last run: rounds that decided nodes, and device time of its phases in microseconds (sort and keys,
    // symmetrise, rounds)
    long long rounds() const { return rounds_; }
    const long long *phase_us() const { return phase_us_; }

private:
    void *state_ = nullptr;
    hipEvent_t ev_[2] = {};
    long long rounds_ = 0;
    long long phase_us_[3] = {};
};

}  // namespace msspe
