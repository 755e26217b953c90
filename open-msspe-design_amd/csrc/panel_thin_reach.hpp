// panel_thin_reach.hpp -- a primer panel thinned on target reach (include/msspe_hip.h msspe_panel_thin_reach*; DESIGN.md
// 4.20): from the stable keys of a scored pass to every primer's reached columns as disjoint intervals, the greedy set
// cover over columns, and the kept primers' site planes for the reach report.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/msspe_hip.h"

namespace msspe {

class PanelThinReach {
public:
    PanelThinReach() = default;
    PanelThinReach(const PanelThinReach &) = delete;
    PanelThinReach &operator=(const PanelThinReach &) = delete;
    ~PanelThinReach() { release(); }
    void release();

    // Zeroes the figures of the last call (a call that returns before run() reports none).
    void reset();

    // d_keys: m stable keys pos << 32 | strand << 31 | primer (device, m < 2^31); d_starts: n_records record starts
    // (device); d_cover: a plane of ceil(total_len / 64) words (device) that run() clears and leaves holding the
    // columns ALL primers reach; d_plus / d_minus (both or neither): site planes cleared by the caller, which take the
    // kept primers' sites.  keep_out arrives holding the forced flags.  Returns with the stream idle and every host
    // output written; total_len < 2^32.
    int run(const uint64_t *d_keys, uint32_t m, int n, size_t total_len, int k, uint64_t reach,
            const uint64_t *d_starts, int n_records, uint64_t *d_cover, uint64_t *d_plus, uint64_t *d_minus,
            uint32_t min_gain, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
            uint32_t *reach_out, long long *reached_all_out, long long *reached_kept_out, hipStream_t stream,
            std::string &err);

    // Behind the reach report of the kept planes: closes the last phase's clock (the stream is idle).
    int end_report(hipStream_t stream, std::string &err);

    long long sites() const { return sites_; }
    long long intervals() const { return intervals_; }
    long long rounds() const { return rounds_; }
    const long long *phase_us() const { return phase_us_; }   // prepare, first gains, rounds, report

private:
    enum { kSortIn, kSortOut, kHiIn, kHiOut, kExcl, kLo, kWithin, kTiles, kPrim, kIvLo, kIvHi, kFirst, kGain, kReach,
           kLive, kFlag, kOrder, kState, kTemp, kSlots };
    int ensure(int slot, size_t bytes, std::string &err);
    void *buf_[kSlots] = {};
    size_t cap_[kSlots] = {};
    hipEvent_t ev_[5] = {};
    bool reported_ = false;   // ev_[3] was recorded by run(): end_report() has a phase to close
    long long sites_ = 0, intervals_ = 0, rounds_ = 0;
    long long phase_us_[4] = {};
};

}  // namespace msspe
