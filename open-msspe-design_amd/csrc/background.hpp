// background.hpp -- off-target sites of a primer set in a background stream, both strands, within N mismatches with
// the primer's 3' end exact (engine extension, no reference counterpart: include/msspe_hip.h msspe_background_sites*).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/msspe_hip.h"

namespace msspe {

// ASCII columns [0, n_cols) of a stream chunk that starts at a stream column divisible by 64 -> the chunk's words of
// the packed stream: n_cols / 32 (rounded up) base words at `bases`, n_cols / 64 (rounded up) validity words at `valid`.
// Bits past n_cols are written as zero.
hipError_t launch_pack_stream(const uint8_t *d_ascii, size_t n_cols, uint64_t *bases, uint64_t *valid,
                              hipStream_t stream);

class BackgroundSites {
public:
    // d_packed: one packed row of total_len columns (msspe_device_put_stream_packed); words: host, msspe_pack_oligos
    // form; sites_out (host, 2 n): sites per primer and strand; d_sites / capacity / d_count: the optional device
    // site list (d_sites == nullptr: not made).  Returns an msspe_status; err says why.
    int run(const uint64_t *d_packed, size_t total_len, int k, int max_mismatches, int exact_3p,
            const uint64_t *words, int n, uint64_t *sites_out, msspe_site *d_sites, uint64_t capacity,
            uint64_t *d_count, int n_cu, hipStream_t stream, std::string &err);
    void release();

    // The pieces msspe_background_thal* drives itself.  check: run()'s argument statuses.  prepare: the n primer
    // words in plane form on the device (kept until the next prepare or run).  list_slab: the site list -- no
    // counts -- of primers [p0, p1) over the runs [run0, run1) of the stream, n_runs() runs of 2048 positions in all;
    // *d_count (zeroed by the caller) runs past the capacity, which is how a slab that did not fit is seen.  One
    // run against one primer has at most kMaxSitesPerRunPrimer sites.
    static constexpr uint32_t kMaxSitesPerRunPrimer = 4096;
    static uint32_t n_runs(size_t total_len, int k);
    static int check(size_t total_len, int k, int max_mismatches, int exact_3p, const uint64_t *words, int n,
                     std::string &err);
    int prepare(int k, const uint64_t *words, int n, hipStream_t stream, std::string &err);
    int list_slab(const uint64_t *d_packed, size_t total_len, int k, int max_mismatches, int exact_3p, int p0, int p1,
                  uint32_t run0, uint32_t run1, msspe_site *d_sites, uint64_t capacity, uint64_t *d_count, int n_cu,
                  hipStream_t stream, std::string &err);

private:
    void *buf_[2] = {};      // [0] primer words in plane form, [1] 2 n 64-bit counts
    size_t cap_[2] = {};
    std::vector<uint32_t> w32_;   // host copies of the plane words (kept: the upload is asynchronous)
    std::vector<uint2> w64_;
    int ensure(int slot, size_t bytes, std::string &err);
};

}  // namespace msspe
