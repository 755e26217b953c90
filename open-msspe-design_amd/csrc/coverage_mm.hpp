// coverage_mm.hpp -- segment coverage of a primer set within N mismatches, the primer's 3' end exact (engine
// extension: generalises the exact rule of od-msspe/src/main.rs:518-594, which KmerStage::coverage restates).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "kmer_stage.hpp"

namespace msspe {

class MismatchCoverage {
public:
    // fwd_words / rev_words: host, packed as msspe_pack_oligos packs them (a reverse word in primer orientation).
    // best_out[seq * P + partition] (host): the smallest mismatch count of a match in the segment, 255 when none;
    // primer_segments_out (host, optional, n_fwd + n_rev): segments whose head (forward) / tail (reverse) window
    // holds a match of the primer.  Returns an msspe_status; err says why.
    int run(const SeqView &seqs, int n_seq, size_t seq_len, const msspe_kmer_opt &opt, int max_mismatches,
            int exact_3p, const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
            uint8_t *best_out, uint32_t *primer_segments_out, hipStream_t stream, std::string &err);
    void release();

private:
    void *buf_[3] = {};
    size_t cap_[3] = {};
    int ensure(int slot, size_t bytes, std::string &err);
};

}  // namespace msspe
