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
    // The panel thinning's first pass (panel_thin.hip): the same comparisons, and instead of the counts the matrix
    // d_inc[g * n_pad + p] (device; n_pad = n_fwd + n_rev rounded up to 64) -- bit b says primer p (forward primers
    // first) has a match in segment g * group_size(opt) + b.  Every word with p < n_fwd + n_rev is written once.
    // Needs segments (check() first); returns with the stream idle.
    int incidence(const SeqView &seqs, int n_seq, size_t seq_len, const msspe_kmer_opt &opt, int max_mismatches,
                  int exact_3p, const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                  uint64_t *d_inc, hipStream_t stream, std::string &err);
    // the argument rules of run(); *P_out: partitions per record (0: no segments)
    static int check(int n_seq, size_t seq_len, const msspe_kmer_opt &opt, int max_mismatches, int exact_3p,
                     const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev, long *P_out,
                     std::string &err);
    static int group_size(const msspe_kmer_opt &opt);   // segments per block (<= 64): one bit each in a matrix word
    void release();

private:
    void *buf_[3] = {};
    size_t cap_[3] = {};
    int ensure(int slot, size_t bytes, std::string &err);
    int run(const SeqView &seqs, int n_seq, size_t seq_len, const msspe_kmer_opt &opt, int max_mismatches,
            int exact_3p, const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
            uint8_t *best_out, uint32_t *primer_segments_out, uint64_t *d_inc, hipStream_t stream, std::string &err);
};

}  // namespace msspe
