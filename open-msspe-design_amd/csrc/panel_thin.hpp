// panel_thin.hpp -- a primer panel thinned to the primers its coverage needs: a greedy set cover over the incidence
// "primer p has a match in segment s" of the mismatch-tolerant coverage (engine extension, no reference counterpart;
// DESIGN.md 4.10).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "coverage_mm.hpp"

namespace msspe {

class PanelThin {
public:
    // The alignment, options and primer words of MismatchCoverage::run; forced (host, optional, n_fwd + n_rev): primers
    // kept whatever they cover, never picked.  Rounds: the unpicked, unforced primer with the most uncovered segments
    // (ties: the lowest index), until that gain is below min_gain.  keep_out[n]: forced or picked; order_out /
    // gain_out[n]: the picks in order with their gains; covered_out (optional, n_seq * P bytes): segments the kept
    // set covers.  max_matrix_bytes bounds the incidence matrix (MSSPE_ERR_CAPACITY above it).  Returns an
    // msspe_status; err says why.
    int run(MismatchCoverage &cov, const SeqView &seqs, int n_seq, size_t seq_len, const msspe_kmer_opt &opt,
            int max_mismatches, int exact_3p, int min_gain, const uint64_t *fwd_words, int n_fwd,
            const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out,
            uint32_t *gain_out, int *n_picked_out, uint8_t *covered_out, long long *covered_all_out,
            long long *covered_kept_out, size_t max_matrix_bytes, int n_cu, hipStream_t stream, std::string &err);
    // run() in its two halves, for a caller that fills the matrix itself (msspe_panel_thin_thal*: the held incidence).
    // matrix: the buffers of a run over n primers and n_seg segments in groups of S, under the same cap; *inc_out is
    // the matrix (inc[g * n_pad + p], n_pad = n rounded up to 64, bit b = segment g * S + b), not yet written.  The
    // caller writes every word of it on `stream`, then calls rounds: forced rows (keep_out holds the forced flags on
    // entry), first gains, the round batches and the read-back, with run's outputs.  Returns with the stream idle.
    int matrix(int n, long n_seg, int S, size_t max_matrix_bytes, uint64_t **inc_out, std::string &err);
    int rounds(int n, long n_seg, int S, int min_gain, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
               int *n_picked_out, uint8_t *covered_out, long long *covered_all_out, long long *covered_kept_out,
               int n_cu, hipStream_t stream, std::string &err);
    void release();
    // the last run: rounds enqueued that ran (the picks and the one that stopped), segment groups (matrix rows), and
    // device time in microseconds of the incidence pass, the first gains and the rounds
    long long rounds() const { return rounds_; }
    long long groups() const { return groups_; }
    const long long *phase_us() const { return phase_us_; }

private:
    enum { kSlots = 8 };
    void *buf_[kSlots] = {};
    size_t cap_[kSlots] = {};
    hipEvent_t ev_[4] = {};
    long long rounds_ = 0, groups_ = 0;
    long long phase_us_[3] = {};
    int ensure(int slot, size_t bytes, std::string &err);
};

}  // namespace msspe
