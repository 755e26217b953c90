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

// What a weighted call (msspe_panel_thin_weighted*, msspe_panel_select_weighted*) hands to
// PanelThin::rounds / PanelSelect::rounds: the weights (host, one per segment in the order of covered_out; the caller
// has checked that their total fits a uint32) and the two optional sums, the weight of the segments that all primers
// cover and that the kept set covers.  With it a gain is a sum of weights and min_gain is in weight units.
struct PanelWeights {
    const uint32_t *weights;
    uint64_t *weight_all_out, *weight_kept_out;
};

// What a cost call (msspe_panel_thin_cost*, msspe_panel_select_cost*) hands to PanelThin::rounds /
// PanelSelect::rounds: a cost per primer (host, n_fwd + n_rev entries in the order of keep_out, every one at least 1:
// the caller has checked) and the two optional sums, over all primers and over the kept ones.  With it a round picks
// the greatest gain / cost, compared exactly, among the live primers whose gain reaches min_gain; the gains themselves
// are the sibling's, weights or counts.
struct PanelCosts {
    const uint32_t *costs;
    uint64_t *cost_all_out, *cost_kept_out;
};

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
            long long *covered_kept_out, size_t max_matrix_bytes, int n_cu, hipStream_t stream, std::string &err,
            const PanelWeights *wts = nullptr, const PanelCosts *cst = nullptr);
    // run() in its two halves, for a caller that fills the matrix itself (msspe_panel_thin_thal*: the held incidence).
    // matrix: the buffers of a run over n primers and n_seg segments in groups of S, under the same cap; *inc_out is
    // the matrix (inc[g * n_pad + p], n_pad = n rounded up to 64, bit b = segment g * S + b), not yet written.  The
    // caller writes every word of it on `stream`, then calls rounds: forced rows (keep_out holds the forced flags on
    // entry), first gains, the round batches and the read-back, with run's outputs.  Returns with the stream idle.
    int matrix(int n, long n_seg, int S, size_t max_matrix_bytes, uint64_t **inc_out, std::string &err);
    int rounds(int n, long n_seg, int S, int min_gain, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
               int *n_picked_out, uint8_t *covered_out, long long *covered_all_out, long long *covered_kept_out,
               int n_cu, hipStream_t stream, std::string &err, const PanelWeights *wts = nullptr,
               const PanelCosts *cst = nullptr);
    // Depth (msspe_panel_thin_depth*): every segment keeps min(depth, primers it has) primers.  run's
    // arguments plus depth (1..255, checked by the caller); depth_all_out / depth_kept_out (optional, n_seq * P bytes):
    // representatives per segment among all and among the kept, saturating at 255; counts_out[4] (optional): segments
    // with depth_all >= 1, depth_kept >= 1, depth_all >= depth, depth_kept >= depth.  rounds_depth is rounds' sibling
    // for a caller that fills the matrix itself; shadow (host, n flags): primers that count in nothing and are never
    // picked.  shadows() marks them: among primers of one direction with the same word, all but the forced one of
    // lowest index (without a forced one, the lowest index); returns how many.
    int run_depth(MismatchCoverage &cov, const SeqView &seqs, int n_seq, size_t seq_len, const msspe_kmer_opt &opt,
                  int max_mismatches, int exact_3p, int min_gain, int depth, const uint64_t *fwd_words, int n_fwd,
                  const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out,
                  uint32_t *gain_out, int *n_picked_out, uint8_t *depth_all_out, uint8_t *depth_kept_out,
                  long long *counts_out, size_t max_matrix_bytes, int n_cu, hipStream_t stream, std::string &err);
    int rounds_depth(int n, long n_seg, int S, int min_gain, int depth, const uint8_t *shadow, uint8_t *keep_out,
                     uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *depth_all_out,
                     uint8_t *depth_kept_out, long long *counts_out, int n_cu, hipStream_t stream, std::string &err);
    static int shadows(const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                       const uint8_t *forced, uint8_t *shadow_out);
    // The column sums alone, enqueued on `stream` (k_thin_colsum, for PanelSelect::rounds_depth): out[g * 64 + b] =
    // min(255, primers p with mask[p] set and bit b in inc[g * n_pad + p]) over G groups, G * 64 bytes; c1 / cR
    // (device, optional, both or neither): += the segments with a count of at least 1 / of at least R.
    static void colsum(const uint64_t *inc, int n, long G, const uint8_t *mask, uint32_t R, uint8_t *out,
                       unsigned long long *c1, unsigned long long *cR, int n_cu, hipStream_t stream);
    void release();
    // the last depth run: shadows among its primers, device time of the three column-sum passes and the init
    long long depth_shadows() const { return shadows_; }
    long long depth_colsum_us() const { return colsum_us_; }
    // the last run: rounds enqueued that ran (the picks and the one that stopped), segment groups (matrix rows), and
    // device time in microseconds of the incidence pass, the first gains and the rounds
    long long rounds() const { return rounds_; }
    long long groups() const { return groups_; }
    const long long *phase_us() const { return phase_us_; }

private:
    enum { kSlots = 12 };
    void *buf_[kSlots] = {};
    size_t cap_[kSlots] = {};
    hipEvent_t ev_[4] = {};
    hipEvent_t ev_depth_[2] = {};   // after the first column sums and the init; after the kept column sums
    long long rounds_ = 0, groups_ = 0, shadows_ = 0, colsum_us_ = 0;
    long long phase_us_[3] = {};
    int ensure(int slot, size_t bytes, std::string &err);
};

}  // namespace msspe
