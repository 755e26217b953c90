// kmer_stage.hpp -- stage A on the device: k-mer candidate generation
// (replaces get_segment_manager + find_candidates_kmers,
//  /root/reference/od-msspe/src/main.rs:196-235 and :331-406).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/msspe_hip.h"

namespace msspe {

// The alignment as the kernels read it.  ascii != nullptr: n_seq x seq_len bytes, upper case, U -> T
// (od-msspe/src/main.rs:115-118).  Otherwise packed rows of row_words() uint64 each: first
// (seq_len + 31) / 32 words of 2-bit bases (A 0, C 1, G 2, T 3; column c in bits [2 (c % 32), +1] of word
// c / 32), then (seq_len + 63) / 64 words of validity bits (1 = the column holds A, C, G or T).
struct SeqView {
    const uint8_t *ascii;
    const uint64_t *packed;
    size_t seq_len;
    static size_t base_words(size_t seq_len) { return (seq_len + 31) / 32; }
    static size_t row_words(size_t seq_len) { return (seq_len + 31) / 32 + (seq_len + 63) / 64; }
};

// device ASCII rows (n_rows x row_len) -> packed rows (n_rows x SeqView::row_words(row_len))
hipError_t launch_pack_rows(const uint8_t *d_ascii, int n_rows, size_t row_len, uint64_t *d_packed,
                            hipStream_t stream);

class KmerStage {
public:
    // d_seqs: device, n_seq x seq_len bytes.  words_out / freq_out / n_out: host buffers.
    // seed / n_seed (host, optional): packed words (msspe_pack_oligos) of the direction's key space, taken as
    // already picked -- their segments covered and their partitions' coverage bumped once each before the first
    // iteration (main.rs:371-378); order and duplicates do not matter, words absent from the index do nothing
    // exclude / n_exclude (host, optional): packed words of the same key space that are treated as occurring in no
    // search window -- taken out of the extracted keys before the index is built (k_exclude), so they have no
    // postings, no count, and can be neither winners nor seeds; every other word keeps its own occurrences
    // seed_from (optional; then seed / n_seed must be empty): the run is seeded by the caller instead of k_seed.  It is
    // called once, at the point where k_seed would run -- the index built, the live counts set, ignored and coverage
    // zero, all in stream order -- and seeds the state with seed_rows (any number of times); the loop then starts as
    // a seeded run's does.  With no word in the index, or max_iterations == 0, it is still called (the state is then
    // the flags and the coverage alone) and the run returns without winners.  A nonzero return ends the run with it.
    using SeedFrom = std::function<int(KmerStage &, hipStream_t, std::string &)>;
    int run(const SeqView &seqs, int n_seq, size_t seq_len, const msspe_kmer_opt &opt,
            int direction, uint64_t *words_out, uint32_t *freq_out, int capacity, int *n_out,
            hipStream_t stream, std::string &err, const uint64_t *seed = nullptr, int n_seed = 0,
            const uint64_t *exclude = nullptr, int n_exclude = 0, const SeedFrom *seed_from = nullptr);
    // Inside seed_from.  seed_rows: the post-push update of main.rs:371-378 for rows [0, n_rows) of an incidence
    // matrix d_inc[g * n_pad + p] (device; group-major, bit b of a word = segment g * S + b, s = r * P + j; the words
    // of rows >= n_rows are not read) -- a row's segments become ignored, and coverage[j] goes up by one for every
    // distinct partition j among all of them.
    // seed_state: ignored as covered_out[r * P + j] and coverage[] as partitions_out[P] (host, either may be null),
    // and the segments seed_rows covered so far in this run; returns with the stream idle.
    int seed_rows(const uint64_t *d_inc, size_t n_pad, int n_rows, long n_groups, int S, hipStream_t stream,
                  std::string &err);
    int seed_state(uint8_t *covered_out, uint32_t *partitions_out, long long *covered_count_out, hipStream_t stream,
                   std::string &err);
    // Segment coverage of a primer set (main.rs:518-594): hit_out[seq * P + partition] = 1 when the
    // segment's head window holds a forward primer or its tail window the reverse complement of a
    // reverse primer.  fwd_words / rev_words / hit_out: host buffers.
    int coverage(const SeqView &seqs, int n_seq, size_t seq_len, const msspe_kmer_opt &opt,
                 const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                 uint8_t *hit_out, hipStream_t stream, std::string &err);
    void release();
    void set_use_graph(bool on) { use_graph_ = on; }
    // false: every iteration of the greedy loop scans all the words (the five-launch iteration)
    void set_narrow_loop(bool on) { narrow_loop_ = on; }
    // the last run's candidate-list loop: iterations that recorded winners without a posting walk / with one,
    // iterations that rebuilt the list, idle iterations at the end of the last batch
    const int *loop_stats() const { return loop_stats_; }
    // per winner of the last run: iteration << 8 | how it was selected (1 a partition's leader, 2 a several-partition
    // word, 3 the same with a re-computed key, 4 after posting walks, 0 the all-words loop)
    const std::vector<uint32_t> &trace() const { return trace_; }

private:
    void *buf_[20] = {};
    size_t cap_[20] = {};
    void *pinned_ = nullptr;   // the loop state's host copy (pinned: read back once per batch)
    bool use_graph_ = true;
    bool narrow_loop_ = true;
    int loop_stats_[4] = {};
    std::vector<uint32_t> trace_;
    // the candidate-list loop's graph (eight iterations), kept across runs for as long as its kernels' arguments are
    // what they were (same buffers, same shape: the two directions of one alignment, repeated calls); capturing and
    // instantiating it costs 0.9 ms
    hipGraph_t loop_graph_ = nullptr;
    hipGraphExec_t loop_exec_ = nullptr;
    std::vector<uint64_t> loop_sig_;
    void drop_loop_graph();
    // the run's state where the seeding happens (valid inside seed_from): per == 0 when there is no index
    struct SeedPoint {
        uint8_t *ignored;
        uint32_t *coverage;
        int32_t *count;
        const int32_t *kid_of_inst;
        int P, n_seq, per, n_seg;
    } seed_point_ = {};
    int ensure(int slot, size_t bytes, std::string &err);
};

}  // namespace msspe
