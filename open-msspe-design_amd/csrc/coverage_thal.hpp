// coverage_thal.hpp -- segment coverage scored with thal (engine extension: include/msspe_hip.h
// msspe_segment_coverage_thal*): the matches of msspe_segment_coverage_mm* as a list, their template oligos, and the
// fold of their scores into per-segment and per-primer results.  The scoring between the two is the background
// screen's (capi.cpp score_site_pairs), over the same work list (msspe_ctx::site_work).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/msspe_hip.h"
#include "kmer_stage.hpp"

namespace msspe {

// One match in the work list: the size of an msspe_site, whose buffer it shares.
struct CovMatch {
    uint32_t primer;    // 0 .. n_fwd + n_rev - 1, forward primers first
    uint32_t segment;   // r * P + j
    uint32_t off_mm;    // window position p | mismatches << kCovOffBits
};
constexpr int kCovOffBits = 26;   // W - k < 2^26 (checked); mismatches <= 31 fit above
static_assert(sizeof(CovMatch) == sizeof(msspe_site), "the match list lives in the site work list");

class CoverageThal {
public:
    // The primer words as planes on the device; held, t_best and the two per-primer counters zeroed for n_seg
    // segments and n primers.  The caller has checked that W - k < 2^kCovOffBits.
    int prepare(const msspe_kmer_opt &opt, const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                long n_seg, hipStream_t stream, std::string &err);
    // The first half of prepare alone -- the primer words as planes, the events -- for a caller that needs list_slab
    // and oligos but none of the per-segment or per-primer results (msspe_panel_thin_thal*).
    int prepare_words(const msspe_kmer_opt &opt, const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words,
                      int n_rev, hipStream_t stream, std::string &err);
    // Groups [g0, g1) (MismatchCoverage::group_size segments each) against primers [p0, p1): every match is appended
    // at list[(*d_count)++] while that is below cap; the counter (zeroed by the caller) runs on past it.
    int list_slab(const SeqView &seqs, long n_seg, long P, const msspe_kmer_opt &opt, int max_mismatches, int exact_3p,
                  long g0, long g1, int p0, int p1, CovMatch *list, uint64_t cap, uint64_t *d_count,
                  hipStream_t stream, std::string &err);
    // Matches [first, first + count) of list: the template oligo -- the strand the primer anneals to, 5'->3',
    // msspe_pack_oligos form -- of match idx goes to pool[n + idx], the pair (primer, n + idx) to
    // pairs[idx - first]; *list_count = count.
    hipError_t oligos(const SeqView &seqs, long P, const msspe_kmer_opt &opt, const CovMatch *list, uint32_t first,
                      uint32_t count, uint64_t *pool, uint2 *pairs, uint32_t *list_count, hipStream_t stream);
    // The scored matches [0, count) of a slab that list_slab made for (g0, g1, p0, p1): held and t_best per segment,
    // the slab's (group, primer) cells marked and counted into the per-primer counters, and with d_count one
    // msspe_scored_match per match appended to d_out (at most capacity are stored, *d_count runs on).
    int fold_slab(const CovMatch *list, uint32_t count, const double *dg, const double *t, double t_cut,
                  const msspe_kmer_opt &opt, long g0, long g1, int p0, int p1, msspe_scored_match *d_out,
                  uint64_t capacity, uint64_t *d_count, hipStream_t stream, std::string &err);
    // The results to the host (held_out required, the others optional); returns with the stream idle.
    int finish(long n_seg, uint8_t *held_out, double *t_best_out, uint32_t *primer_segments_out,
               uint32_t *primer_held_out, hipStream_t stream, std::string &err);
    // The caller's list on the device: room for `capacity` records and, behind them, the count (zeroed here).
    int out_list(uint64_t capacity, msspe_scored_match **d_out, uint64_t **d_count, hipStream_t stream,
                 std::string &err);
    // groups a first slab may hold so that its cell bitmaps stay within the budget
    static long max_slab_groups(int n_primers);
    void release();

    long long matches = 0, slabs = 0, redone = 0;        // of the last call (msspe_get_info "coverage_thal_*")
    long long list_us = 0, score_us = 0, fold_us = 0;
    hipEvent_t ev[5] = {};   // before / after the listing; before the oligos, after the scores, after the fold

private:
    enum { kWords, kHeld, kBest, kCells, kCounts, kOut, kSlots };
    void *buf_[kSlots] = {};
    size_t cap_[kSlots] = {};
    int n_fwd_ = 0, n_rev_ = 0;
    int ensure(int slot, size_t bytes, hipStream_t stream, std::string &err);
};

}  // namespace msspe
