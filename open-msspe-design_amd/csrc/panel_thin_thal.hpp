// panel_thin_thal.hpp -- a panel thinned on the segments it holds at a temperature (engine extension:
// include/msspe_hip.h msspe_panel_thin_thal*): between the match list of msspe_segment_coverage_thal*
// (CoverageThal::list_slab / oligos, the work list msspe_ctx::site_work) and the greedy rounds of msspe_panel_thin*
// (PanelThin::rounds), the two steps this call adds -- every distinct (primer, template) pair of a slab once, and the
// fold of the scores into the held incidence matrix.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "coverage_thal.hpp"

namespace msspe {

class PanelThinThal {
public:
    // The matches [0, count) of a listed slab whose template words are in pool[n + idx] (CoverageThal::oligos), ordered
    // by (primer, template word); pairs[u] = (primer, n + idx of the run's first match) for run u, *unique_count() =
    // the number of runs.  keys_a / keys_b: two planes of `count` 64-bit words the sort may use (the work list's dg /
    // t planes, which the scoring writes only afterwards).  k: the oligo length, n: primers.
    int unique(const CovMatch *list, const uint64_t *pool, int n, int k, uint32_t count, uint64_t *keys_a,
               uint64_t *keys_b, uint2 *pairs, hipStream_t stream, std::string &err);
    // inc[g * n_pad + primer] |= bit of the segment, for every match whose pair scored stable (max(0, t) > t_cut).
    // by_run: t is read at the first match of the match's run (unique() ran for this slab; the scoring may have
    // reordered its pair list, the run heads are kept here); otherwise at the match's own index.
    int fold(const CovMatch *list, uint32_t count, bool by_run, const double *t, double t_cut, int S, size_t n_pad,
             uint64_t *inc, hipStream_t stream, std::string &err);
    const uint32_t *unique_count() const { return (const uint32_t *)buf_[kCount]; }
    int events(std::string &err);
    void release();

    // of the last call (msspe_get_info "panel_thin_thal_*")
    long long matches = 0, unique_pairs = 0, slabs = 0, redone = 0;
    long long list_us = 0, unique_us = 0, score_us = 0, fold_us = 0;
    void reset_stats()
    {
        matches = unique_pairs = slabs = redone = 0;
        list_us = unique_us = score_us = fold_us = 0;
    }
    hipEvent_t ev[6] = {};   // before / after the listing; before the oligos, after the unique step, the scores, the fold

private:
    enum { kOrderA, kOrderB, kSlot, kHead, kTemp, kCount, kSlots };
    void *buf_[kSlots] = {};
    size_t cap_[kSlots] = {};
    const uint32_t *sorted_ = nullptr;   // the order unique() left: kOrderA or kOrderB
    int ensure(int slot, size_t bytes, hipStream_t stream, std::string &err);
};

}  // namespace msspe
