// background_thal.hpp -- the kernels between the background site list and the thal pair kernels
// (include/msspe_hip.h msspe_background_thal*): a site's template oligo, and the fold of the scores.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/msspe_hip.h"

namespace msspe {

// Sites [first, first + count) of d_sites (positions in the packed stream d_packed of total_len columns): the
// template oligo of site idx -- the strand the primer anneals to, 5'->3', msspe_pack_oligos form -- goes to
// pool[n + idx] and the pair (primer, n + idx) to list[idx - first]; *list_count = count.
hipError_t launch_site_oligos(const uint64_t *d_packed, size_t total_len, int k, const msspe_site *d_sites,
                              uint32_t first, uint32_t count, int n, uint64_t *pool, uint2 *list,
                              uint32_t *list_count, hipStream_t stream);

// Template flanks (msspe_background_*_flank*): a site's template oligo takes up to kMaxSiteFlank base columns on
// either side of its window; sites are classed by the (fl, fr) they found, class code fl * (flank + 1) + fr.
constexpr int kMaxSiteFlank = 4;
constexpr int kSiteClasses = (kMaxSiteFlank + 1) * (kMaxSiteFlank + 1);
struct SiteClassOffsets {
    uint32_t at[kSiteClasses];   // first list entry of each class's run
};

// launch_site_oligos with flanks: fl / fr = the base columns that end at pos - 1 / start at pos + k, up to `flank`
// each (an invalid column, the separator and the stream's ends stop the count); the template oligo of the
// k + fl + fr columns at pos - fl goes to pool[n + idx], the site's class code to cls[idx - first], and
// class_count[code] (zeroed by the caller) counts the sites of each class.  1 <= flank <= kMaxSiteFlank, k + 2 flank <= 32.
hipError_t launch_site_oligos_flank(const uint64_t *d_packed, size_t total_len, int k, int flank,
                                    const msspe_site *d_sites, uint32_t first, uint32_t count, int n, uint64_t *pool,
                                    uint8_t *cls, uint32_t *class_count, hipStream_t stream);

// The pairs (primer, n + idx) of sites [first, first + count) grouped by class: class c fills
// list[offsets.at[c] ...) in no particular order (offsets: the exclusive scan of launch_site_oligos_flank's counters;
// cursor: kSiteClasses counters, zeroed by the caller).
hipError_t launch_site_group(const msspe_site *d_sites, uint32_t first, uint32_t count, int n, const uint8_t *cls,
                             const SiteClassOffsets &offsets, uint32_t *cursor, uint2 *list, hipStream_t stream);

// Sites [0, count) with their raw scores dg[idx], t[idx]: counts[2 i + s] += sites, counts[2 n + 2 i + s] += stable
// ones (max(0, t) > t_cut) of primer i on strand s; with d_count, one msspe_scored_site per site is appended to
// d_out (at most capacity are stored, *d_count runs on).
hipError_t launch_site_fold(const msspe_site *d_sites, uint32_t count, const double *dg, const double *t,
                            double t_cut, int n, unsigned long long *counts, msspe_scored_site *d_out,
                            uint64_t capacity, uint64_t *d_count, hipStream_t stream);

// The same fold with the stable-key sink of msspe_background_amplicons*: every stable site also appends
// pos << 32 | strand << 31 | primer at d_keys[(*d_key_count)++].  The caller makes room for *d_key_count + count keys
// before the launch (key_cap, the buffer's size, is only the kernel's guard).
hipError_t launch_site_fold_keys(const msspe_site *d_sites, uint32_t count, const double *dg, const double *t,
                                 double t_cut, int n, unsigned long long *counts, msspe_scored_site *d_out,
                                 uint64_t capacity, uint64_t *d_count, uint64_t *d_keys, uint64_t key_cap,
                                 uint64_t *d_key_count, hipStream_t stream);

// The same fold with the position-indexed sink of msspe_stream_reach*: every stable site also ORs bit pos into the
// plane of its strand (d_plane_plus / d_plane_minus: ceil(total_len / 64) words each, cleared by the caller).
hipError_t launch_site_fold_planes(const msspe_site *d_sites, uint32_t count, const double *dg, const double *t,
                                   double t_cut, int n, unsigned long long *counts, msspe_scored_site *d_out,
                                   uint64_t capacity, uint64_t *d_count, uint64_t *d_plane_plus,
                                   uint64_t *d_plane_minus, hipStream_t stream);

}  // namespace msspe
