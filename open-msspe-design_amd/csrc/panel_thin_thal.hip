// panel_thin_thal.hip -- a panel thinned on the segments it holds at a temperature (engine extension).
//
// msspe_panel_thin* thins on the string rule's incidence; msspe_segment_coverage_thal* showed that rule to be a poor
// stand-in for "the primer holds here".  This call runs the greedy rounds of panel_thin.hip over H[p][s] = "primer p
// has a STABLE match in segment s": the matches come slab by slab from coverage_thal.hip's listing, are scored by the
// pair-list kernels (capi.cpp score_site_pairs), and are folded into the group-major matrix the rounds read.
//
// Stability is a property of (primer, template oligo) alone, and an alignment of related genomes repeats its templates
// row after row, so a slab's matches hold few distinct pairs (10,000 x 30 kb, config2 panel: 5.6 M matches, 63 k
// pairs).  Four small kernels around two rocPRIM calls score each pair once:
//
// k_match_keys: one lane per match, the key (primer, template word).  The template is 2 k <= 62 bits; with the primer
// index above it where both fit 64 bits, one sort pass orders the matches.  Where they do not (long oligos, large
// panels) the sort runs twice, both stable: by template, then -- k_primer_keys gathers the keys in the new order -- by
// primer.
// k_unique_heads: position j of the sorted order starts a run when its primer or its template differs from position
// j - 1's (read from the list and the pool through the order, so the rule is one for both key forms).  An inclusive
// scan of the flags numbers the runs from 1.
// k_unique_pairs: a run's head writes the pair (primer, pool index of its own template) at the run's slot; the last
// position writes the number of runs.  The scores land at the head's match index, as score_site_pairs writes them;
// that index is also kept per run, because the list stages of the scoring sort the pair list they are given in place.
// k_held_incidence: one lane per match; t is read where the match's run was scored (or at the match itself when every
// match was scored), and a stable match sets its segment's bit in inc[g * n_pad + primer] with an atomic OR: slabs are
// split by groups and by primers, several matches of a primer share a word, and the matrix is zeroed once per call.
#include "panel_thin_thal.hpp"

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace msspe {
namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) k_match_keys(const CovMatch *list, const uint64_t *pool, int n,
                                                         uint32_t count, int primer_shift, uint64_t *keys,
                                                         uint32_t *order)
{
    const uint32_t idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= count) return;
    const uint64_t tmpl = pool[(size_t)n + idx];
    // primer_shift < 0: the template alone (the primer is the second pass's key)
    keys[idx] = primer_shift >= 0 ? ((uint64_t)list[idx].primer << primer_shift) | tmpl : tmpl;
    order[idx] = idx;
}

__global__ void __launch_bounds__(kThreads) k_primer_keys(const CovMatch *list, const uint32_t *order, uint32_t count,
                                                          uint32_t *keys)
{
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j < count) keys[j] = list[order[j]].primer;
}

__global__ void __launch_bounds__(kThreads) k_unique_heads(const CovMatch *list, const uint64_t *pool, int n,
                                                           const uint32_t *order, uint32_t count, uint32_t *heads)
{
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= count) return;
    const uint32_t idx = order[j];
    uint32_t head = 1;
    if (j) {
        const uint32_t prev = order[j - 1];
        head = list[idx].primer != list[prev].primer || pool[(size_t)n + idx] != pool[(size_t)n + prev];
    }
    heads[j] = head;
}

__global__ void __launch_bounds__(kThreads) k_unique_pairs(const CovMatch *list, const uint32_t *order,
                                                           const uint32_t *heads, const uint32_t *slot, uint32_t count,
                                                           int n, uint2 *pairs, uint32_t *run_head,
                                                           uint32_t *n_unique)
{
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= count) return;
    const uint32_t s = slot[j];   // 1 .. runs, and runs <= count: the pair list holds `count` entries
    if (heads[j]) {
        const uint32_t idx = order[j];
        pairs[s - 1] = make_uint2(list[idx].primer, (uint32_t)n + idx);
        run_head[s - 1] = idx;
    }
    if (j == count - 1) *n_unique = s;
}

__global__ void __launch_bounds__(kThreads) k_held_incidence(const CovMatch *list, uint32_t count,
                                                             const uint32_t *order, const uint32_t *slot,
                                                             const uint32_t *run_head, const double *t,
                                                             double t_cut, int S, size_t n_pad,
                                                             unsigned long long *inc)
{
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    const bool live = j < count;
    if (!__ballot(live)) return;   // wave-uniform
    if (!live) return;
    // by run: position j of the sorted order, scored at its run's head; otherwise match j, scored itself
    const uint32_t idx = order ? order[j] : j;
    const uint32_t at = order ? run_head[slot[j] - 1] : idx;
    const double ti = t[at];
    if (!((ti > 0.0 ? ti : 0.0) > t_cut)) return;
    const CovMatch m = list[idx];
    const uint32_t g = m.segment / (uint32_t)S;
    atomicOr(&inc[(size_t)g * n_pad + (size_t)m.primer], 1ull << (m.segment - g * (uint32_t)S));
}

#define TT_TRY(expr)                                                                   \
    do {                                                                               \
        hipError_t e__ = (expr);                                                       \
        if (e__ != hipSuccess) {                                                       \
            err = std::string("panel thin thal, " #expr ": ") + hipGetErrorString(e__); \
            return MSSPE_ERR_DEVICE;                                                   \
        }                                                                              \
    } while (0)

}  // namespace

int PanelThinThal::ensure(int slot, size_t bytes, hipStream_t stream, std::string &err)
{
    if (cap_[slot] >= bytes && buf_[slot]) return MSSPE_OK;
    if (buf_[slot]) {
        TT_TRY(hipStreamSynchronize(stream));   // an earlier slab's last reader
        (void)hipFree(buf_[slot]);
    }
    buf_[slot] = nullptr;
    cap_[slot] = 0;
    const hipError_t e = hipMalloc(&buf_[slot], bytes ? bytes : 16);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        buf_[slot] = nullptr;
        err = std::string("hipMalloc (panel thin thal): ") + hipGetErrorString(e);
        return MSSPE_ERR_DEVICE;
    }
    cap_[slot] = bytes;
    return MSSPE_OK;
}

int PanelThinThal::events(std::string &err)
{
    for (hipEvent_t &e : ev)
        if (!e) TT_TRY(hipEventCreate(&e));
    return MSSPE_OK;
}

void PanelThinThal::release()
{
    for (int s = 0; s < kSlots; ++s) {
        if (buf_[s]) (void)hipFree(buf_[s]);
        buf_[s] = nullptr;
        cap_[s] = 0;
    }
    for (hipEvent_t &e : ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    sorted_ = nullptr;
}

int PanelThinThal::unique(const CovMatch *list, const uint64_t *pool, int n, int k, uint32_t count, uint64_t *keys_a,
                          uint64_t *keys_b, uint2 *pairs, hipStream_t stream, std::string &err)
{
    sorted_ = nullptr;
    if (!count) return MSSPE_OK;
    unsigned n_bits = 1;   // bits of the greatest primer index
    while (n_bits < 32 && ((uint64_t)1 << n_bits) < (uint64_t)n) ++n_bits;
    const unsigned t_bits = 2u * (unsigned)k;
    const bool one_pass = t_bits + n_bits <= 64;
    // the arrays grow by doubling, so a call's first slabs do not each allocate
    size_t room = cap_[kSlot] / sizeof(uint32_t);
    if (room < count) {
        room = std::max<size_t>(room, 4096);
        while (room < count) room *= 2;
    }
    size_t tmp_sort = 0, tmp_sort2 = 0, tmp_scan = 0;
    uint32_t *o_a = nullptr, *o_b = nullptr;
    TT_TRY(rocprim::radix_sort_pairs(nullptr, tmp_sort, keys_a, keys_b, o_a, o_b, room, 0u,
                                     one_pass ? t_bits + n_bits : t_bits, stream));
    if (!one_pass)
        TT_TRY(rocprim::radix_sort_pairs(nullptr, tmp_sort2, (uint32_t *)nullptr, (uint32_t *)nullptr, o_b, o_a, room,
                                         0u, n_bits, stream));
    TT_TRY(rocprim::inclusive_scan(nullptr, tmp_scan, (uint32_t *)nullptr, (uint32_t *)nullptr, room,
                                   rocprim::plus<uint32_t>(), stream));
    size_t tmp_bytes = std::max(std::max(tmp_sort, tmp_sort2), tmp_scan);
    int rc;
    if ((rc = ensure(kOrderA, sizeof(uint32_t) * room, stream, err)) ||
        (rc = ensure(kOrderB, sizeof(uint32_t) * room, stream, err)) ||
        (rc = ensure(kSlot, sizeof(uint32_t) * room, stream, err)) ||
        (rc = ensure(kHead, sizeof(uint32_t) * room, stream, err)) || (rc = ensure(kTemp, tmp_bytes, stream, err)) ||
        (rc = ensure(kCount, sizeof(uint32_t), stream, err)))
        return rc;
    o_a = (uint32_t *)buf_[kOrderA];
    o_b = (uint32_t *)buf_[kOrderB];
    uint32_t *slot = (uint32_t *)buf_[kSlot], *heads = (uint32_t *)keys_a;   // the keys are done with by then
    tmp_bytes = cap_[kTemp];
    const dim3 grid((count + kThreads - 1) / kThreads), block(kThreads);
    hipLaunchKernelGGL(k_match_keys, grid, block, 0, stream, list, pool, n, count, one_pass ? (int)t_bits : -1, keys_a,
                       o_a);
    TT_TRY(hipGetLastError());
    TT_TRY(rocprim::radix_sort_pairs(buf_[kTemp], tmp_bytes, keys_a, keys_b, o_a, o_b, (size_t)count, 0u,
                                     one_pass ? t_bits + n_bits : t_bits, stream));
    const uint32_t *order = o_b;
    if (!one_pass) {
        uint32_t *k32_in = (uint32_t *)keys_a, *k32_out = (uint32_t *)keys_b;
        hipLaunchKernelGGL(k_primer_keys, grid, block, 0, stream, list, o_b, count, k32_in);
        TT_TRY(hipGetLastError());
        TT_TRY(rocprim::radix_sort_pairs(buf_[kTemp], tmp_bytes, k32_in, k32_out, o_b, o_a, (size_t)count, 0u, n_bits,
                                         stream));
        order = o_a;
    }
    hipLaunchKernelGGL(k_unique_heads, grid, block, 0, stream, list, pool, n, order, count, heads);
    TT_TRY(hipGetLastError());
    TT_TRY(rocprim::inclusive_scan(buf_[kTemp], tmp_bytes, heads, slot, (size_t)count, rocprim::plus<uint32_t>(),
                                   stream));
    hipLaunchKernelGGL(k_unique_pairs, grid, block, 0, stream, list, order, heads, slot, count, n, pairs,
                       (uint32_t *)buf_[kHead], (uint32_t *)buf_[kCount]);
    TT_TRY(hipGetLastError());
    sorted_ = order;
    return MSSPE_OK;
}

int PanelThinThal::fold(const CovMatch *list, uint32_t count, bool by_run, const double *t, double t_cut, int S,
                        size_t n_pad, uint64_t *inc, hipStream_t stream, std::string &err)
{
    if (!count) return MSSPE_OK;
    if (by_run && !sorted_) {
        err = "panel thin thal: a fold by run without the slab's order";
        return MSSPE_ERR_DEVICE;
    }
    hipLaunchKernelGGL(k_held_incidence, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, list,
                       count, by_run ? sorted_ : (const uint32_t *)nullptr,
                       by_run ? (const uint32_t *)buf_[kSlot] : (const uint32_t *)nullptr,
                       (const uint32_t *)buf_[kHead], t, t_cut, S, n_pad, (unsigned long long *)inc);
    TT_TRY(hipGetLastError());
    return MSSPE_OK;
}

}  // namespace msspe
