// background_thal.hip -- what lies between the background site list (background.hip) and the f64 thal kernels that
// take explicit pair lists (engine extension, no reference counterpart: include/msspe_hip.h msspe_background_thal*).
//
// k_site_oligos: one lane per site record.  The k columns at pos are cut out of the packed 2-bit row (a window
// straddles at most two 64-bit words for k <= 31; a site's window is all bases, so the validity words are not read).
// The packed row and msspe_pack_oligos agree on the coding (A C G T = 0 1 2 3, the first base in the low bits), so
// the window IS the word of the minus-strand site's template; the plus strand's is its reverse complement: v_bfrev,
// a swap within pairs, a shift and a not.  The word goes into the site pool behind the primers, P' = [primers | site
// oligos], and the pair is (primer, n + idx): a PairSinks with ncols = 0 and col0 = n then lands on the list index.
//
// k_site_fold: one lane per scored site.  Sites arrive grouped by (primer, strand) in long stretches (the site
// kernel walks the primers of a tile in order), so a wave whose lanes agree on the key adds its two popcounts with
// one atomic each; a mixed wave adds per lane.  The caller's records take one atomic per wave for their places.
// k_site_fold_keys is the same fold with a second sink (msspe_background_amplicons*): one 64-bit key,
// pos << 32 | strand << 31 | primer, per STABLE site, appended to a buffer the caller has sized for every site of
// the launch, again with one atomic per wave.  The sink is a template flag of the shared body, so k_site_fold itself
// is the kernel it was.
// k_site_fold_planes is the fold with a position-indexed sink (msspe_stream_reach*): every STABLE site ORs bit pos
// into the bit plane of its strand, one 64-bit atomicOr each -- several primers at one position set one bit, so what the
// planes hold does not depend on the number of sites.  Again a template flag of the shared body.
//
// k_site_oligos_flank (msspe_background_*_flank* with flank f > 0): one lane per site record.  The lane gathers the
// validity bits of the 2 f + k columns at pos - f (columns before the stream and behind it read as invalid) and counts
// the base columns that end at pos - 1 (fl) and start at pos + k (fr), each capped at f; the k + fl + fr <= 32
// columns at pos - fl lie in at most two base words.  Sites of one (fl, fr) share one template length, the pair
// kernels take one length per launch, so the lane also writes its class code fl (f + 1) + fr and the wave adds to the
// (f + 1)^2 class counters with one atomic per class it holds.  k_site_group then scatters the pairs
// (primer, n + idx) into one contiguous run of the list per class -- the runs' offsets are the host's exclusive scan
// of the counters, a wave takes its places in a run with one atomic on the run's cursor -- so that every class is one
// explicit pair list; dg and t stay indexed by the site, and the fold is the one above.
#include "background_thal.hpp"

#include <cmath>

namespace msspe {
namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ uint64_t revcomp_word(uint64_t w, int k)
{
    uint64_t r = __brevll(w);                                                       // bases and their bits reversed
    r = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);    // bit order inside a base restored
    return ~(r >> (64 - 2 * k)) & ((1ull << (2 * k)) - 1ull);                       // 3 - b is ~b on two bits
}

__global__ void __launch_bounds__(kThreads) k_site_oligos(const uint64_t *packed, size_t total_len, int k,
                                                          const msspe_site *sites, uint32_t first, uint32_t count,
                                                          int n, uint64_t *pool, uint2 *list, uint32_t *list_count)
{
    const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
    if (e == 0) *list_count = count;
    if (e >= count) return;
    const uint32_t idx = first + e;
    const msspe_site s = sites[idx];
    const size_t bw = (total_len + 31) / 32, wi = (size_t)(s.pos >> 5);
    const int sh = 2 * (int)(s.pos & 31u);
    const uint64_t lo = wi < bw ? packed[wi] : 0ull;
    const uint64_t hi = (sh + 2 * k > 64 && wi + 1 < bw) ? packed[wi + 1] : 0ull;
    uint64_t w = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    w &= (1ull << (2 * k)) - 1ull;
    pool[(size_t)n + idx] = s.strand ? w : revcomp_word(w, k);
    list[e] = make_uint2(s.primer, (uint32_t)n + idx);
}

__device__ __forceinline__ uint64_t low_bases(int len) { return len >= 32 ? ~0ull : (1ull << (2 * len)) - 1ull; }

// 64 validity bits from column c0 on (c0 may be negative): bit j is column c0 + j, 0 outside the stream
__device__ __forceinline__ uint64_t valid_from(const uint64_t *valid, size_t nv, long long c0)
{
    const int lead = c0 < 0 ? (int)-c0 : 0;   // <= kMaxSiteFlank
    const size_t c = (size_t)(c0 + lead), wi = c >> 6;
    const int sh = (int)(c & 63u);
    const uint64_t lo = wi < nv ? valid[wi] : 0ull;
    const uint64_t hi = (sh && wi + 1 < nv) ? valid[wi + 1] : 0ull;
    const uint64_t v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    return v << lead;
}

__global__ void __launch_bounds__(kThreads) k_site_oligos_flank(const uint64_t *packed, size_t total_len, int k,
                                                                int f, const msspe_site *sites, uint32_t first,
                                                                uint32_t count, int n, uint64_t *pool, uint8_t *cls,
                                                                uint32_t *class_count)
{
    const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
    const bool live = e < count;
    const int lane = threadIdx.x & 63;
    int code = 0;
    if (live) {
        const uint32_t idx = first + e;
        const msspe_site s = sites[idx];
        const size_t bw = (total_len + 31) / 32, nv = (total_len + 63) / 64;
        // columns beyond total_len hold validity 0 (k_pack_stream), so the stream's end stops a flank like an N
        const uint64_t v = valid_from(packed + bw, nv, (long long)s.pos - f);
        const uint32_t fmask = (1u << f) - 1u;
        const uint32_t gap_l = ~(uint32_t)v & fmask;                   // bit j: column pos - f + j holds no base
        const uint32_t gap_r = ~(uint32_t)(v >> (f + k)) & fmask;      // bit j: column pos + k + j holds none
        const int fl = gap_l ? f - 1 - (31 - __clz((int)gap_l)) : f;   // base columns above the highest gap
        const int fr = gap_r ? __ffs((int)gap_r) - 1 : f;              // ... below the lowest
        const int len = k + fl + fr;
        const size_t a = (size_t)s.pos - (size_t)fl, wi = a >> 5;
        const int sh = 2 * (int)(a & 31u);
        const uint64_t lo = wi < bw ? packed[wi] : 0ull;
        const uint64_t hi = (sh + 2 * len > 64 && wi + 1 < bw) ? packed[wi + 1] : 0ull;
        uint64_t w = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
        w &= low_bases(len);
        if (!s.strand) {   // revcomp_word at a length that may be 32
            uint64_t r = __brevll(w);
            r = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);
            w = ~(r >> (64 - 2 * len)) & low_bases(len);
        }
        pool[(size_t)n + idx] = w;
        code = fl * (f + 1) + fr;
        cls[e] = (uint8_t)code;
    }
    unsigned long long todo = __ballot(live);
    while (todo) {   // wave-uniform: one turn per class the wave holds
        const int leader = __ffsll(todo) - 1;
        const int c0 = __shfl(code, leader);
        const unsigned long long same = __ballot(live && code == c0);
        if (lane == leader) atomicAdd(&class_count[c0], (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

__global__ void __launch_bounds__(kThreads) k_site_group(const msspe_site *sites, uint32_t first, uint32_t count,
                                                         int n, const uint8_t *cls, SiteClassOffsets off,
                                                         uint32_t *cursor, uint2 *list)
{
    const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
    const bool live = e < count;
    const int lane = threadIdx.x & 63;
    const int code = live ? (int)cls[e] : 0;
    const uint32_t primer = live ? sites[first + e].primer : 0u;
    unsigned long long todo = __ballot(live);
    while (todo) {   // wave-uniform
        const int leader = __ffsll(todo) - 1;
        const int c0 = __shfl(code, leader);
        const unsigned long long same = __ballot(live && code == c0);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&cursor[c0], (uint32_t)__popcll(same));
        base = (uint32_t)__shfl((int)base, leader);
        if (live && code == c0) {
            const uint32_t at = off.at[c0] + base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
            if (at < count) list[at] = make_uint2(primer, (uint32_t)n + first + e);
        }
        todo &= ~same;
    }
}

template <bool kKeys, bool kPlanes = false>
__device__ __forceinline__ void site_fold(const msspe_site *sites, uint32_t count, const double *dg, const double *t,
                                          double t_cut, int n, unsigned long long *counts, msspe_scored_site *out,
                                          unsigned long long capacity, unsigned long long *out_count,
                                          unsigned long long *keys, unsigned long long key_cap,
                                          unsigned long long *key_count,
                                          unsigned long long *plane_plus = nullptr,
                                          unsigned long long *plane_minus = nullptr)
{
    const uint32_t idx = blockIdx.x * kThreads + threadIdx.x;
    const bool live = idx < count;
    const int lane = threadIdx.x & 63;
    msspe_site s = sites[live ? idx : 0];
    const double ti = live ? t[idx] : 0.0, gi = live ? dg[idx] : 0.0;
    const bool stable = live && (ti > 0.0 ? ti : 0.0) > t_cut;
    const uint32_t key = 2u * s.primer + s.strand;
    const unsigned long long m_live = __ballot(live), m_stable = __ballot(stable);
    if (!m_live) return;   // wave-uniform
    const uint32_t key0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);   // lane 0 is live where any lane is
    if (__all(!live || key == key0)) {
        if (lane == 0) {
            atomicAdd(&counts[key0], (unsigned long long)__popcll(m_live));
            if (m_stable) atomicAdd(&counts[2 * (size_t)n + key0], (unsigned long long)__popcll(m_stable));
        }
    } else if (live) {
        atomicAdd(&counts[key], 1ull);
        if (stable) atomicAdd(&counts[2 * (size_t)n + key], 1ull);
    }
    if (out_count) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(out_count, (unsigned long long)__popcll(m_live));
        base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
               (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        const unsigned long long at = base + (unsigned long long)__popcll(m_live & ((1ull << lane) - 1ull));
        if (live && at < capacity) {
            msspe_scored_site r;
            r.primer = s.primer;
            r.pos = s.pos;
            r.mismatches = s.mismatches;
            r.strand = s.strand;
            r.stable = stable ? 1u : 0u;
            r.dg = gi;
            r.t = ti;
            out[at] = r;
        }
    }
    if (kKeys && m_stable) {   // wave-uniform
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(key_count, (unsigned long long)__popcll(m_stable));
        base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
               (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        const unsigned long long at = base + (unsigned long long)__popcll(m_stable & ((1ull << lane) - 1ull));
        if (stable && at < key_cap)
            keys[at] = ((unsigned long long)s.pos << 32) | ((unsigned long long)s.strand << 31) | s.primer;
    }
    if (kPlanes && stable) atomicOr(&(s.strand ? plane_minus : plane_plus)[s.pos >> 6], 1ull << (s.pos & 63u));
}

__global__ void __launch_bounds__(kThreads) k_site_fold(const msspe_site *sites, uint32_t count, const double *dg,
                                                        const double *t, double t_cut, int n,
                                                        unsigned long long *counts, msspe_scored_site *out,
                                                        unsigned long long capacity, unsigned long long *out_count)
{
    site_fold<false>(sites, count, dg, t, t_cut, n, counts, out, capacity, out_count, nullptr, 0, nullptr);
}

__global__ void __launch_bounds__(kThreads) k_site_fold_keys(const msspe_site *sites, uint32_t count,
                                                             const double *dg, const double *t, double t_cut, int n,
                                                             unsigned long long *counts, msspe_scored_site *out,
                                                             unsigned long long capacity,
                                                             unsigned long long *out_count, unsigned long long *keys,
                                                             unsigned long long key_cap,
                                                             unsigned long long *key_count)
{
    site_fold<true>(sites, count, dg, t, t_cut, n, counts, out, capacity, out_count, keys, key_cap, key_count);
}

__global__ void __launch_bounds__(kThreads) k_site_fold_planes(const msspe_site *sites, uint32_t count,
                                                               const double *dg, const double *t, double t_cut, int n,
                                                               unsigned long long *counts, msspe_scored_site *out,
                                                               unsigned long long capacity,
                                                               unsigned long long *out_count,
                                                               unsigned long long *plane_plus,
                                                               unsigned long long *plane_minus)
{
    site_fold<false, true>(sites, count, dg, t, t_cut, n, counts, out, capacity, out_count, nullptr, 0, nullptr,
                           plane_plus, plane_minus);
}

}  // namespace

hipError_t launch_site_oligos(const uint64_t *d_packed, size_t total_len, int k, const msspe_site *d_sites,
                              uint32_t first, uint32_t count, int n, uint64_t *pool, uint2 *list,
                              uint32_t *list_count, hipStream_t stream)
{
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(k_site_oligos, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, d_packed,
                       total_len, k, d_sites, first, count, n, pool, list, list_count);
    return hipGetLastError();
}

hipError_t launch_site_oligos_flank(const uint64_t *d_packed, size_t total_len, int k, int flank,
                                    const msspe_site *d_sites, uint32_t first, uint32_t count, int n, uint64_t *pool,
                                    uint8_t *cls, uint32_t *class_count, hipStream_t stream)
{
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(k_site_oligos_flank, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, stream,
                       d_packed, total_len, k, flank, d_sites, first, count, n, pool, cls, class_count);
    return hipGetLastError();
}

hipError_t launch_site_group(const msspe_site *d_sites, uint32_t first, uint32_t count, int n, const uint8_t *cls,
                             const SiteClassOffsets &offsets, uint32_t *cursor, uint2 *list, hipStream_t stream)
{
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(k_site_group, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, d_sites,
                       first, count, n, cls, offsets, cursor, list);
    return hipGetLastError();
}

hipError_t launch_site_fold(const msspe_site *d_sites, uint32_t count, const double *dg, const double *t,
                            double t_cut, int n, unsigned long long *counts, msspe_scored_site *d_out,
                            uint64_t capacity, uint64_t *d_count, hipStream_t stream)
{
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(k_site_fold, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, d_sites,
                       count, dg, t, t_cut, n, counts, d_out, (unsigned long long)capacity,
                       (unsigned long long *)d_count);
    return hipGetLastError();
}

hipError_t launch_site_fold_keys(const msspe_site *d_sites, uint32_t count, const double *dg, const double *t,
                                 double t_cut, int n, unsigned long long *counts, msspe_scored_site *d_out,
                                 uint64_t capacity, uint64_t *d_count, uint64_t *d_keys, uint64_t key_cap,
                                 uint64_t *d_key_count, hipStream_t stream)
{
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(k_site_fold_keys, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, d_sites,
                       count, dg, t, t_cut, n, counts, d_out, (unsigned long long)capacity,
                       (unsigned long long *)d_count, (unsigned long long *)d_keys, (unsigned long long)key_cap,
                       (unsigned long long *)d_key_count);
    return hipGetLastError();
}

hipError_t launch_site_fold_planes(const msspe_site *d_sites, uint32_t count, const double *dg, const double *t,
                                   double t_cut, int n, unsigned long long *counts, msspe_scored_site *d_out,
                                   uint64_t capacity, uint64_t *d_count, uint64_t *d_plane_plus,
                                   uint64_t *d_plane_minus, hipStream_t stream)
{
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(k_site_fold_planes, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, d_sites,
                       count, dg, t, t_cut, n, counts, d_out, (unsigned long long)capacity,
                       (unsigned long long *)d_count, (unsigned long long *)d_plane_plus,
                       (unsigned long long *)d_plane_minus);
    return hipGetLastError();
}

}  // namespace msspe
