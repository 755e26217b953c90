// coverage_thal.hip -- segment coverage scored with thal (engine extension, no reference counterpart:
// include/msspe_hip.h msspe_segment_coverage_thal*).  Four kernels around the thal kernels that take explicit pair
// lists (capi.cpp score_site_pairs):
//
// k_coverage_mm_list: the comparison of k_coverage_mm (coverage_mm.hip) -- the same lane mapping, bit planes, LDS
// primer tiles and broadcast reads, from the helpers both share (coverage_mm_core.hpp) -- over groups [g0, g1) and
// primers [p0, p1) of the forward-then-reverse order.  Where the COUNTS instance ORs a segment bit this one appends
// {primer, segment, position, mismatches} to the work list: one 64-bit atomic per match on the list's counter, which
// runs on past the capacity while nothing is written behind it (BackgroundSites::list_slab's contract).  On small
// inputs matches are rare beside comparisons; at 10,000 genomes they are millions and the one counter is what the
// listing costs (measured): a wave-aggregated or LDS-staged append is the next step there.
// It keeps no per-segment minima and no per-primer words, so its tile is the primer words alone: 16 KB, which
// leaves the LDS to more blocks per CU.
//
// k_match_oligos: one lane per list entry.  The k columns of the match are read base by base in either SeqView form
// (a match's window is all bases); read as a word they are the template of a reverse primer as written, and their
// reverse complement is a forward primer's: the plus- and minus-strand rules of k_site_oligos (background_thal.hip).
//
// k_match_fold: one lane per scored match.  held: atomic max of 1 / 2 into the segment's word.  t_best: max(0, t) is
// never negative, so its bits order as an unsigned integer; the word holds bits + 1 and 0 means "no match", which
// keeps a match at 0.0 apart from none.  A slab holds whole (group, primer) cells, so the segments a primer matched
// in, and those it is held in, are two slab-local bitmaps cells[(g - g0) * n_pad + (p - p0)], bit b = segment
// g * S + b (the group-major layout of panel_thin.hip), set with atomic OR.  k_cell_counts then adds every word's
// popcount to the per-primer counters, which therefore add up across slabs.
#include "coverage_thal.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

#include "coverage_mm.hpp"
#include "coverage_mm_core.hpp"

namespace msspe {
namespace {

using namespace mm_core;

constexpr size_t kListLds = 16384;                 // the listing kernel's primer tile
constexpr size_t kCellBudget = (size_t)256 << 20;  // both cell bitmaps of one slab
constexpr uint32_t kOffMask = (1u << kCovOffBits) - 1u;

template <typename T>
__global__ void __launch_bounds__(kThreads) k_coverage_mm_list(const SeqView seqs, int n_seg, int P, int seg_size,
                                                               int stride, int W, int k, int S, int g0, const T *fwd,
                                                               int n_fwd, const T *rev, int n_rev, int p0, int p1,
                                                               int tile_cap, uint32_t lim, uint32_t max_score,
                                                               int scale_shift, CovMatch *list,
                                                               unsigned long long cap, unsigned long long *count)
{
    extern __shared__ __align__(16) unsigned char smem[];
    T *tile = reinterpret_cast<T *>(smem);
    const int tid = threadIdx.x;
    const int per = W - k + 1;
    const long seg0 = ((long)g0 + (long)blockIdx.x) * S;
    const int n_blk = (int)std::min<long>(S, (long)n_seg - seg0);
    const int n_items = n_blk * per;

    for (int dir = 0; dir < 2; ++dir) {
        const T *src = dir ? rev : fwd;
        const int n_u = dir ? n_rev : n_fwd, first = dir ? n_fwd : 0;
        const int lo = std::min(std::max(p0 - first, 0), n_u), hi = std::min(std::max(p1 - first, 0), n_u);
        for (int t0 = lo; t0 < hi; t0 += tile_cap) {
            const int cnt = std::min(tile_cap, hi - t0), cnt4 = (cnt + 3) & ~3;
            __syncthreads();   // the previous tile's readers are done
            for (int i = tid; i < cnt4; i += kThreads) tile[i] = src[t0 + std::min(i, cnt - 1)];   // pad: repeats
            __syncthreads();
            for (int base = 0; base < n_items; base += kRound) {
                uint2 w[kItems];
                uint32_t valid = 0;   // bit j: position j of this round exists and holds k bases
#pragma unroll
                for (int j = 0; j < kItems; ++j) {
                    const int item = base + j * kThreads + tid;
                    uint32_t wl = 0, wh = 0;
                    if (item < n_items) {
                        const int sl = item / per, p = item - sl * per;
                        const int g = (int)seg0 + sl, r = g / P;   // n_seg < 2^31 (checked by the caller)
                        const size_t rec = (size_t)r, part = (size_t)(g - r * P);
                        const size_t col = part * (size_t)stride + (size_t)(dir ? seg_size - W : 0) + (size_t)p;
                        bool ok = true;
                        for (int q = 0; q < k; ++q) {
                            int c = base_at(seqs, rec, col + (size_t)(dir ? k - 1 - q : q));
                            ok &= c >= 0;
                            c = dir ? 3 - (c & 3) : c & 3;   // reverse: complement of the tail base, in primer order
                            wl |= (uint32_t)(c & 1) << q;
                            wh |= (uint32_t)(c >> 1) << q;
                        }
                        valid |= (uint32_t)ok << j;
                    }
                    w[j] = make_word(wl, wh, T());
                }
                if (!valid) continue;   // per lane: no barrier inside a round
                for (int i = 0; i < cnt4; i += 4) {
                    uint2 u[4];
                    load4(tile, i, u);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int j = 0; j < kItems; ++j) {
                            const uint32_t d = diff_mask(w[j], u[q]);
                            const uint32_t pc = (uint32_t)__popc(d);
                            // i + q < cnt: a padding repeat of the tile's last primer is not a primer
                            if (d <= lim && pc <= max_score && ((valid >> j) & 1u) && i + q < cnt) {
                                const unsigned long long at = atomicAdd(count, 1ull);
                                if (at < cap) {
                                    const int item = base + j * kThreads + tid;
                                    const int sl = item / per;
                                    CovMatch m;
                                    m.primer = (uint32_t)(first + t0 + i + q);
                                    m.segment = (uint32_t)(seg0 + sl);
                                    m.off_mm = (uint32_t)(item - sl * per) | ((pc >> scale_shift) << kCovOffBits);
                                    list[at] = m;
                                }
                            }
                        }
                }
            }
        }
    }
}

__device__ __forceinline__ uint64_t revcomp_word(uint64_t w, int k)
{
    uint64_t r = __brevll(w);                                                       // bases and their bits reversed
    r = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);    // bit order inside a base restored
    return ~(r >> (64 - 2 * k)) & ((1ull << (2 * k)) - 1ull);                       // 3 - b is ~b on two bits
}

__global__ void __launch_bounds__(kThreads) k_match_oligos(const SeqView seqs, int P, int seg_size, int stride, int W,
                                                           int k, int n_fwd, int n, const CovMatch *list,
                                                           uint32_t first, uint32_t count, uint64_t *pool,
                                                           uint2 *pairs, uint32_t *list_count)
{
    const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
    if (e == 0) *list_count = count;
    if (e >= count) return;
    const uint32_t idx = first + e;
    const CovMatch m = list[idx];
    const bool rev = m.primer >= (uint32_t)n_fwd;
    const uint32_t r = m.segment / (uint32_t)P, part = m.segment - r * (uint32_t)P;
    const size_t col = (size_t)part * (size_t)stride + (size_t)(rev ? seg_size - W : 0) + (size_t)(m.off_mm & kOffMask);
    uint64_t w = 0;
    for (int q = 0; q < k; ++q) w |= (uint64_t)(base_at(seqs, (size_t)r, col + (size_t)q) & 3) << (2 * q);
    pool[(size_t)n + idx] = rev ? w : revcomp_word(w, k);
    pairs[e] = make_uint2(m.primer, (uint32_t)n + idx);
}

__global__ void __launch_bounds__(kThreads) k_match_fold(const CovMatch *list, uint32_t count, const double *dg,
                                                         const double *t, double t_cut, int S, long g0, int p0,
                                                         size_t n_pad, size_t plane, uint32_t *held,
                                                         unsigned long long *best, unsigned long long *cells,
                                                         msspe_scored_match *out, unsigned long long capacity,
                                                         unsigned long long *out_count)
{
    const uint32_t idx = blockIdx.x * kThreads + threadIdx.x;
    const bool live = idx < count;
    const int lane = threadIdx.x & 63;
    const unsigned long long m_live = __ballot(live);
    if (!m_live) return;   // wave-uniform
    CovMatch m = list[live ? idx : 0];
    const double ti = live ? t[idx] : 0.0, gi = live ? dg[idx] : 0.0;
    const double tm = ti > 0.0 ? ti : 0.0;
    const bool stable = live && tm > t_cut;
    if (live) {
        atomicMax(&held[m.segment], stable ? 2u : 1u);
        atomicMax(&best[m.segment], (unsigned long long)__double_as_longlong(tm) + 1ull);
        const long g = (long)(m.segment / (uint32_t)S);
        const unsigned long long bit = 1ull << (m.segment - (uint32_t)g * (uint32_t)S);
        const size_t cell = (size_t)(g - g0) * n_pad + (size_t)((int)m.primer - p0);
        atomicOr(&cells[cell], bit);
        if (stable) atomicOr(&cells[plane + cell], bit);
    }
    if (out_count) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(out_count, (unsigned long long)__popcll(m_live));   // lane 0 is live
        base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
               (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        const unsigned long long at = base + (unsigned long long)__popcll(m_live & ((1ull << lane) - 1ull));
        if (live && at < capacity) {
            msspe_scored_match r;
            r.primer = m.primer;
            r.segment = m.segment;
            r.offset = m.off_mm & kOffMask;
            r.mismatches = (uint16_t)(m.off_mm >> kCovOffBits);
            r.stable = stable ? 1u : 0u;
            r.dg = gi;
            r.t = ti;
            out[at] = r;
        }
    }
}

// counts[p] += segments primer p matched in, counts[n + p] += segments it is held in, over the slab's cells
__global__ void __launch_bounds__(kThreads) k_cell_counts(const unsigned long long *cells, size_t plane, size_t n_pad,
                                                          int p0, int n_slab, int n, uint32_t *counts)
{
    const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= 2 * plane) return;
    const size_t which = idx >= plane ? 1 : 0, c = idx - which * plane, pl = c % n_pad;
    if (pl >= (size_t)n_slab) return;
    const int bits = __popcll(cells[idx]);
    if (bits) atomicAdd(&counts[which * (size_t)n + (size_t)p0 + pl], (uint32_t)bits);
}

#define CT_TRY(expr)                                                        \
    do {                                                                    \
        hipError_t e__ = (expr);                                            \
        if (e__ != hipSuccess) {                                            \
            err = std::string(#expr) + ": " + hipGetErrorString(e__);       \
            return MSSPE_ERR_DEVICE;                                        \
        }                                                                   \
    } while (0)

template <typename T>
int launch_list(const SeqView &d_seqs, long n_seg, long P, const msspe_kmer_opt &opt, int M, int E, long g0, long g1,
                int p0, int p1, const void *d_words, int n_fwd, int n_rev, CovMatch *list, uint64_t cap,
                uint64_t *d_count, hipStream_t stream, std::string &err)
{
    const int k = opt.kmer_size;
    constexpr bool narrow = sizeof(T) == 4;
    const int tile_cap = std::max(4, std::min((int)(kListLds / sizeof(T)), (p1 - p0 + 3) & ~3));
    const T *words = (const T *)d_words;
    hipLaunchKernelGGL((k_coverage_mm_list<T>), dim3((unsigned)(g1 - g0)), dim3(kThreads),
                       (size_t)tile_cap * sizeof(T), stream, d_seqs, (int)n_seg, (int)P, opt.segment_size,
                       opt.overlap_size, opt.search_window_size, k, MismatchCoverage::group_size(opt), (int)g0, words,
                       n_fwd, words + n_fwd, n_rev, p0, p1, tile_cap, exact_3p_limit<T>(k, E),
                       (uint32_t)(M * (narrow ? 2 : 1)), narrow ? 1 : 0, list, (unsigned long long)cap,
                       (unsigned long long *)d_count);
    CT_TRY(hipGetLastError());
    return MSSPE_OK;
}

}  // namespace

int CoverageThal::ensure(int slot, size_t bytes, hipStream_t stream, std::string &err)
{
    if (cap_[slot] >= bytes && buf_[slot]) return MSSPE_OK;
    if (buf_[slot]) {
        CT_TRY(hipStreamSynchronize(stream));   // an earlier call's last reader
        (void)hipFree(buf_[slot]);
    }
    buf_[slot] = nullptr;
    cap_[slot] = 0;
    const hipError_t e = hipMalloc(&buf_[slot], bytes ? bytes : 16);
    if (e != hipSuccess) {
        err = std::string("hipMalloc (coverage_thal): ") + hipGetErrorString(e);
        return MSSPE_ERR_DEVICE;
    }
    cap_[slot] = bytes;
    return MSSPE_OK;
}

void CoverageThal::release()
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
}

long CoverageThal::max_slab_groups(int n_primers)
{
    const size_t n_pad = ((size_t)std::max(n_primers, 1) + 63) & ~(size_t)63;
    return (long)std::max<size_t>(1, kCellBudget / (2 * sizeof(uint64_t) * n_pad));
}

int CoverageThal::prepare(const msspe_kmer_opt &opt, const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words,
                          int n_rev, long n_seg, hipStream_t stream, std::string &err)
{
    const int n = n_fwd + n_rev;
    int rc;
    if ((rc = ensure(kHeld, sizeof(uint32_t) * (size_t)n_seg, stream, err)) ||
        (rc = ensure(kBest, sizeof(uint64_t) * (size_t)n_seg, stream, err)) ||
        (rc = ensure(kCounts, sizeof(uint32_t) * 2 * (size_t)n, stream, err)) ||
        (rc = prepare_words(opt, fwd_words, n_fwd, rev_words, n_rev, stream, err)))
        return rc;
    CT_TRY(hipMemsetAsync(buf_[kHeld], 0, sizeof(uint32_t) * (size_t)n_seg, stream));
    CT_TRY(hipMemsetAsync(buf_[kBest], 0, sizeof(uint64_t) * (size_t)n_seg, stream));
    CT_TRY(hipMemsetAsync(buf_[kCounts], 0, sizeof(uint32_t) * 2 * (size_t)n, stream));
    return MSSPE_OK;
}

int CoverageThal::prepare_words(const msspe_kmer_opt &opt, const uint64_t *fwd_words, int n_fwd,
                                const uint64_t *rev_words, int n_rev, hipStream_t stream, std::string &err)
{
    const int k = opt.kmer_size, n = n_fwd + n_rev;
    for (hipEvent_t &e : ev)
        if (!e) CT_TRY(hipEventCreate(&e));
    const bool narrow = k <= 16;
    int rc;
    if ((rc = ensure(kWords, (narrow ? 4 : 8) * (size_t)n, stream, err))) return rc;
    n_fwd_ = n_fwd;
    n_rev_ = n_rev;
    // the host copies of the planes end with their block: the stream is drained there
    if (narrow) {
        std::vector<uint32_t> w;
        to_planes<uint32_t>(fwd_words, n_fwd, w);
        to_planes<uint32_t>(rev_words, n_rev, w);
        if (!w.empty())
            CT_TRY(hipMemcpyAsync(buf_[kWords], w.data(), sizeof(uint32_t) * w.size(), hipMemcpyHostToDevice, stream));
        CT_TRY(hipStreamSynchronize(stream));
    } else {
        std::vector<uint2> w;
        to_planes<uint2>(fwd_words, n_fwd, w);
        to_planes<uint2>(rev_words, n_rev, w);
        if (!w.empty())
            CT_TRY(hipMemcpyAsync(buf_[kWords], w.data(), sizeof(uint2) * w.size(), hipMemcpyHostToDevice, stream));
        CT_TRY(hipStreamSynchronize(stream));
    }
    return MSSPE_OK;
}

int CoverageThal::list_slab(const SeqView &seqs, long n_seg, long P, const msspe_kmer_opt &opt, int max_mismatches,
                            int exact_3p, long g0, long g1, int p0, int p1, CovMatch *list, uint64_t cap,
                            uint64_t *d_count, hipStream_t stream, std::string &err)
{
    if (g1 <= g0 || p1 <= p0) return MSSPE_OK;
    return opt.kmer_size <= 16
               ? launch_list<uint32_t>(seqs, n_seg, P, opt, max_mismatches, exact_3p, g0, g1, p0, p1, buf_[kWords],
                                       n_fwd_, n_rev_, list, cap, d_count, stream, err)
               : launch_list<uint2>(seqs, n_seg, P, opt, max_mismatches, exact_3p, g0, g1, p0, p1, buf_[kWords],
                                    n_fwd_, n_rev_, list, cap, d_count, stream, err);
}

hipError_t CoverageThal::oligos(const SeqView &seqs, long P, const msspe_kmer_opt &opt, const CovMatch *list,
                                uint32_t first, uint32_t count, uint64_t *pool, uint2 *pairs, uint32_t *list_count,
                                hipStream_t stream)
{
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(k_match_oligos, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, seqs,
                       (int)P, opt.segment_size, opt.overlap_size, opt.search_window_size, opt.kmer_size, n_fwd_,
                       n_fwd_ + n_rev_, list, first, count, pool, pairs, list_count);
    return hipGetLastError();
}

int CoverageThal::fold_slab(const CovMatch *list, uint32_t count, const double *dg, const double *t, double t_cut,
                            const msspe_kmer_opt &opt, long g0, long g1, int p0, int p1, msspe_scored_match *d_out,
                            uint64_t capacity, uint64_t *d_count, hipStream_t stream, std::string &err)
{
    if (!count) return MSSPE_OK;
    const size_t n_pad = ((size_t)(p1 - p0) + 63) & ~(size_t)63, plane = (size_t)(g1 - g0) * n_pad;
    int rc = ensure(kCells, 2 * sizeof(uint64_t) * plane, stream, err);
    if (rc) return rc;
    unsigned long long *cells = (unsigned long long *)buf_[kCells];
    CT_TRY(hipMemsetAsync(cells, 0, 2 * sizeof(uint64_t) * plane, stream));
    hipLaunchKernelGGL(k_match_fold, dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, list, count,
                       dg, t, t_cut, MismatchCoverage::group_size(opt), g0, p0, n_pad, plane, (uint32_t *)buf_[kHeld],
                       (unsigned long long *)buf_[kBest], cells, d_out, (unsigned long long)capacity,
                       (unsigned long long *)(d_out ? d_count : nullptr));
    CT_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cell_counts, dim3((unsigned)((2 * plane + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       stream, cells, plane, n_pad, p0, p1 - p0, n_fwd_ + n_rev_, (uint32_t *)buf_[kCounts]);
    CT_TRY(hipGetLastError());
    return MSSPE_OK;
}

int CoverageThal::out_list(uint64_t capacity, msspe_scored_match **d_out, uint64_t **d_count, hipStream_t stream,
                           std::string &err)
{
    const size_t list_bytes = sizeof(msspe_scored_match) * (size_t)capacity;
    int rc = ensure(kOut, list_bytes + sizeof(uint64_t), stream, err);
    if (rc) return rc;
    *d_out = (msspe_scored_match *)buf_[kOut];
    *d_count = (uint64_t *)((char *)buf_[kOut] + list_bytes);
    CT_TRY(hipMemsetAsync(*d_count, 0, sizeof(uint64_t), stream));
    return MSSPE_OK;
}

int CoverageThal::finish(long n_seg, uint8_t *held_out, double *t_best_out, uint32_t *primer_segments_out,
                         uint32_t *primer_held_out, hipStream_t stream, std::string &err)
{
    const size_t n = (size_t)(n_fwd_ + n_rev_);
    std::vector<uint32_t> held((size_t)n_seg), counts(2 * n);
    std::vector<uint64_t> best(t_best_out ? (size_t)n_seg : 0);
    CT_TRY(hipMemcpyAsync(held.data(), buf_[kHeld], sizeof(uint32_t) * held.size(), hipMemcpyDeviceToHost, stream));
    if (t_best_out)
        CT_TRY(hipMemcpyAsync(best.data(), buf_[kBest], sizeof(uint64_t) * best.size(), hipMemcpyDeviceToHost,
                              stream));
    if (n) CT_TRY(hipMemcpyAsync(counts.data(), buf_[kCounts], sizeof(uint32_t) * 2 * n, hipMemcpyDeviceToHost, stream));
    CT_TRY(hipStreamSynchronize(stream));
    for (size_t s = 0; s < held.size(); ++s) held_out[s] = (uint8_t)held[s];
    if (t_best_out)
        for (size_t s = 0; s < best.size(); ++s) {
            const uint64_t bits = best[s] ? best[s] - 1 : 0;   // 0: no match
            std::memcpy(&t_best_out[s], &bits, sizeof bits);
        }
    if (primer_segments_out) std::copy(counts.begin(), counts.begin() + n, primer_segments_out);
    if (primer_held_out) std::copy(counts.begin() + n, counts.end(), primer_held_out);
    return MSSPE_OK;
}

}  // namespace msspe
