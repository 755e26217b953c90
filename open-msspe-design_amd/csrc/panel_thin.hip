// panel_thin.hip -- a primer panel thinned to the primers its coverage needs (engine extension).
//
// Stage A picks words by exact occurrence, so two words that differ at one 5' base are both picked although either
// primes both variants.  The rule here is the greedy set cover over the incidence I[p][s] = "primer p has a match in
// segment s" under msspe_segment_coverage_mm's rule: forced primers cover first, then every round keeps the unpicked
// primer with the most uncovered segments (ties: the lowest index) until that gain falls below min_gain.
//
// Phases.  (1) The incidence pass is coverage_mm.hip's kernel in its third instance: the 64-bit LDS word of a block's
// segments a primer matched in is stored, group-major (inc[g * n_pad + p], bit b = segment g * S + b), instead of
// counted.  (2) The forced primers' rows are ORed into cov[g]; one pass over the matrix gives every primer's gain
// (lanes over p: coalesced) and the segments the whole set covers.  (3) A round is three small launches: the argmax of
// gain << 32 | ~p over the live primers, the pick's new segments per group (cov |= new, the groups with any go on a
// list), and for the listed groups alone gain[p] -= popc(inc[g][p] & new[g]).  gain[p] == |I[p] & ~cov| holds for every
// p after every round, so nothing is recomputed.  The rounds are enqueued 16 at a time behind a device word, as the
// tube split's are: after the round that stops, the launches of the batch return at once, and the host reads one
// word per batch.
//
// Depth (msspe_panel_thin_depth*).  Every segment keeps min(R, primers it has) primers instead of one.
// cov[g] then reads "closed": a bit is set once cnt[s] has reached need[s], and gain0 / pick / update run as they
// stand over it.  k_thin_colsum gives the per-segment primer counts (all, forced, kept), k_thin_depth_init the needs
// and the first closed words, k_thin_apply_depth a round's counter bumps and the bits it closes.  Primers listed twice
// (shadows) are masked out of every count and are never live.
//
// Weights (msspe_panel_thin_weighted*).  gain(p) is the sum of a weight per segment over the uncovered
// segments of row p.  The first gains and the update run in their weighted instances (panel_weighted.hpp) over a weight
// plane with the cell layout of the depth planes; forced, pick and apply are the kernels above, unchanged.
//
// Costs (msspe_panel_thin_cost*).  A round keeps the greatest gain / cost instead of the greatest gain:
// the pick runs in its cost instance (panel_cost.hpp) over a cost per primer; every other kernel of the round is the
// one above, weighted or not.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/msspe_hip.h"
#include "panel_cost.hpp"
#include "panel_thin.hpp"
#include "panel_weighted.hpp"

namespace msspe {

namespace {

constexpr int kRoundsPerBatch = 16;   // rounds enqueued between two reads of the "done" word
constexpr int kThreads = 256;
constexpr int kChunk = 32;            // groups per block of the first gains

struct ThinState {
    uint32_t done;        // 1: a round found no gain of min_gain or more (the launches that follow return at once)
    uint32_t rounds;      // rounds that ran: the picks and the one that stopped
    uint32_t n_picked;
    uint32_t pick;        // of the current round
    uint32_t n_touched;   // groups in which the current pick covers something new
    uint32_t pad;
    unsigned long long covered_all;      // |OR of all I[p]|
    unsigned long long covered_forced;   // |OR of the forced I[p]|
};

enum { kInc, kCov, kTouched, kNew, kGain, kLive, kOrder, kForced, kDepth, kMask, kWeight, kCost };   // PanelThin::buf_

__device__ __forceinline__ uint64_t wave_or(uint64_t x)
{
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    for (int o = 32; o; o >>= 1) {
        lo |= __shfl_xor(lo, o, 64);
        hi |= __shfl_xor(hi, o, 64);
    }
    return (uint64_t)hi << 32 | lo;
}

__device__ __forceinline__ uint64_t wave_max(uint64_t x)
{
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)x, o, 64), hi = __shfl_xor((uint32_t)(x >> 32), o, 64);
        x = std::max(x, (uint64_t)hi << 32 | lo);
    }
    return x;
}

// cov[g] = OR of the forced primers' words of group g: one wave per group, lanes over the forced list
__global__ __launch_bounds__(kThreads) void k_thin_forced(const uint64_t *inc, size_t n_pad, int G,
                                                          const uint32_t *forced, int n_forced, uint64_t *cov,
                                                          ThinState *st)
{
    const int lane = threadIdx.x & 63;
    const int waves = gridDim.x * (kThreads / 64);
    for (int g = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); g < G; g += waves) {   // whole waves
        uint64_t w = 0;
        for (int i = lane; i < n_forced; i += 64) w |= inc[(size_t)g * n_pad + forced[i]];
        w = wave_or(w);
        if (lane == 0) {
            cov[g] = w;
            if (w) atomicAdd(&st->covered_forced, (unsigned long long)__popcll(w));
        }
    }
}

// gain[p] += popc(inc[g][p] & ~cov[g]) over the block's chunk of groups: one atomic per (block, primer); the OR of a
// group's words over all primers is collected in LDS, and its popcount added to covered_all
__global__ __launch_bounds__(kThreads) void k_thin_gain0(const uint64_t *inc, int n, size_t n_pad, int G,
                                                         const uint64_t *cov, uint32_t *gain, ThinState *st)
{
    __shared__ uint64_t scov[kChunk], sall[kChunk];
    const int tid = threadIdx.x, lane = tid & 63;
    const int g0 = blockIdx.x * kChunk, cnt = std::min(kChunk, G - g0);
    if (tid < kChunk) {
        scov[tid] = tid < cnt ? cov[g0 + tid] : 0ull;
        sall[tid] = 0ull;
    }
    __syncthreads();
    for (int p0 = 0; p0 < n; p0 += kThreads) {   // whole blocks: the wave reductions below need every lane
        const int p = p0 + tid;
        const bool in = p < n;
        const uint64_t *col = inc + (size_t)g0 * n_pad + (size_t)(in ? p : 0);
        uint32_t sum = 0;
        for (int gi = 0; gi < cnt; ++gi) {
            const uint64_t w = in ? col[(size_t)gi * n_pad] : 0ull;
            sum += (uint32_t)__popcll(w & ~scov[gi]);
            const uint64_t o = wave_or(w);
            if (lane == 0 && o) atomicOr((unsigned long long *)&sall[gi], (unsigned long long)o);
        }
        if (in && sum) atomicAdd(&gain[p], sum);
    }
    __syncthreads();
    if (tid < cnt) {
        const int c = __popcll(sall[tid]);
        if (c) atomicAdd(&st->covered_all, (unsigned long long)c);
    }
}

// One block: the live primer of greatest (gain, lowest index).  Below min_gain (or nobody live) the loop is done.
__global__ __launch_bounds__(kThreads) void k_thin_pick(const uint32_t *gain, uint8_t *live, int n, uint32_t min_gain,
                                                        uint32_t *order, uint32_t *gains, ThinState *st)
{
    if (st->done) return;
    __shared__ uint64_t skey[kThreads / 64];
    const int tid = threadIdx.x;
    uint64_t key = 0;   // a live primer's key is never 0: its low half is 0xFFFFFFFF - p with p < 2^31
    for (int p = tid; p < n; p += kThreads)
        if (live[p]) key = std::max(key, (uint64_t)gain[p] << 32 | (uint64_t)(0xFFFFFFFFu - (uint32_t)p));
    key = wave_max(key);
    if ((tid & 63) == 0) skey[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kThreads / 64; ++w) key = std::max(key, skey[w]);
        const uint32_t g = (uint32_t)(key >> 32);
        st->rounds += 1;
        if (key == 0 || g < min_gain) {
            st->done = 1;
        } else {
            const uint32_t p = 0xFFFFFFFFu - (uint32_t)key, i = st->n_picked;   // i < n: every pick leaves the live set
            order[i] = p;
            gains[i] = g;
            live[p] = 0;
            st->n_picked = i + 1;
            st->pick = p;
            st->n_touched = 0;
        }
    }
}

// new[g] = inc[g][pick] & ~cov[g]; cov[g] |= new[g]; the groups with any go on the touched list (at most G entries)
__global__ __launch_bounds__(kThreads) void k_thin_apply(const uint64_t *inc, size_t n_pad, int G, uint64_t *cov,
                                                         uint32_t *touched, uint64_t *fresh, ThinState *st)
{
    if (st->done) return;
    const long g = (long)blockIdx.x * kThreads + threadIdx.x;
    if (g >= G) return;
    const uint64_t c = cov[g], w = inc[(size_t)g * n_pad + st->pick] & ~c;
    if (!w) return;
    cov[g] = c | w;
    const uint32_t i = atomicAdd(&st->n_touched, 1u);
    touched[i] = (uint32_t)g;
    fresh[i] = w;
}

// gain[p] -= popc(inc[g][p] & new[g]) over the touched groups (blockIdx.y strides over the list), lanes over p
__global__ __launch_bounds__(kThreads) void k_thin_update(const uint64_t *inc, int n, size_t n_pad,
                                                          const uint32_t *touched, const uint64_t *fresh,
                                                          uint32_t *gain, const ThinState *st)
{
    if (st->done) return;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const uint32_t nt = st->n_touched;
    uint32_t sum = 0;
    for (uint32_t i = blockIdx.y; i < nt; i += gridDim.y)
        sum += (uint32_t)__popcll(inc[(size_t)touched[i] * n_pad + (size_t)p] & fresh[i]);
    if (sum) atomicSub(&gain[p], sum);
}

// out[g * 64 + b] = min(255, number of primers p with mask[p] set, not_live[p] clear where given, and bit b in
// inc[g][p]): one wave per group, lane b counts bit b.  The lanes load 64 words of the row at once and hand them round
// with readlane, so every word is read once.  c1 / cR (optional): += segments with a count of at least 1 / of at least R.
__global__ __launch_bounds__(kThreads) void k_thin_colsum(const uint64_t *inc, int n, size_t n_pad, int G,
                                                          const uint8_t *mask, const uint8_t *not_live, uint32_t R,
                                                          uint8_t *out, unsigned long long *c1, unsigned long long *cR)
{
    const int lane = threadIdx.x & 63, sh = lane & 31;
    const bool upper = lane >= 32;
    const int waves = gridDim.x * (kThreads / 64);
    for (int g = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); g < G; g += waves) {   // whole waves
        const uint64_t *row = inc + (size_t)g * n_pad;
        uint32_t c = 0;
        for (int p0 = 0; p0 < n; p0 += 64) {
            const int p = p0 + lane;
            uint64_t w = 0;
            if (p < n && mask[p] && !(not_live && not_live[p])) w = row[p];
            if (!__ballot(w != 0)) continue;   // wave-uniform
            const uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
#pragma unroll
            for (int j = 0; j < 64; ++j) {
                const uint32_t l = __builtin_amdgcn_readlane(lo, j), h = __builtin_amdgcn_readlane(hi, j);
                c += ((upper ? h : l) >> sh) & 1u;
            }
        }
        out[(size_t)g * 64 + lane] = (uint8_t)std::min(c, 255u);
        if (c1) {
            const unsigned long long a = __ballot(c >= 1u), b = __ballot(c >= R);
            if (lane == 0) {
                if (a) atomicAdd(c1, (unsigned long long)__popcll(a));
                if (b) atomicAdd(cR, (unsigned long long)__popcll(b));
            }
        }
    }
}

// need = min(R, all), cnt = min(need, cnt); cov[g] = ~(open bits of g): a thread per (group, bit), a wave per group.
// A bit past S or past the last segment reads as closed.
__global__ __launch_bounds__(kThreads) void k_thin_depth_init(const uint8_t *all, uint8_t *cnt, uint8_t *need, int G,
                                                              int S, long n_seg, uint32_t R, uint64_t *cov)
{
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    const long g = t >> 6;
    if (g >= G) return;   // whole waves: 64 threads per group
    const int b = (int)(t & 63);
    const uint32_t nd = std::min(R, (uint32_t)all[t]), c = std::min(nd, (uint32_t)cnt[t]);
    need[t] = (uint8_t)nd;
    cnt[t] = (uint8_t)c;
    const bool open = b < S && g * S + b < n_seg && c < nd;
    const unsigned long long o = __ballot(open);
    if (b == 0) cov[g] = ~(uint64_t)o;
}

// A round's pick counts once on every open segment it matches in; the segments that reach their need close:
// cov[g] |= closed, and the groups with any go on the touched list with the closed bits as their fresh word.  A
// thread per group: it alone touches the group's 64 counters.
__global__ __launch_bounds__(kThreads) void k_thin_apply_depth(const uint64_t *inc, size_t n_pad, int G, uint64_t *cov,
                                                               uint8_t *cnt, const uint8_t *need, uint32_t *touched,
                                                               uint64_t *fresh, ThinState *st)
{
    if (st->done) return;
    const long g = (long)blockIdx.x * kThreads + threadIdx.x;
    if (g >= G) return;
    const uint64_t c = cov[g];
    uint64_t w = inc[(size_t)g * n_pad + st->pick] & ~c, closed = 0;
    if (!w) return;
    while (w) {
        const int b = __ffsll((unsigned long long)w) - 1;
        w &= w - 1;
        const size_t t = (size_t)g * 64 + (size_t)b;
        const uint8_t v = (uint8_t)(cnt[t] + 1);   // cnt < need <= 255 on an open bit
        cnt[t] = v;
        if (v >= need[t]) closed |= 1ull << b;
    }
    if (!closed) return;
    cov[g] = c | closed;
    const uint32_t i = atomicAdd(&st->n_touched, 1u);
    touched[i] = (uint32_t)g;
    fresh[i] = closed;
}

#define THIN_TRY(expr)                                                              \
    do {                                                                            \
        hipError_t e__ = (expr);                                                    \
        if (e__ != hipSuccess) {                                                    \
            err = std::string("panel thin, " #expr ": ") + hipGetErrorString(e__);  \
            return MSSPE_ERR_DEVICE;                                                \
        }                                                                           \
    } while (0)

}  // namespace

int PanelThin::ensure(int slot, size_t bytes, std::string &err)
{
    if (cap_[slot] >= bytes && buf_[slot]) return MSSPE_OK;
    if (buf_[slot]) (void)hipFree(buf_[slot]);
    buf_[slot] = nullptr;
    cap_[slot] = 0;
    const hipError_t e = hipMalloc(&buf_[slot], bytes ? bytes : 16);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        buf_[slot] = nullptr;
        err = std::string("hipMalloc (panel thin): ") + hipGetErrorString(e);
        return MSSPE_ERR_DEVICE;
    }
    cap_[slot] = bytes;
    return MSSPE_OK;
}

void PanelThin::release()
{
    for (int s = 0; s < kSlots; ++s) {
        if (buf_[s]) (void)hipFree(buf_[s]);
        buf_[s] = nullptr;
        cap_[s] = 0;
    }
    for (auto &e : ev_) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    for (auto &e : ev_depth_) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

int PanelThin::matrix(int n, long n_seg, int S, size_t max_matrix_bytes, uint64_t **inc_out, std::string &err)
{
    rounds_ = groups_ = 0;
    for (auto &p : phase_us_) p = 0;
    const long G = (n_seg + S - 1) / S;
    const size_t n_pad = ((size_t)n + 63) & ~(size_t)63;
    const size_t mib = (size_t)1 << 20, matrix = (size_t)G * n_pad * sizeof(uint64_t);
    if (matrix > max_matrix_bytes) {
        err = "panel thin: the incidence matrix needs " + std::to_string((matrix + mib - 1) / mib) +
              " MB, panel_thin_matrix_max_mb is " + std::to_string(max_matrix_bytes / mib);
        return MSSPE_ERR_CAPACITY;
    }
    groups_ = G;
    int rc;
    if ((rc = ensure(kInc, matrix, err)) || (rc = ensure(kCov, sizeof(uint64_t) * (size_t)G + sizeof(ThinState), err)) ||
        (rc = ensure(kTouched, sizeof(uint32_t) * (size_t)G, err)) ||
        (rc = ensure(kNew, sizeof(uint64_t) * (size_t)G, err)) ||
        (rc = ensure(kGain, sizeof(uint32_t) * (size_t)n, err)) || (rc = ensure(kLive, (size_t)n, err)) ||
        (rc = ensure(kOrder, 2 * sizeof(uint32_t) * (size_t)n, err)) ||
        (rc = ensure(kForced, sizeof(uint32_t) * (size_t)n, err)))
        return rc;
    for (auto &e : ev_)
        if (!e && hipEventCreate(&e) != hipSuccess) {
            err = "panel thin: hipEventCreate failed";
            return MSSPE_ERR_DEVICE;
        }
    *inc_out = (uint64_t *)buf_[kInc];
    return MSSPE_OK;
}

int PanelThin::run(MismatchCoverage &cov, const SeqView &seqs, int n_seq, size_t seq_len, const msspe_kmer_opt &opt,
                   int max_mismatches, int exact_3p, int min_gain, const uint64_t *fwd_words, int n_fwd,
                   const uint64_t *rev_words, int n_rev, const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out,
                   uint32_t *gain_out, int *n_picked_out, uint8_t *covered_out, long long *covered_all_out,
                   long long *covered_kept_out, size_t max_matrix_bytes, int n_cu, hipStream_t stream,
                   std::string &err, const PanelWeights *wts, const PanelCosts *cst)
{
    rounds_ = groups_ = 0;
    for (auto &p : phase_us_) p = 0;
    *n_picked_out = 0;
    if (covered_all_out) *covered_all_out = 0;
    if (covered_kept_out) *covered_kept_out = 0;
    if (wts && wts->weight_all_out) *wts->weight_all_out = 0;
    if (wts && wts->weight_kept_out) *wts->weight_kept_out = 0;
    if (cst && cst->cost_all_out) *cst->cost_all_out = 0;
    if (cst && cst->cost_kept_out) *cst->cost_kept_out = 0;
    long P = 0;
    int rc = MismatchCoverage::check(n_seq, seq_len, opt, max_mismatches, exact_3p, fwd_words, n_fwd, rev_words, n_rev,
                                     &P, err);
    if (rc) return rc;
    const int n = n_fwd + n_rev;
    const long n_seg = P * n_seq;
    for (int p = 0; p < n; ++p) keep_out[p] = forced && forced[p] ? 1 : 0;
    if (covered_out) std::fill(covered_out, covered_out + n_seg, (uint8_t)0);
    if (n == 0 || n_seg == 0) return MSSPE_OK;

    uint64_t *d_inc = nullptr;
    if ((rc = matrix(n, n_seg, MismatchCoverage::group_size(opt), max_matrix_bytes, &d_inc, err))) return rc;

    // (1) the incidence matrix
    THIN_TRY(hipEventRecord(ev_[0], stream));
    if ((rc = cov.incidence(seqs, n_seq, seq_len, opt, max_mismatches, exact_3p, fwd_words, n_fwd, rev_words, n_rev,
                            d_inc, stream, err)))
        return rc;
    if ((rc = rounds(n, n_seg, MismatchCoverage::group_size(opt), min_gain, keep_out, order_out, gain_out,
                     n_picked_out, covered_out, covered_all_out, covered_kept_out, n_cu, stream, err, wts, cst)))
        return rc;
    float ms = 0.f;   // rounds() returned with the stream idle
    (void)hipEventElapsedTime(&ms, ev_[0], ev_[1]);
    phase_us_[0] = (long long)(ms * 1000.0f);
    return MSSPE_OK;
}

int PanelThin::rounds(int n, long n_seg, int S, int min_gain, uint8_t *keep_out, uint32_t *order_out,
                      uint32_t *gain_out, int *n_picked_out, uint8_t *covered_out, long long *covered_all_out,
                      long long *covered_kept_out, int n_cu, hipStream_t stream, std::string &err,
                      const PanelWeights *wts, const PanelCosts *cst)
{
    const long G = (n_seg + S - 1) / S;
    const size_t n_pad = ((size_t)n + 63) & ~(size_t)63;
    if (wts)   // the sums, the plane and the weights as given: the one slot a weighted call adds
        if (int rc = ensure(kWeight, weighted::Plane::bytes(G, n_seg), err)) return rc;
    if (cst)   // a cost per primer: the one slot a cost call adds
        if (int rc = ensure(kCost, sizeof(uint32_t) * (size_t)n, err)) return rc;
    const uint32_t *d_cost = cst ? (const uint32_t *)buf_[kCost] : nullptr;
    const weighted::Plane wp(wts ? buf_[kWeight] : nullptr, G);
    uint64_t *d_inc = (uint64_t *)buf_[kInc], *d_cov = (uint64_t *)buf_[kCov], *d_new = (uint64_t *)buf_[kNew];
    ThinState *st = (ThinState *)(d_cov + G);   // behind the covered words: 8-byte aligned
    uint32_t *d_touched = (uint32_t *)buf_[kTouched], *d_gain = (uint32_t *)buf_[kGain];
    uint32_t *d_order = (uint32_t *)buf_[kOrder], *d_gains = d_order + n, *d_forced = (uint32_t *)buf_[kForced];
    uint8_t *d_live = (uint8_t *)buf_[kLive];
    THIN_TRY(hipEventRecord(ev_[1], stream));

    // (2) forced rows, first gains
    std::vector<uint8_t> live((size_t)n);
    std::vector<uint32_t> forced_idx;
    for (int p = 0; p < n; ++p) {
        live[(size_t)p] = keep_out[p] ? 0 : 1;
        if (keep_out[p]) forced_idx.push_back((uint32_t)p);
    }
    THIN_TRY(hipMemsetAsync(d_cov, 0, sizeof(uint64_t) * (size_t)G + sizeof(ThinState), stream));
    THIN_TRY(hipMemsetAsync(d_gain, 0, sizeof(uint32_t) * (size_t)n, stream));
    THIN_TRY(hipMemcpyAsync(d_live, live.data(), (size_t)n, hipMemcpyHostToDevice, stream));
    if (cst)
        THIN_TRY(hipMemcpyAsync(buf_[kCost], cst->costs, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, stream));
    if (!forced_idx.empty()) {
        THIN_TRY(hipMemcpyAsync(d_forced, forced_idx.data(), sizeof(uint32_t) * forced_idx.size(),
                                hipMemcpyHostToDevice, stream));
        const int blocks = (int)std::max<long>(1, std::min<long>((G + 3) / 4, 8L * n_cu));
        hipLaunchKernelGGL(k_thin_forced, dim3(blocks), dim3(kThreads), 0, stream, d_inc, n_pad, (int)G, d_forced,
                           (int)forced_idx.size(), d_cov, st);
    }
    if (wts) {   // the plane is rewritten by every call: nothing of the last one's is read
        const unsigned cells = (unsigned)(((size_t)G * 64 + kThreads - 1) / kThreads);
        THIN_TRY(hipMemsetAsync(wp.sums, 0, 2 * sizeof(unsigned long long), stream));
        THIN_TRY(hipMemcpyAsync(wp.by_segment, wts->weights, sizeof(uint32_t) * (size_t)n_seg,
                                hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(weighted::k_weight_plane, dim3(cells), dim3(kThreads), 0, stream, wp.by_segment, (int)G, S,
                           n_seg, wp.wt);
        if (!forced_idx.empty())
            hipLaunchKernelGGL(weighted::k_weight_of_cover, dim3(cells), dim3(kThreads), 0, stream, d_cov, (int)G,
                               wp.wt, wp.sums + 1);
        hipLaunchKernelGGL(weighted::k_weighted_gain0<ThinState>, dim3((unsigned)((G + kChunk - 1) / kChunk)),
                           dim3(kThreads), 0, stream, d_inc, n, n_pad, (int)G, d_cov, wp.wt, d_gain, st, wp.sums);
    } else {
        hipLaunchKernelGGL(k_thin_gain0, dim3((unsigned)((G + kChunk - 1) / kChunk)), dim3(kThreads), 0, stream, d_inc,
                           n, n_pad, (int)G, d_cov, d_gain, st);
    }
    THIN_TRY(hipGetLastError());
    THIN_TRY(hipEventRecord(ev_[2], stream));

    // (3) rounds, kRoundsPerBatch per read of the state; every round but the last picks a primer, so there are at
    // most n + 1 of them
    const unsigned gx = (unsigned)((n + kThreads - 1) / kThreads);
    const unsigned gy = (unsigned)std::max<long>(1, std::min<long>(std::min<long>(G, 65535), 2048 / gx));
    const unsigned ga = (unsigned)((G + kThreads - 1) / kThreads);
    ThinState hs{};
    for (int batch = 0;; ++batch) {
        for (int b = 0; b < kRoundsPerBatch; ++b) {
            if (cst)
                hipLaunchKernelGGL(cost::k_thin_pick_cost<ThinState>, dim3(1), dim3(kThreads), 0, stream, d_gain,
                                   d_cost, d_live, n, (uint32_t)min_gain, d_order, d_gains, st);
            else
                hipLaunchKernelGGL(k_thin_pick, dim3(1), dim3(kThreads), 0, stream, d_gain, d_live, n,
                                   (uint32_t)min_gain, d_order, d_gains, st);
            hipLaunchKernelGGL(k_thin_apply, dim3(ga), dim3(kThreads), 0, stream, d_inc, n_pad, (int)G, d_cov,
                               d_touched, d_new, st);
            if (wts)
                hipLaunchKernelGGL(weighted::k_weighted_update<ThinState>, dim3(gx, gy), dim3(kThreads), 0, stream,
                                   d_inc, n, n_pad, d_touched, d_new, wp.wt, d_gain, st);
            else
                hipLaunchKernelGGL(k_thin_update, dim3(gx, gy), dim3(kThreads), 0, stream, d_inc, n, n_pad, d_touched,
                                   d_new, d_gain, st);
        }
        THIN_TRY(hipGetLastError());
        THIN_TRY(hipMemcpyAsync(&hs, st, sizeof hs, hipMemcpyDeviceToHost, stream));
        THIN_TRY(hipStreamSynchronize(stream));
        if (hs.done) break;
        if (batch + 1 >= n / kRoundsPerBatch + 2) {
            err = "panel thin: more rounds than primers";
            return MSSPE_ERR_DEVICE;
        }
    }
    THIN_TRY(hipEventRecord(ev_[3], stream));

    const int n_picked = (int)hs.n_picked;
    if (n_picked > n) {
        err = "panel thin: more picks than primers";
        return MSSPE_ERR_DEVICE;
    }
    if (n_picked) {
        THIN_TRY(hipMemcpyAsync(order_out, d_order, sizeof(uint32_t) * (size_t)n_picked, hipMemcpyDeviceToHost, stream));
        THIN_TRY(hipMemcpyAsync(gain_out, d_gains, sizeof(uint32_t) * (size_t)n_picked, hipMemcpyDeviceToHost, stream));
    }
    std::vector<uint64_t> h_cov;
    unsigned long long h_sums[2] = {};
    if (covered_out || wts) {   // weighted: the gains are weights, so the kept count comes from the words
        h_cov.resize((size_t)G);
        THIN_TRY(hipMemcpyAsync(h_cov.data(), d_cov, sizeof(uint64_t) * (size_t)G, hipMemcpyDeviceToHost, stream));
    }
    if (wts) THIN_TRY(hipMemcpyAsync(h_sums, wp.sums, sizeof h_sums, hipMemcpyDeviceToHost, stream));
    THIN_TRY(hipEventSynchronize(ev_[3]));
    THIN_TRY(hipStreamSynchronize(stream));
    for (int ph = 1; ph < 3; ++ph) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev_[ph], ev_[ph + 1]);
        phase_us_[ph] = (long long)(ms * 1000.0f);
    }
    rounds_ = hs.rounds;
    long long kept = (long long)hs.covered_forced;
    for (int i = 0; i < n_picked; ++i) {
        if (order_out[i] >= (uint32_t)n) {
            err = "panel thin: a pick outside the panel";
            return MSSPE_ERR_DEVICE;
        }
        keep_out[order_out[i]] = 1;
        kept += gain_out[i];
    }
    if (wts) {   // kept holds weights here: the forced rows' and the picks' gains
        if (wts->weight_all_out) *wts->weight_all_out = h_sums[0];
        if (wts->weight_kept_out) *wts->weight_kept_out = h_sums[1] + (uint64_t)(kept - (long long)hs.covered_forced);
        kept = 0;
        for (long g = 0; g < G; ++g) kept += __builtin_popcountll(h_cov[(size_t)g]);
    }
    if (cst) {   // the two cost sums are formed here: the costs never left the host
        uint64_t all = 0, kept_cost = 0;
        for (int p = 0; p < n; ++p) {
            all += cst->costs[p];
            if (keep_out[p]) kept_cost += cst->costs[p];
        }
        if (cst->cost_all_out) *cst->cost_all_out = all;
        if (cst->cost_kept_out) *cst->cost_kept_out = kept_cost;
    }
    *n_picked_out = n_picked;
    if (covered_all_out) *covered_all_out = (long long)hs.covered_all;
    if (covered_kept_out) *covered_kept_out = kept;
    if (covered_out)
        for (long g = 0; g < G; ++g)
            for (int b = 0; b < S && g * S + b < n_seg; ++b) covered_out[g * S + b] = (uint8_t)((h_cov[(size_t)g] >> b) & 1ull);
    return MSSPE_OK;
}

int PanelThin::shadows(const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                       const uint8_t *forced, uint8_t *shadow_out)
{
    std::vector<int> idx;
    int count = 0;
    for (int dir = 0; dir < 2; ++dir) {   // a forward word that equals a reverse word is no duplicate
        const uint64_t *words = dir ? rev_words : fwd_words;
        const int base = dir ? n_fwd : 0, m = dir ? n_rev : n_fwd;
        idx.resize((size_t)m);
        for (int i = 0; i < m; ++i) idx[(size_t)i] = i;
        // by word, a forced primer before an unforced one, then by index: a run's first entry is its representative
        std::sort(idx.begin(), idx.end(), [&](int a, int b) {
            if (words[a] != words[b]) return words[a] < words[b];
            const bool fa = forced && forced[base + a], fb = forced && forced[base + b];
            if (fa != fb) return fa;
            return a < b;
        });
        for (int i = 0; i < m; ++i) {
            const bool dup = i && words[idx[(size_t)i]] == words[idx[(size_t)i - 1]];
            shadow_out[base + idx[(size_t)i]] = dup ? 1 : 0;
            count += dup;
        }
    }
    return count;
}

int PanelThin::run_depth(MismatchCoverage &cov, const SeqView &seqs, int n_seq, size_t seq_len,
                         const msspe_kmer_opt &opt, int max_mismatches, int exact_3p, int min_gain, int depth,
                         const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
                         const uint8_t *forced, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                         int *n_picked_out, uint8_t *depth_all_out, uint8_t *depth_kept_out, long long *counts_out,
                         size_t max_matrix_bytes, int n_cu, hipStream_t stream, std::string &err)
{
    rounds_ = groups_ = shadows_ = colsum_us_ = 0;
    for (auto &p : phase_us_) p = 0;
    *n_picked_out = 0;
    if (counts_out) std::fill(counts_out, counts_out + 4, 0LL);
    long P = 0;
    int rc = MismatchCoverage::check(n_seq, seq_len, opt, max_mismatches, exact_3p, fwd_words, n_fwd, rev_words, n_rev,
                                     &P, err);
    if (rc) return rc;
    const int n = n_fwd + n_rev;
    const long n_seg = P * n_seq;
    for (int p = 0; p < n; ++p) keep_out[p] = forced && forced[p] ? 1 : 0;
    if (depth_all_out) std::fill(depth_all_out, depth_all_out + n_seg, (uint8_t)0);
    if (depth_kept_out) std::fill(depth_kept_out, depth_kept_out + n_seg, (uint8_t)0);
    if (n == 0 || n_seg == 0) return MSSPE_OK;

    uint64_t *d_inc = nullptr;
    if ((rc = matrix(n, n_seg, MismatchCoverage::group_size(opt), max_matrix_bytes, &d_inc, err))) return rc;
    std::vector<uint8_t> shadow((size_t)n);
    (void)shadows(fwd_words, n_fwd, rev_words, n_rev, forced, shadow.data());
    THIN_TRY(hipEventRecord(ev_[0], stream));
    if ((rc = cov.incidence(seqs, n_seq, seq_len, opt, max_mismatches, exact_3p, fwd_words, n_fwd, rev_words, n_rev,
                            d_inc, stream, err)))
        return rc;
    if ((rc = rounds_depth(n, n_seg, MismatchCoverage::group_size(opt), min_gain, depth, shadow.data(), keep_out,
                           order_out, gain_out, n_picked_out, depth_all_out, depth_kept_out, counts_out, n_cu, stream,
                           err)))
        return rc;
    float ms = 0.f;   // rounds_depth() returned with the stream idle
    (void)hipEventElapsedTime(&ms, ev_[0], ev_[1]);
    phase_us_[0] = (long long)(ms * 1000.0f);
    return MSSPE_OK;
}

void PanelThin::colsum(const uint64_t *inc, int n, long G, const uint8_t *mask, uint32_t R, uint8_t *out,
                       unsigned long long *c1, unsigned long long *cR, int n_cu, hipStream_t stream)
{
    const size_t n_pad = ((size_t)n + 63) & ~(size_t)63;
    const int blocks = (int)std::max<long>(1, std::min<long>((G + 3) / 4, 8L * n_cu));
    hipLaunchKernelGGL(k_thin_colsum, dim3(blocks), dim3(kThreads), 0, stream, inc, n, n_pad, (int)G, mask,
                       (const uint8_t *)nullptr, R, out, c1, cR);
}

int PanelThin::rounds_depth(int n, long n_seg, int S, int min_gain, int depth, const uint8_t *shadow,
                            uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                            uint8_t *depth_all_out, uint8_t *depth_kept_out, long long *counts_out, int n_cu,
                            hipStream_t stream, std::string &err)
{
    const long G = (n_seg + S - 1) / S;
    const size_t n_pad = ((size_t)n + 63) & ~(size_t)63, cells = (size_t)G * 64;
    shadows_ = colsum_us_ = 0;
    // the four counts and the depth planes all, kept, cnt, need (a byte per (group, bit)); two primer masks
    int rc;
    if ((rc = ensure(kDepth, 4 * cells + 4 * sizeof(unsigned long long), err)) ||
        (rc = ensure(kMask, 2 * (size_t)n, err)))
        return rc;
    for (auto &e : ev_depth_)
        if (!e && hipEventCreate(&e) != hipSuccess) {
            err = "panel thin: hipEventCreate failed";
            return MSSPE_ERR_DEVICE;
        }
    uint64_t *d_inc = (uint64_t *)buf_[kInc], *d_cov = (uint64_t *)buf_[kCov], *d_new = (uint64_t *)buf_[kNew];
    ThinState *st = (ThinState *)(d_cov + G);
    uint32_t *d_touched = (uint32_t *)buf_[kTouched], *d_gain = (uint32_t *)buf_[kGain];
    uint32_t *d_order = (uint32_t *)buf_[kOrder], *d_gains = d_order + n;
    uint8_t *d_live = (uint8_t *)buf_[kLive];
    unsigned long long *d_counts = (unsigned long long *)buf_[kDepth];   // first: 8-byte aligned
    uint8_t *d_all = (uint8_t *)(d_counts + 4), *d_kept = d_all + cells, *d_cnt = d_kept + cells, *d_need = d_cnt + cells;
    uint8_t *d_rep = (uint8_t *)buf_[kMask], *d_frep = d_rep + n;
    THIN_TRY(hipEventRecord(ev_[1], stream));

    // (2) the representatives' and the forced representatives' column sums, needs, first closed words, first gains
    std::vector<uint8_t> masks(2 * (size_t)n), live((size_t)n);
    bool any_forced = false;
    for (int p = 0; p < n; ++p) {
        const bool sh = shadow && shadow[p], f = keep_out[p] != 0;
        shadows_ += sh;
        masks[(size_t)p] = sh ? 0 : 1;
        masks[(size_t)n + (size_t)p] = !sh && f ? 1 : 0;
        any_forced |= !sh && f;
        live[(size_t)p] = !sh && !f ? 1 : 0;
    }
    THIN_TRY(hipMemsetAsync(st, 0, sizeof(ThinState), stream));
    THIN_TRY(hipMemsetAsync(d_counts, 0, 4 * sizeof(unsigned long long), stream));
    THIN_TRY(hipMemsetAsync(d_gain, 0, sizeof(uint32_t) * (size_t)n, stream));
    THIN_TRY(hipMemcpyAsync(d_live, live.data(), (size_t)n, hipMemcpyHostToDevice, stream));
    THIN_TRY(hipMemcpyAsync(d_rep, masks.data(), 2 * (size_t)n, hipMemcpyHostToDevice, stream));
    const int cs_blocks = (int)std::max<long>(1, std::min<long>((G + 3) / 4, 8L * n_cu));
    hipLaunchKernelGGL(k_thin_colsum, dim3(cs_blocks), dim3(kThreads), 0, stream, d_inc, n, n_pad, (int)G, d_rep,
                       (const uint8_t *)nullptr, (uint32_t)depth, d_all, d_counts + 0, d_counts + 2);
    if (any_forced)
        hipLaunchKernelGGL(k_thin_colsum, dim3(cs_blocks), dim3(kThreads), 0, stream, d_inc, n, n_pad, (int)G, d_frep,
                           (const uint8_t *)nullptr, (uint32_t)depth, d_cnt, (unsigned long long *)nullptr,
                           (unsigned long long *)nullptr);
    else
        THIN_TRY(hipMemsetAsync(d_cnt, 0, cells, stream));
    hipLaunchKernelGGL(k_thin_depth_init, dim3((unsigned)((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                       d_all, d_cnt, d_need, (int)G, S, n_seg, (uint32_t)depth, d_cov);
    THIN_TRY(hipGetLastError());
    THIN_TRY(hipEventRecord(ev_depth_[0], stream));
    hipLaunchKernelGGL(k_thin_gain0, dim3((unsigned)((G + kChunk - 1) / kChunk)), dim3(kThreads), 0, stream, d_inc, n,
                       n_pad, (int)G, d_cov, d_gain, st);
    THIN_TRY(hipGetLastError());
    THIN_TRY(hipEventRecord(ev_[2], stream));

    // (3) the rounds, by the protocol of rounds()
    const unsigned gx = (unsigned)((n + kThreads - 1) / kThreads);
    const unsigned gy = (unsigned)std::max<long>(1, std::min<long>(std::min<long>(G, 65535), 2048 / gx));
    const unsigned ga = (unsigned)((G + kThreads - 1) / kThreads);
    ThinState hs{};
    for (int batch = 0;; ++batch) {
        for (int b = 0; b < kRoundsPerBatch; ++b) {
            hipLaunchKernelGGL(k_thin_pick, dim3(1), dim3(kThreads), 0, stream, d_gain, d_live, n, (uint32_t)min_gain,
                               d_order, d_gains, st);
            hipLaunchKernelGGL(k_thin_apply_depth, dim3(ga), dim3(kThreads), 0, stream, d_inc, n_pad, (int)G, d_cov,
                               d_cnt, d_need, d_touched, d_new, st);
            hipLaunchKernelGGL(k_thin_update, dim3(gx, gy), dim3(kThreads), 0, stream, d_inc, n, n_pad, d_touched,
                               d_new, d_gain, st);
        }
        THIN_TRY(hipGetLastError());
        THIN_TRY(hipMemcpyAsync(&hs, st, sizeof hs, hipMemcpyDeviceToHost, stream));
        THIN_TRY(hipStreamSynchronize(stream));
        if (hs.done) break;
        if (batch + 1 >= n / kRoundsPerBatch + 2) {
            err = "panel thin: more rounds than primers";
            return MSSPE_ERR_DEVICE;
        }
    }
    THIN_TRY(hipEventRecord(ev_[3], stream));

    // (4) the kept representatives' column sums: a representative that is not live is forced or picked
    hipLaunchKernelGGL(k_thin_colsum, dim3(cs_blocks), dim3(kThreads), 0, stream, d_inc, n, n_pad, (int)G, d_rep,
                       (const uint8_t *)d_live, (uint32_t)depth, d_kept, d_counts + 1, d_counts + 3);
    THIN_TRY(hipGetLastError());
    THIN_TRY(hipEventRecord(ev_depth_[1], stream));

    const int n_picked = (int)hs.n_picked;
    if (n_picked > n) {
        err = "panel thin: more picks than primers";
        return MSSPE_ERR_DEVICE;
    }
    if (n_picked) {
        THIN_TRY(hipMemcpyAsync(order_out, d_order, sizeof(uint32_t) * (size_t)n_picked, hipMemcpyDeviceToHost, stream));
        THIN_TRY(hipMemcpyAsync(gain_out, d_gains, sizeof(uint32_t) * (size_t)n_picked, hipMemcpyDeviceToHost, stream));
    }
    unsigned long long h_counts[4] = {};
    THIN_TRY(hipMemcpyAsync(h_counts, d_counts, sizeof h_counts, hipMemcpyDeviceToHost, stream));
    std::vector<uint8_t> h_depth;
    if (depth_all_out || depth_kept_out) {
        h_depth.resize(2 * cells);   // all and kept lie side by side
        THIN_TRY(hipMemcpyAsync(h_depth.data(), d_all, 2 * cells, hipMemcpyDeviceToHost, stream));
    }
    THIN_TRY(hipStreamSynchronize(stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev_[1], ev_depth_[0]);
    float ms_kept = 0.f;
    (void)hipEventElapsedTime(&ms_kept, ev_[3], ev_depth_[1]);
    colsum_us_ = (long long)((ms + ms_kept) * 1000.0f);
    (void)hipEventElapsedTime(&ms, ev_depth_[0], ev_[2]);
    phase_us_[1] = (long long)(ms * 1000.0f);
    (void)hipEventElapsedTime(&ms, ev_[2], ev_[3]);
    phase_us_[2] = (long long)(ms * 1000.0f);
    rounds_ = hs.rounds;
    for (int i = 0; i < n_picked; ++i) {
        if (order_out[i] >= (uint32_t)n) {
            err = "panel thin: a pick outside the panel";
            return MSSPE_ERR_DEVICE;
        }
        keep_out[order_out[i]] = 1;
    }
    *n_picked_out = n_picked;
    if (counts_out)
        for (int i = 0; i < 4; ++i) counts_out[i] = (long long)h_counts[i];
    for (int plane = 0; plane < 2; ++plane) {
        uint8_t *out = plane ? depth_kept_out : depth_all_out;
        if (!out) continue;
        const uint8_t *src = h_depth.data() + (size_t)plane * cells;
        for (long g = 0; g < G; ++g)
            for (int b = 0; b < S && g * S + b < n_seg; ++b) out[g * S + b] = src[(size_t)g * 64 + (size_t)b];
    }
    return MSSPE_OK;
}

}  // namespace msspe
