// panel_select.hip -- a conflict-free panel selected by coverage (engine extension).
//
// The vertex cover deletes primers by conflict degree and never looks at coverage; the thinning that follows cannot
// bring a segment back.  The rule here joins the two: the greedy set cover of panel_thin.hip in which a pick bars its
// conflict neighbours -- with more than one tube, from its own tube only.
//
//   Graph: the cover's.  S = B | B^T, padding bits ignored, with drop_self_pairs the diagonal and the reverse-
//     complement partners cleared first.  p is self-conflicting when S[p][p] is still set.
//   State: covered = the OR of the forced rows.  mask[p] = the tubes barred to p: every neighbour of a forced primer
//     starts with all T bits set (the panel is in every tube), everyone else at 0.  p is live when it is not forced,
//     not picked, not self-conflicting, and mask[p] lacks at least one of the low T bits.
//   Rounds: gain(p) = |row(p) & ~covered| over the live p.  The greatest gain wins, ties to the lowest index; below
//     min_gain, or with nobody live, the loop ends.  Otherwise p joins the order with its gain, tube(p) = the lowest
//     tube not in mask[p], covered |= row(p), and mask[u] |= 1 << tube(p) for every u != p with S[p][u] set.
//
// Phases.  The cover's (ranks, duplicate check, partners, S; CoverStage::prepare) and the thinning's matrix, then (1)
// forced rows into cov[g], the first barring (a thread per primer reads its bit of every forced primer's row of S and
// its own diagonal bit), the first gains; (2) rounds of three launches, the thinning's three: the argmax of
// gain << 32 | ~p over the LIVE primers, which also takes the pick's tube from its mask; the apply step, whose threads
// serve a group each (the pick's new segments, cov |= new, the touched list) and a primer each (thread u reads bit u
// of row S[pick] and ORs the tube's bit into its own word: no atomics); and gain[p] -= popc(inc[g][p] & new[g]) over
// the touched groups.  gain[p] == |I[p] & ~cov| holds for every p after every round, live or not, so a primer that
// is barred costs nothing to keep up to date.  Sixteen rounds are enqueued per batch behind a device word; after the
// round that stops the launches return at once, and the host reads one word per batch.
//
// Depth (msspe_panel_select_depth*).  The same rounds run in layers r = 1 .. L.  Two byte planes, a
// cell per (group, bit), hold depth_all (the column sums of inc over all primers: PanelThin::colsum) and cnt (the kept
// primers on the segment, first the forced rows' column sums).  k_select_layer opens a layer: a segment is open while
// cnt < min(r, all), cov[g] = ~open, so that the gain, pick and update kernels above run unchanged with cov read as
// "closed".  k_select_apply_depth is the apply step of a layered round: the pick counts on EVERY segment of its row,
// open or not, the open ones that reach min(r, all) close, and the barring is k_select_apply's.  Picks, masks and
// cnt carry over from layer to layer; between layers the host clears `done` and the gains.
//
// Weights (msspe_panel_select_weighted*).  gain(p) is the sum of a weight per segment over the
// uncovered segments of row p: the first gains and the update run in their weighted instances (panel_weighted.hpp);
// forced, first barring, pick and apply are the kernels above, unchanged.
//
// Costs (msspe_panel_select_cost*).  A round keeps the live primer of greatest gain / cost: the pick
// runs in its cost instance (panel_cost.hpp) over a cost per primer; every other kernel of the round is the one above,
// weighted or not.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/msspe_hip.h"
#include "panel_cost.hpp"
#include "panel_select.hpp"
#include "panel_thin.hpp"
#include "panel_weighted.hpp"

namespace msspe {

namespace {

constexpr int kRoundsPerBatch = 16;   // rounds enqueued between two reads of the "done" word
constexpr int kThreads = 256;
constexpr int kChunk = 32;            // groups per block of the first gains
constexpr uint8_t kLive = 1;          // flags[p]: not forced, not picked, not self-conflicting
constexpr uint8_t kSelf = 2;          // flags[p]: S[p][p] is set

struct SelectState {
    uint32_t done;        // 1: a round found no live gain of min_gain or more (the launches that follow return at once)
    uint32_t rounds;      // rounds that ran: the picks and the one that stopped
    uint32_t n_picked;
    uint32_t pick;        // of the current round
    uint32_t tube;        // of the current pick
    uint32_t used;        // highest tube in use + 1
    uint32_t n_touched;   // groups in which the current pick covers something new
    uint32_t deeper;      // depth runs: r + 1 once layer r has seen a segment with more than r primers; else unused
    unsigned long long covered_all;      // |OR of all I[p]|
    unsigned long long covered_forced;   // |OR of the forced I[p]|
};

enum { kPool, kCov, kTouched, kNew, kGain, kMask, kBytes, kOrder, kForced, kDepth, kPrimerMask, kWeight, kCost };   // PanelSelect::buf_

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
__global__ __launch_bounds__(kThreads) void k_select_forced(const uint64_t *inc, size_t n_pad, int G,
                                                            const uint32_t *forced, int n_forced, uint64_t *cov,
                                                            SelectState *st)
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

// The first barring, a thread per primer u: mask[u] = all T tubes when u is the neighbour of a forced primer (bit u of
// that primer's row of S; a wave reads one word of the row), else 0; a set diagonal bit takes u out of the live set
// for good.  flags[u] holds kLive for the unforced primers on entry.
__global__ __launch_bounds__(kThreads) void k_select_bar0(const uint64_t *S, int n, int W, const uint32_t *forced,
                                                          int n_forced, uint64_t tubes_mask, uint64_t *mask,
                                                          uint8_t *flags)
{
    const int u = blockIdx.x * kThreads + threadIdx.x;
    if (u >= n) return;
    const int w = u >> 6, b = u & 63;
    uint64_t m = 0;
    for (int i = 0; i < n_forced; ++i) {
        const uint32_t f = forced[i];
        if (f != (uint32_t)u && ((S[(size_t)f * W + w] >> b) & 1ull)) m = tubes_mask;
    }
    mask[u] = m;
    if ((S[(size_t)u * W + w] >> b) & 1ull) flags[u] = kSelf;
}

// gain[p] += popc(inc[g][p] & ~cov[g]) over the block's chunk of groups: one atomic per (block, primer); the OR of a
// group's words over all primers is collected in LDS, and its popcount added to covered_all
__global__ __launch_bounds__(kThreads) void k_select_gain0(const uint64_t *inc, int n, size_t n_pad, int G,
                                                           const uint64_t *cov, uint32_t *gain, SelectState *st)
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

// One block: the live primer of greatest (gain, lowest index); live = its flag and a tube left in its mask.  Below
// min_gain (or nobody live) the loop is done.  The pick takes the lowest tube its mask leaves.
__global__ __launch_bounds__(kThreads) void k_select_pick(const uint32_t *gain, uint8_t *flags, const uint64_t *mask,
                                                          int n, uint32_t min_gain, uint64_t tubes_mask,
                                                          uint32_t *order, uint32_t *gains, uint8_t *tube,
                                                          SelectState *st)
{
    if (st->done) return;
    __shared__ uint64_t skey[kThreads / 64];
    const int tid = threadIdx.x;
    uint64_t key = 0;   // a live primer's key is never 0: its low half is 0xFFFFFFFF - p with p < 2^31
    for (int p = tid; p < n; p += kThreads)
        if ((flags[p] & kLive) && (~mask[p] & tubes_mask))
            key = std::max(key, (uint64_t)gain[p] << 32 | (uint64_t)(0xFFFFFFFFu - (uint32_t)p));
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
            const uint32_t t = (uint32_t)__builtin_ctzll(~mask[p] & tubes_mask);   // nonzero: p is live
            order[i] = p;
            gains[i] = g;
            flags[p] = 0;
            tube[p] = (uint8_t)t;
            st->n_picked = i + 1;
            st->pick = p;
            st->tube = t;
            if (t + 1 > st->used) st->used = t + 1;
            st->n_touched = 0;
        }
    }
}

// Thread i serves group i and primer i.  Group: new[g] = inc[g][pick] & ~cov[g]; cov[g] |= new[g]; the groups with any
// go on the touched list (at most G entries).  Primer: a neighbour of the pick gets the pick's tube into its mask --
// every thread writes its own word, and the pick's own is left alone.
__global__ __launch_bounds__(kThreads) void k_select_apply(const uint64_t *inc, size_t n_pad, int G, uint64_t *cov,
                                                           uint32_t *touched, uint64_t *fresh, const uint64_t *S,
                                                           int n, int W, uint64_t *mask, SelectState *st)
{
    if (st->done) return;
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t pick = st->pick;
    if (i < G) {
        const uint64_t c = cov[i], w = inc[(size_t)i * n_pad + pick] & ~c;
        if (w) {
            cov[i] = c | w;
            const uint32_t at = atomicAdd(&st->n_touched, 1u);
            touched[at] = (uint32_t)i;
            fresh[at] = w;
        }
    }
    if (i < n && (uint32_t)i != pick && ((S[(size_t)pick * W + (i >> 6)] >> (i & 63)) & 1ull))
        mask[i] |= 1ull << st->tube;
}

// gain[p] -= popc(inc[g][p] & new[g]) over the touched groups (blockIdx.y strides over the list), lanes over p
__global__ __launch_bounds__(kThreads) void k_select_update(const uint64_t *inc, int n, size_t n_pad,
                                                            const uint32_t *touched, const uint64_t *fresh,
                                                            uint32_t *gain, const SelectState *st)
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

// Layer r opens, a thread per (group, bit), a wave per group: a segment is open while cnt < min(r, all); cov[g] =
// ~(open bits), so a bit past S or past the last segment reads as closed.  A group that has a segment with more than r
// primers says that a layer r + 1 exists (deeper only grows, so nobody has to clear it).
__global__ __launch_bounds__(kThreads) void k_select_layer(const uint8_t *all, const uint8_t *cnt, int G, int S,
                                                           long n_seg, uint32_t r, uint64_t *cov, SelectState *st)
{
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    const long g = t >> 6;
    if (g >= G) return;   // whole waves: 64 threads per group
    const int b = (int)(t & 63);
    const uint32_t a = all[t], c = cnt[t];
    const bool open = b < S && g * S + b < n_seg && c < std::min(r, a);
    const unsigned long long o = __ballot(open), more = __ballot(a > r);
    if (b == 0) {
        cov[g] = ~(uint64_t)o;
        if (more) atomicMax(&st->deeper, r + 1);
    }
}

// The apply step of a layered round; thread i serves group i and primer i.  Group: the pick counts once on every
// segment of its row, open or not, saturating at 255; the open ones that reach min(r, all) close: cov[g] |= closed,
// and the groups with any go on the touched list with the closed bits as their fresh word.  A thread alone touches its
// group's 64 counters.  Primer: the barring of k_select_apply.
__global__ __launch_bounds__(kThreads) void k_select_apply_depth(const uint64_t *inc, size_t n_pad, int G,
                                                                 uint64_t *cov, uint8_t *cnt, const uint8_t *all,
                                                                 uint32_t r, uint32_t *touched, uint64_t *fresh,
                                                                 const uint64_t *S, int n, int W, uint64_t *mask,
                                                                 SelectState *st)
{
    if (st->done) return;
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t pick = st->pick;
    if (i < G) {
        const uint64_t c = cov[i];
        uint64_t w = inc[(size_t)i * n_pad + pick], closed = 0;
        while (w) {
            const int b = __ffsll((unsigned long long)w) - 1;
            w &= w - 1;
            const size_t t = (size_t)i * 64 + (size_t)b;   // b < 64: inside the group's cells
            const uint32_t v = std::min((uint32_t)cnt[t] + 1u, 255u);
            cnt[t] = (uint8_t)v;
            if (!((c >> b) & 1ull) && v >= std::min(r, (uint32_t)all[t])) closed |= 1ull << b;
        }
        if (closed) {
            cov[i] = c | closed;
            const uint32_t at = atomicAdd(&st->n_touched, 1u);
            touched[at] = (uint32_t)i;
            fresh[at] = closed;
        }
    }
    if (i < n && (uint32_t)i != pick && ((S[(size_t)pick * W + (i >> 6)] >> (i & 63)) & 1ull))
        mask[i] |= 1ull << st->tube;
}

#define SELECT_TRY(expr)                                                              \
    do {                                                                              \
        hipError_t e__ = (expr);                                                      \
        if (e__ != hipSuccess) {                                                      \
            err = std::string("panel select, " #expr ": ") + hipGetErrorString(e__);  \
            return MSSPE_ERR_DEVICE;                                                  \
        }                                                                             \
    } while (0)

}  // namespace

int PanelSelect::ensure(int slot, size_t bytes, std::string &err)
{
    if (cap_[slot] >= bytes && buf_[slot]) return MSSPE_OK;
    if (buf_[slot]) (void)hipFree(buf_[slot]);
    buf_[slot] = nullptr;
    cap_[slot] = 0;
    const hipError_t e = hipMalloc(&buf_[slot], bytes ? bytes : 16);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        buf_[slot] = nullptr;
        err = std::string("hipMalloc (panel select): ") + hipGetErrorString(e);
        return MSSPE_ERR_DEVICE;
    }
    cap_[slot] = bytes;
    return MSSPE_OK;
}

void PanelSelect::release()
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
    for (auto &e : ev_layer_) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

int PanelSelect::begin(int n, long n_seg, int S, const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words,
                       int n_rev, const uint64_t **d_pool_out, hipStream_t stream, std::string &err)
{
    reset_stats();
    const long G = (n_seg + S - 1) / S;
    int rc;
    if ((rc = ensure(kPool, sizeof(uint64_t) * (size_t)n, err)) ||
        (rc = ensure(kCov, sizeof(uint64_t) * (size_t)G + sizeof(SelectState), err)) ||
        (rc = ensure(kTouched, sizeof(uint32_t) * (size_t)G, err)) ||
        (rc = ensure(kNew, sizeof(uint64_t) * (size_t)G, err)) ||
        (rc = ensure(kGain, sizeof(uint32_t) * (size_t)n, err)) ||
        (rc = ensure(kMask, sizeof(uint64_t) * (size_t)n, err)) || (rc = ensure(kBytes, 2 * (size_t)n, err)) ||
        (rc = ensure(kOrder, 2 * sizeof(uint32_t) * (size_t)n, err)) ||
        (rc = ensure(kForced, sizeof(uint32_t) * (size_t)n, err)))
        return rc;
    for (auto &e : ev_)
        if (!e && hipEventCreate(&e) != hipSuccess) {
            err = "panel select: hipEventCreate failed";
            return MSSPE_ERR_DEVICE;
        }
    uint64_t *d_pool = (uint64_t *)buf_[kPool];
    if (n_fwd)
        SELECT_TRY(hipMemcpyAsync(d_pool, fwd_words, sizeof(uint64_t) * (size_t)n_fwd, hipMemcpyHostToDevice, stream));
    if (n_rev)
        SELECT_TRY(hipMemcpyAsync(d_pool + n_fwd, rev_words, sizeof(uint64_t) * (size_t)n_rev, hipMemcpyHostToDevice,
                                  stream));
    *d_pool_out = d_pool;
    return MSSPE_OK;
}

int PanelSelect::rounds(const uint64_t *d_inc, const uint64_t *d_sym, int n, long n_seg, int S, int min_gain,
                        int max_tubes, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                        uint8_t *tube_out, uint8_t *barred_out, uint8_t *covered_out, long long *covered_all_out,
                        long long *covered_kept_out, int *n_tubes_used_out, int n_cu, hipStream_t stream,
                        std::string &err, const PanelWeights *wts, const PanelCosts *cst)
{
    const long G = (n_seg + S - 1) / S;
    const int W = (n + 63) / 64;
    const size_t n_pad = ((size_t)n + 63) & ~(size_t)63;
    if (wts)   // the sums, the plane and the weights as given: the one slot a weighted call adds
        if (int rc = ensure(kWeight, weighted::Plane::bytes(G, n_seg), err)) return rc;
    if (cst)   // a cost per primer: the one slot a cost call adds
        if (int rc = ensure(kCost, sizeof(uint32_t) * (size_t)n, err)) return rc;
    const uint32_t *d_cost = cst ? (const uint32_t *)buf_[kCost] : nullptr;
    if (cst && cst->cost_all_out) *cst->cost_all_out = 0;
    if (cst && cst->cost_kept_out) *cst->cost_kept_out = 0;
    const weighted::Plane wp(wts ? buf_[kWeight] : nullptr, G);
    const uint64_t tubes_mask = max_tubes >= 64 ? ~0ull : (1ull << max_tubes) - 1;
    uint64_t *d_cov = (uint64_t *)buf_[kCov], *d_new = (uint64_t *)buf_[kNew], *d_mask = (uint64_t *)buf_[kMask];
    SelectState *st = (SelectState *)(d_cov + G);   // behind the covered words: 8-byte aligned
    uint32_t *d_touched = (uint32_t *)buf_[kTouched], *d_gain = (uint32_t *)buf_[kGain];
    uint32_t *d_order = (uint32_t *)buf_[kOrder], *d_gains = d_order + n, *d_forced = (uint32_t *)buf_[kForced];
    uint8_t *d_flags = (uint8_t *)buf_[kBytes], *d_tube = d_flags + n;
    SELECT_TRY(hipEventRecord(ev_[0], stream));

    // (1) forced rows, first barring, first gains
    std::vector<uint8_t> flags((size_t)n);
    std::vector<uint32_t> forced_idx;
    for (int p = 0; p < n; ++p) {
        flags[(size_t)p] = keep_out[p] ? 0 : kLive;
        if (keep_out[p]) forced_idx.push_back((uint32_t)p);
    }
    SELECT_TRY(hipMemsetAsync(d_cov, 0, sizeof(uint64_t) * (size_t)G + sizeof(SelectState), stream));
    SELECT_TRY(hipMemsetAsync(d_gain, 0, sizeof(uint32_t) * (size_t)n, stream));
    SELECT_TRY(hipMemsetAsync(d_tube, MSSPE_TUBE_NONE, (size_t)n, stream));
    SELECT_TRY(hipMemcpyAsync(d_flags, flags.data(), (size_t)n, hipMemcpyHostToDevice, stream));
    if (cst)
        SELECT_TRY(hipMemcpyAsync(buf_[kCost], cst->costs, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, stream));
    const unsigned gx = (unsigned)((n + kThreads - 1) / kThreads);
    if (!forced_idx.empty()) {
        SELECT_TRY(hipMemcpyAsync(d_forced, forced_idx.data(), sizeof(uint32_t) * forced_idx.size(),
                                  hipMemcpyHostToDevice, stream));
        const int blocks = (int)std::max<long>(1, std::min<long>((G + 3) / 4, 8L * n_cu));
        hipLaunchKernelGGL(k_select_forced, dim3(blocks), dim3(kThreads), 0, stream, d_inc, n_pad, (int)G, d_forced,
                           (int)forced_idx.size(), d_cov, st);
    }
    hipLaunchKernelGGL(k_select_bar0, dim3(gx), dim3(kThreads), 0, stream, d_sym, n, W, d_forced,
                       (int)forced_idx.size(), tubes_mask, d_mask, d_flags);
    if (wts) {   // the plane is rewritten by every call: nothing of the last one's is read
        const unsigned cells = (unsigned)(((size_t)G * 64 + kThreads - 1) / kThreads);
        SELECT_TRY(hipMemsetAsync(wp.sums, 0, 2 * sizeof(unsigned long long), stream));
        SELECT_TRY(hipMemcpyAsync(wp.by_segment, wts->weights, sizeof(uint32_t) * (size_t)n_seg, hipMemcpyHostToDevice,
                                  stream));
        hipLaunchKernelGGL(weighted::k_weight_plane, dim3(cells), dim3(kThreads), 0, stream, wp.by_segment, (int)G, S,
                           n_seg, wp.wt);
        if (!forced_idx.empty())
            hipLaunchKernelGGL(weighted::k_weight_of_cover, dim3(cells), dim3(kThreads), 0, stream, d_cov, (int)G,
                               wp.wt, wp.sums + 1);
        hipLaunchKernelGGL(weighted::k_weighted_gain0<SelectState>, dim3((unsigned)((G + kChunk - 1) / kChunk)),
                           dim3(kThreads), 0, stream, d_inc, n, n_pad, (int)G, d_cov, wp.wt, d_gain, st, wp.sums);
    } else {
        hipLaunchKernelGGL(k_select_gain0, dim3((unsigned)((G + kChunk - 1) / kChunk)), dim3(kThreads), 0, stream,
                           d_inc, n, n_pad, (int)G, d_cov, d_gain, st);
    }
    SELECT_TRY(hipGetLastError());
    SELECT_TRY(hipEventRecord(ev_[1], stream));

    // (2) rounds, kRoundsPerBatch per read of the state; every round but the last picks a primer, so there are at
    // most n + 1 of them
    const unsigned gy = (unsigned)std::max<long>(1, std::min<long>(std::min<long>(G, 65535), 2048 / gx));
    const unsigned ga = (unsigned)((std::max<long>(G, n) + kThreads - 1) / kThreads);
    SelectState hs{};
    for (int batch = 0;; ++batch) {
        for (int b = 0; b < kRoundsPerBatch; ++b) {
            if (cst)
                hipLaunchKernelGGL(cost::k_select_pick_cost<SelectState>, dim3(1), dim3(kThreads), 0, stream, d_gain,
                                   d_cost, d_flags, kLive, d_mask, n, (uint32_t)min_gain, tubes_mask, d_order, d_gains,
                                   d_tube, st);
            else
                hipLaunchKernelGGL(k_select_pick, dim3(1), dim3(kThreads), 0, stream, d_gain, d_flags, d_mask, n,
                                   (uint32_t)min_gain, tubes_mask, d_order, d_gains, d_tube, st);
            hipLaunchKernelGGL(k_select_apply, dim3(ga), dim3(kThreads), 0, stream, d_inc, n_pad, (int)G, d_cov,
                               d_touched, d_new, d_sym, n, W, d_mask, st);
            if (wts)
                hipLaunchKernelGGL(weighted::k_weighted_update<SelectState>, dim3(gx, gy), dim3(kThreads), 0, stream,
                                   d_inc, n, n_pad, d_touched, d_new, wp.wt, d_gain, st);
            else
                hipLaunchKernelGGL(k_select_update, dim3(gx, gy), dim3(kThreads), 0, stream, d_inc, n, n_pad,
                                   d_touched, d_new, d_gain, st);
        }
        SELECT_TRY(hipGetLastError());
        SELECT_TRY(hipMemcpyAsync(&hs, st, sizeof hs, hipMemcpyDeviceToHost, stream));
        SELECT_TRY(hipStreamSynchronize(stream));
        if (hs.done) break;
        if (batch + 1 >= n / kRoundsPerBatch + 2) {
            err = "panel select: more rounds than primers";
            return MSSPE_ERR_DEVICE;
        }
    }
    SELECT_TRY(hipEventRecord(ev_[2], stream));

    const int n_picked = (int)hs.n_picked;
    if (n_picked > n || hs.used > (uint32_t)max_tubes) {
        err = "panel select: more picks than primers, or a tube past max_tubes";
        return MSSPE_ERR_DEVICE;
    }
    if (n_picked) {
        SELECT_TRY(hipMemcpyAsync(order_out, d_order, sizeof(uint32_t) * (size_t)n_picked, hipMemcpyDeviceToHost, stream));
        SELECT_TRY(hipMemcpyAsync(gain_out, d_gains, sizeof(uint32_t) * (size_t)n_picked, hipMemcpyDeviceToHost, stream));
    }
    std::vector<uint64_t> h_cov, h_mask((size_t)n);
    SELECT_TRY(hipMemcpyAsync(tube_out, d_tube, (size_t)n, hipMemcpyDeviceToHost, stream));
    SELECT_TRY(hipMemcpyAsync(flags.data(), d_flags, (size_t)n, hipMemcpyDeviceToHost, stream));
    SELECT_TRY(hipMemcpyAsync(h_mask.data(), d_mask, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
    unsigned long long h_sums[2] = {};
    if (covered_out || wts) {   // weighted: the gains are weights, so the kept count comes from the words
        h_cov.resize((size_t)G);
        SELECT_TRY(hipMemcpyAsync(h_cov.data(), d_cov, sizeof(uint64_t) * (size_t)G, hipMemcpyDeviceToHost, stream));
    }
    if (wts) SELECT_TRY(hipMemcpyAsync(h_sums, wp.sums, sizeof h_sums, hipMemcpyDeviceToHost, stream));
    SELECT_TRY(hipEventSynchronize(ev_[2]));
    SELECT_TRY(hipStreamSynchronize(stream));
    for (int ph = 0; ph < 2; ++ph) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev_[ph], ev_[ph + 1]);
        phase_us_[ph] = (long long)(ms * 1000.0f);
    }
    rounds_ = hs.rounds;
    tubes_ = hs.used;
    long long kept = (long long)hs.covered_forced;
    for (int i = 0; i < n_picked; ++i) {
        if (order_out[i] >= (uint32_t)n) {
            err = "panel select: a pick outside the panel";
            return MSSPE_ERR_DEVICE;
        }
        keep_out[order_out[i]] = 1;
        kept += gain_out[i];
    }
    for (int p = 0; p < n; ++p) {
        const bool barred = !keep_out[p] && ((flags[(size_t)p] & kSelf) || (h_mask[(size_t)p] & tubes_mask) == tubes_mask);
        barred_ += barred;
        if (barred_out) barred_out[p] = barred ? 1 : 0;
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
    if (n_tubes_used_out) *n_tubes_used_out = (int)hs.used;
    if (covered_all_out) *covered_all_out = (long long)hs.covered_all;
    if (covered_kept_out) *covered_kept_out = kept;
    if (covered_out)
        for (long g = 0; g < G; ++g)
            for (int b = 0; b < S && g * S + b < n_seg; ++b) covered_out[g * S + b] = (uint8_t)((h_cov[(size_t)g] >> b) & 1ull);
    return MSSPE_OK;
}

int PanelSelect::rounds_depth(const uint64_t *d_inc, const uint64_t *d_sym, int n, long n_seg, int S, int min_gain,
                              int max_tubes, int depth, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out,
                              int *n_picked_out, uint8_t *tube_out, uint8_t *barred_out, int *n_tubes_used_out,
                              uint8_t *pick_layer_out, uint8_t *depth_all_out, uint8_t *depth_kept_out,
                              long long *counts_out, int n_cu, hipStream_t stream, std::string &err)
{
    const long G = (n_seg + S - 1) / S;
    const int W = (n + 63) / 64;
    const size_t n_pad = ((size_t)n + 63) & ~(size_t)63, cells = (size_t)G * 64;
    const uint64_t tubes_mask = max_tubes >= 64 ? ~0ull : (1ull << max_tubes) - 1;
    // the two counts of depth_all and the planes all, cnt (a byte per (group, bit)); two primer masks: all, forced
    int rc;
    if ((rc = ensure(kDepth, 2 * sizeof(unsigned long long) + 2 * cells, err)) ||
        (rc = ensure(kPrimerMask, 2 * (size_t)n, err)))
        return rc;
    for (auto &e : ev_layer_)
        if (!e && hipEventCreate(&e) != hipSuccess) {
            err = "panel select: hipEventCreate failed";
            return MSSPE_ERR_DEVICE;
        }
    uint64_t *d_cov = (uint64_t *)buf_[kCov], *d_new = (uint64_t *)buf_[kNew], *d_mask = (uint64_t *)buf_[kMask];
    SelectState *st = (SelectState *)(d_cov + G);
    uint32_t *d_touched = (uint32_t *)buf_[kTouched], *d_gain = (uint32_t *)buf_[kGain];
    uint32_t *d_order = (uint32_t *)buf_[kOrder], *d_gains = d_order + n, *d_forced = (uint32_t *)buf_[kForced];
    uint8_t *d_flags = (uint8_t *)buf_[kBytes], *d_tube = d_flags + n;
    unsigned long long *d_counts = (unsigned long long *)buf_[kDepth];   // first: 8-byte aligned
    uint8_t *d_all = (uint8_t *)(d_counts + 2), *d_cnt = d_all + cells;
    uint8_t *d_every = (uint8_t *)buf_[kPrimerMask], *d_isforced = d_every + n;
    SELECT_TRY(hipEventRecord(ev_[0], stream));

    // (1) the first barring and the column sums: depth_all over all primers, the first cnt over the forced ones
    std::vector<uint8_t> flags((size_t)n), masks(2 * (size_t)n);
    std::vector<uint32_t> forced_idx;
    for (int p = 0; p < n; ++p) {
        flags[(size_t)p] = keep_out[p] ? 0 : kLive;
        masks[(size_t)p] = 1;
        masks[(size_t)n + (size_t)p] = keep_out[p] ? 1 : 0;
        if (keep_out[p]) forced_idx.push_back((uint32_t)p);
    }
    SELECT_TRY(hipMemsetAsync(st, 0, sizeof(SelectState), stream));
    SELECT_TRY(hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned long long), stream));
    SELECT_TRY(hipMemsetAsync(d_tube, MSSPE_TUBE_NONE, (size_t)n, stream));
    SELECT_TRY(hipMemcpyAsync(d_flags, flags.data(), (size_t)n, hipMemcpyHostToDevice, stream));
    SELECT_TRY(hipMemcpyAsync(d_every, masks.data(), 2 * (size_t)n, hipMemcpyHostToDevice, stream));
    const unsigned gx = (unsigned)((n + kThreads - 1) / kThreads);
    if (!forced_idx.empty())
        SELECT_TRY(hipMemcpyAsync(d_forced, forced_idx.data(), sizeof(uint32_t) * forced_idx.size(),
                                  hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_select_bar0, dim3(gx), dim3(kThreads), 0, stream, d_sym, n, W, d_forced,
                       (int)forced_idx.size(), tubes_mask, d_mask, d_flags);
    SELECT_TRY(hipGetLastError());
    SELECT_TRY(hipEventRecord(ev_layer_[0], stream));
    PanelThin::colsum(d_inc, n, G, d_every, (uint32_t)depth, d_all, d_counts + 0, d_counts + 1, n_cu, stream);
    if (!forced_idx.empty())
        PanelThin::colsum(d_inc, n, G, d_isforced, (uint32_t)depth, d_cnt, nullptr, nullptr, n_cu, stream);
    else
        SELECT_TRY(hipMemsetAsync(d_cnt, 0, cells, stream));
    SELECT_TRY(hipGetLastError());

    // (2) the layers.  Each opens with its closed words and its first gains (k_select_gain0 also adds to covered_all
    // in the state, once per layer: nothing here reads it) and then runs rounds()'s batches; the round that stops a
    // layer has set `done`, which the next layer clears.  Layer r + 1 exists while r < depth and some segment has
    // more than r primers.
    const unsigned gy = (unsigned)std::max<long>(1, std::min<long>(std::min<long>(G, 65535), 2048 / gx));
    const unsigned ga = (unsigned)((std::max<long>(G, n) + kThreads - 1) / kThreads);
    SelectState hs{};
    std::vector<uint32_t> layer_end;   // picks made when layer r ended
    float layer_ms = 0.f;
    for (uint32_t r = 1;; ++r) {
        if (r > 1) {
            SELECT_TRY(hipEventRecord(ev_layer_[0], stream));
            SELECT_TRY(hipMemsetAsync(&st->done, 0, sizeof(uint32_t), stream));
        }
        SELECT_TRY(hipMemsetAsync(d_gain, 0, sizeof(uint32_t) * (size_t)n, stream));
        hipLaunchKernelGGL(k_select_layer, dim3((unsigned)((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                           stream, d_all, d_cnt, (int)G, S, n_seg, r, d_cov, st);
        hipLaunchKernelGGL(k_select_gain0, dim3((unsigned)((G + kChunk - 1) / kChunk)), dim3(kThreads), 0, stream,
                           d_inc, n, n_pad, (int)G, d_cov, d_gain, st);
        SELECT_TRY(hipGetLastError());
        SELECT_TRY(hipEventRecord(ev_layer_[1], stream));
        if (r == 1) SELECT_TRY(hipEventRecord(ev_[1], stream));
        for (int batch = 0;; ++batch) {
            for (int b = 0; b < kRoundsPerBatch; ++b) {
                hipLaunchKernelGGL(k_select_pick, dim3(1), dim3(kThreads), 0, stream, d_gain, d_flags, d_mask, n,
                                   (uint32_t)min_gain, tubes_mask, d_order, d_gains, d_tube, st);
                hipLaunchKernelGGL(k_select_apply_depth, dim3(ga), dim3(kThreads), 0, stream, d_inc, n_pad, (int)G,
                                   d_cov, d_cnt, d_all, r, d_touched, d_new, d_sym, n, W, d_mask, st);
                hipLaunchKernelGGL(k_select_update, dim3(gx, gy), dim3(kThreads), 0, stream, d_inc, n, n_pad,
                                   d_touched, d_new, d_gain, st);
            }
            SELECT_TRY(hipGetLastError());
            SELECT_TRY(hipMemcpyAsync(&hs, st, sizeof hs, hipMemcpyDeviceToHost, stream));
            SELECT_TRY(hipStreamSynchronize(stream));
            if (batch == 0) {
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, ev_layer_[0], ev_layer_[1]);
                layer_ms += ms;
            }
            if (hs.done) break;
            if (batch + 1 >= n / kRoundsPerBatch + 2) {
                err = "panel select: more rounds in a layer than primers";
                return MSSPE_ERR_DEVICE;
            }
        }
        if (hs.n_picked > (uint32_t)n) break;   // reported below
        layer_end.push_back(hs.n_picked);
        if (r >= (uint32_t)depth || hs.deeper != r + 1) break;
    }
    SELECT_TRY(hipEventRecord(ev_[2], stream));

    const int n_picked = (int)hs.n_picked;
    if (n_picked > n || hs.used > (uint32_t)max_tubes) {
        err = "panel select: more picks than primers, or a tube past max_tubes";
        return MSSPE_ERR_DEVICE;
    }
    if (n_picked) {
        SELECT_TRY(hipMemcpyAsync(order_out, d_order, sizeof(uint32_t) * (size_t)n_picked, hipMemcpyDeviceToHost, stream));
        SELECT_TRY(hipMemcpyAsync(gain_out, d_gains, sizeof(uint32_t) * (size_t)n_picked, hipMemcpyDeviceToHost, stream));
    }
    std::vector<uint64_t> h_mask((size_t)n);
    std::vector<uint8_t> h_depth(2 * cells);   // all and cnt lie side by side
    unsigned long long h_counts[2] = {};
    SELECT_TRY(hipMemcpyAsync(tube_out, d_tube, (size_t)n, hipMemcpyDeviceToHost, stream));
    SELECT_TRY(hipMemcpyAsync(flags.data(), d_flags, (size_t)n, hipMemcpyDeviceToHost, stream));
    SELECT_TRY(hipMemcpyAsync(h_mask.data(), d_mask, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
    SELECT_TRY(hipMemcpyAsync(h_counts, d_counts, sizeof h_counts, hipMemcpyDeviceToHost, stream));
    SELECT_TRY(hipMemcpyAsync(h_depth.data(), d_all, 2 * cells, hipMemcpyDeviceToHost, stream));
    SELECT_TRY(hipEventSynchronize(ev_[2]));
    SELECT_TRY(hipStreamSynchronize(stream));
    for (int ph = 0; ph < 2; ++ph) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev_[ph], ev_[ph + 1]);
        phase_us_[ph] = (long long)(ms * 1000.0f);
    }
    layer_us_ = (long long)(layer_ms * 1000.0f);
    layers_ = (long long)layer_end.size();
    rounds_ = hs.rounds;
    tubes_ = hs.used;
    for (int i = 0, layer = 0; i < n_picked; ++i) {
        if (order_out[i] >= (uint32_t)n) {
            err = "panel select: a pick outside the panel";
            return MSSPE_ERR_DEVICE;
        }
        keep_out[order_out[i]] = 1;
        while ((uint32_t)i >= layer_end[(size_t)layer]) ++layer;   // i < n_picked == layer_end.back()
        if (pick_layer_out) pick_layer_out[i] = (uint8_t)(layer + 1);
    }
    for (int p = 0; p < n; ++p) {
        const bool barred = !keep_out[p] && ((flags[(size_t)p] & kSelf) || (h_mask[(size_t)p] & tubes_mask) == tubes_mask);
        barred_ += barred;
        if (barred_out) barred_out[p] = barred ? 1 : 0;
    }
    long long kept1 = 0, keptR = 0;
    for (long g = 0; g < G; ++g)
        for (int b = 0; b < S && g * S + b < n_seg; ++b) {
            const uint8_t a = h_depth[(size_t)g * 64 + (size_t)b], c = h_depth[cells + (size_t)g * 64 + (size_t)b];
            kept1 += c >= 1;
            keptR += c >= depth;
            if (depth_all_out) depth_all_out[g * S + b] = a;
            if (depth_kept_out) depth_kept_out[g * S + b] = c;
        }
    *n_picked_out = n_picked;
    if (n_tubes_used_out) *n_tubes_used_out = (int)hs.used;
    if (counts_out) {
        counts_out[0] = (long long)h_counts[0];
        counts_out[1] = kept1;
        counts_out[2] = (long long)h_counts[1];
        counts_out[3] = keptR;
    }
    return MSSPE_OK;
}

}  // namespace msspe
