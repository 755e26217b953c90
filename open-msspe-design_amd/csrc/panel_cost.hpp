// panel_cost.hpp -- the cost instances of the set-cover pick (msspe_panel_thin_cost*, msspe_panel_select_cost*;
// DESIGN.md 4.18), shared by panel_thin.hip and panel_select.hip.
//
// A round keeps the live primer of greatest gain(p) / cost(p) instead of greatest gain.  The ratio is never formed: p
// beats q when gain(p) * cost(q) > gain(q) * cost(p) in 64-bit unsigned arithmetic (both factors are uint32, so the
// products are exact), on equal products the greater gain wins, then the lowest index.  A primer whose gain is below
// min_gain is no candidate at all: it cannot win on ratio and then stop the loop while another primer qualifies.  The
// gains are the sibling's, weighted or not; the first gains, apply, update and barring kernels run as they stand, and
// the pick here leaves in the round state exactly what k_thin_pick / k_select_pick leave.  St is the file's round state
// (ThinState / SelectState).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace msspe {

namespace cost {

constexpr int kThreads = 256;
constexpr uint32_t kNobody = 0xFFFFFFFFu;   // no primer has this index: n < 2^31

// A thread's, a wave's, the block's best so far.  Nobody is (gain 0, cost 1, index kNobody): a real candidate of gain
// g >= 1 has g * 1 > 0 * its cost, and one of gain 0 (min_gain 0) ties on product and gain and wins on its index.
struct Best {
    uint32_t gain, cost, p;
};

__device__ __forceinline__ bool beats(const Best &a, const Best &b)
{
    const uint64_t ab = (uint64_t)a.gain * b.cost, ba = (uint64_t)b.gain * a.cost;
    if (ab != ba) return ab > ba;
    if (a.gain != b.gain) return a.gain > b.gain;
    return a.p < b.p;
}

// Every lane ends with the wave's best: the order is total, so both sides of an exchange agree on the winner.
__device__ __forceinline__ Best wave_best(Best x)
{
    for (int o = 32; o; o >>= 1) {
        Best y;
        y.gain = __shfl_xor(x.gain, o, 64);
        y.cost = __shfl_xor(x.cost, o, 64);
        y.p = __shfl_xor(x.p, o, 64);
        if (beats(y, x)) x = y;
    }
    return x;
}

namespace {   // kernels with internal linkage: each of the two files gets its own, as with its own pick

// The block's best from every thread's: the four wave results go through LDS, thread 0 returns the winner (the other
// threads' return value is their wave's).
__device__ __forceinline__ Best block_best(Best x, Best *swave)
{
    const int tid = threadIdx.x;
    x = wave_best(x);
    if ((tid & 63) == 0) swave[tid >> 6] = x;
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < kThreads / 64; ++w)
            if (beats(swave[w], x)) x = swave[w];
    return x;
}

// One block: k_thin_pick under the cost rule.  live[p]: unforced and unpicked.
template <class St>
__global__ __launch_bounds__(kThreads) void k_thin_pick_cost(const uint32_t *gain, const uint32_t *costs, uint8_t *live,
                                                             int n, uint32_t min_gain, uint32_t *order,
                                                             uint32_t *gains, St *st)
{
    if (st->done) return;
    __shared__ Best swave[kThreads / 64];
    Best best = {0u, 1u, kNobody};
    for (int p = threadIdx.x; p < n; p += kThreads) {
        if (!live[p]) continue;
        const Best c = {gain[p], costs[p], (uint32_t)p};
        if (c.gain >= min_gain && beats(c, best)) best = c;
    }
    best = block_best(best, swave);
    if (threadIdx.x == 0) {
        st->rounds += 1;
        if (best.p == kNobody) {
            st->done = 1;
        } else {
            const uint32_t i = st->n_picked;   // i < n: every pick leaves the live set
            order[i] = best.p;
            gains[i] = best.gain;
            live[best.p] = 0;
            st->n_picked = i + 1;
            st->pick = best.p;
            st->n_touched = 0;
        }
    }
}

// One block: k_select_pick under the cost rule.  Live: the flag's live bit and a tube left in the mask; the pick takes
// the lowest tube its mask leaves.
template <class St>
__global__ __launch_bounds__(kThreads) void k_select_pick_cost(const uint32_t *gain, const uint32_t *costs,
                                                               uint8_t *flags, uint8_t live_bit, const uint64_t *mask,
                                                               int n, uint32_t min_gain, uint64_t tubes_mask,
                                                               uint32_t *order, uint32_t *gains, uint8_t *tube, St *st)
{
    if (st->done) return;
    __shared__ Best swave[kThreads / 64];
    Best best = {0u, 1u, kNobody};
    for (int p = threadIdx.x; p < n; p += kThreads) {
        if (!(flags[p] & live_bit) || !(~mask[p] & tubes_mask)) continue;
        const Best c = {gain[p], costs[p], (uint32_t)p};
        if (c.gain >= min_gain && beats(c, best)) best = c;
    }
    best = block_best(best, swave);
    if (threadIdx.x == 0) {
        st->rounds += 1;
        if (best.p == kNobody) {
            st->done = 1;
        } else {
            const uint32_t p = best.p, i = st->n_picked;   // p < n, i < n: every pick leaves the live set
            const uint32_t t = (uint32_t)__builtin_ctzll(~mask[p] & tubes_mask);   // nonzero: p is live
            order[i] = p;
            gains[i] = best.gain;
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

}  // namespace

}  // namespace cost

}  // namespace msspe
