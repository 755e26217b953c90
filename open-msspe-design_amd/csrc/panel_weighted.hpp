// panel_weighted.hpp -- the weighted instances of the set-cover gain kernels (msspe_panel_thin_weighted*,
// msspe_panel_select_weighted*), shared by panel_thin.hip and panel_select.hip.
//
// gain(p) is the sum of weights[s] over the uncovered segments of row p instead of their number.  The weight plane
// wt[g * 64 + b] has the cell layout of the depth planes: a uint32 per (group, bit), 0 on the bits past S and on the
// segments past the last.  Three kernels read it: the first gains (the block's kChunk groups' weights staged in LDS
// beside the covered words), the update of a round, and the sum over the set bits of the covered words (the forced
// rows' weight).  The pick, apply and barring kernels are the unweighted ones: a gain is a uint32 either way, and the
// caller has checked that the weights' total fits one.  St is the file's round state (ThinState / SelectState).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace msspe {

namespace weighted {

constexpr int kThreads = 256;
constexpr int kChunk = 32;   // groups per block of the first gains: 32 x 64 x 4 B = 8 KB of weights in LDS

// The device side of a weighted call: two sums in front (8-byte aligned), the plane, the weights as the caller gave
// them (segment order).
struct Plane {
    unsigned long long *sums;   // [0] weight of the segments all primers cover, [1] of those the forced rows cover
    uint32_t *wt;               // G * 64
    uint32_t *by_segment;       // n_seg
    static size_t bytes(long G, long n_seg)
    {
        return 2 * sizeof(unsigned long long) + sizeof(uint32_t) * ((size_t)G * 64 + (size_t)n_seg);
    }
    Plane(void *buf, long G)
        : sums((unsigned long long *)buf), wt(buf ? (uint32_t *)(sums + 2) : nullptr),
          by_segment(buf ? wt + (size_t)G * 64 : nullptr)   // no buffer: an unweighted call, nothing reads these
    {
    }
};

namespace {   // kernels with internal linkage: each of the two files gets its own, as with its unweighted ones

__device__ __forceinline__ uint64_t wave_or64(uint64_t x)
{
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    for (int o = 32; o; o >>= 1) {
        lo |= __shfl_xor(lo, o, 64);
        hi |= __shfl_xor(hi, o, 64);
    }
    return (uint64_t)hi << 32 | lo;
}

// the sum of cell[b] over the set bits b of w; cell points at a group's 64 cells
template <class Ptr>
__device__ __forceinline__ uint32_t weight_of(uint64_t w, Ptr cell)
{
    uint32_t sum = 0;
    while (w) {
        const int b = __ffsll((unsigned long long)w) - 1;   // b < 64: inside the group's cells
        w &= w - 1;
        sum += cell[b];
    }
    return sum;
}

// wt[g * 64 + b] = weights[g * S + b] on the bits that stand for a segment, else 0: a thread per cell
__global__ __launch_bounds__(kThreads) void k_weight_plane(const uint32_t *weights, int G, int S, long n_seg,
                                                           uint32_t *wt)
{
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    const long g = t >> 6;
    if (g >= G) return;
    const int b = (int)(t & 63);
    const long s = g * S + b;
    wt[t] = b < S && s < n_seg ? weights[s] : 0u;
}

// *out += the weight of the set bits of cov[g] over all groups: a thread per cell, a wave per group
__global__ __launch_bounds__(kThreads) void k_weight_of_cover(const uint64_t *cov, int G, const uint32_t *wt,
                                                              unsigned long long *out)
{
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    const long g = t >> 6;
    if (g >= G) return;   // whole waves: 64 threads per group
    const int b = (int)(t & 63);
    uint32_t v = (cov[g] >> b) & 1ull ? wt[t] : 0u;   // a group's sum is at most the total: it fits
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    if (b == 0 && v) atomicAdd(out, (unsigned long long)v);
}

// gain[p] += weight of (inc[g][p] & ~cov[g]) over the block's chunk of groups: the unweighted first gains with the
// chunk's weights in LDS.  A word no lane of the wave has a bit in is skipped (the OR is wave-uniform).  The OR of a
// group's words over all primers is collected in LDS; its popcount goes to covered_all, its weight to sums[0].
template <class St>
__global__ __launch_bounds__(kThreads) void k_weighted_gain0(const uint64_t *inc, int n, size_t n_pad, int G,
                                                             const uint64_t *cov, const uint32_t *wt, uint32_t *gain,
                                                             St *st, unsigned long long *sums)
{
    __shared__ uint64_t scov[kChunk], sall[kChunk];
    __shared__ uint32_t swt[kChunk * 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int g0 = blockIdx.x * kChunk, cnt = std::min(kChunk, G - g0);
    if (tid < kChunk) {
        scov[tid] = tid < cnt ? cov[g0 + tid] : 0ull;
        sall[tid] = 0ull;
    }
    for (int i = tid; i < kChunk * 64; i += kThreads) swt[i] = (i >> 6) < cnt ? wt[(size_t)g0 * 64 + (size_t)i] : 0u;
    __syncthreads();
    for (int p0 = 0; p0 < n; p0 += kThreads) {   // whole blocks: the wave reductions below need every lane
        const int p = p0 + tid;
        const bool in = p < n;
        const uint64_t *col = inc + (size_t)g0 * n_pad + (size_t)(in ? p : 0);
        uint32_t sum = 0;
        for (int gi = 0; gi < cnt; ++gi) {
            const uint64_t w = in ? col[(size_t)gi * n_pad] : 0ull;
            const uint64_t o = wave_or64(w);
            if (!o) continue;   // wave-uniform
            sum += weight_of(w & ~scov[gi], swt + gi * 64);
            if (lane == 0) atomicOr((unsigned long long *)&sall[gi], (unsigned long long)o);
        }
        if (in && sum) atomicAdd(&gain[p], sum);
    }
    __syncthreads();
    if (tid < cnt) {
        const int c = __popcll(sall[tid]);
        if (c) {
            atomicAdd(&st->covered_all, (unsigned long long)c);
            atomicAdd(&sums[0], (unsigned long long)weight_of(sall[tid], swt + tid * 64));
        }
    }
}

// gain[p] -= weight of (inc[g][p] & new[g]) over the touched groups (blockIdx.y strides over the list), lanes over p
template <class St>
__global__ __launch_bounds__(kThreads) void k_weighted_update(const uint64_t *inc, int n, size_t n_pad,
                                                              const uint32_t *touched, const uint64_t *fresh,
                                                              const uint32_t *wt, uint32_t *gain, const St *st)
{
    if (st->done) return;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const uint32_t nt = st->n_touched;
    uint32_t sum = 0;
    for (uint32_t i = blockIdx.y; i < nt; i += gridDim.y) {
        const uint32_t g = touched[i];   // g < G: k_*_apply wrote it
        sum += weight_of(inc[(size_t)g * n_pad + (size_t)p] & fresh[i], wt + (size_t)g * 64);
    }
    if (sum) atomicSub(&gain[p], sum);
}

}  // namespace

}  // namespace weighted

}  // namespace msspe
