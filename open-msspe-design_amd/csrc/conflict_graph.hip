// conflict_graph.hip -- the conflict graph under a pair of rules: union, counts by kind, ordered edges.
//
// The two screens (thal ANY decided on dG, thal END1 decided on t) each write the bitmap of a block of rows into a plane
// of the context's scratch (capi.cpp runs them through the paths msspe_cross_dimer_dev and msspe_cross_dimer_end_dev
// take).  Three plain kernels follow a row block:
//   k_graph_union  one wave per row: out = any | end, the row's popcount by a wave reduction (one atomic per row), the
//                  three kind counts reduced over the block before three atomics;
//   k_graph_scan   one block: the exclusive scan of the row popcounts, started at the list's running count, which it
//                  then advances -- the carry from one row block to the next stays on the device;
//   k_graph_emit   one wave per row: a wave scan of the per-word popcounts, then every lane writes the set bits of its
//                  word in ascending column order at base + prefix.  The list is ascending in (a, b) by construction.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "conflict_graph.hpp"

namespace msspe {

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kScanThreads = 1024;

__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
{
    for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// inclusive prefix sum over the wave
__device__ __forceinline__ unsigned long long wave_scan(unsigned long long x, int lane)
{
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

__global__ __launch_bounds__(256) void k_graph_union(const uint64_t *any, const uint64_t *end, int rows, int words,
                                                     uint64_t *out, uint32_t *row_conflicts, uint32_t *row_count,
                                                     unsigned long long *kind_counts)
{
    __shared__ uint32_t s_kind[kWavesPerBlock][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r = (long)blockIdx.x * kWavesPerBlock + wave;
    uint32_t cnt = 0, only_any = 0, only_end = 0, both = 0;
    if (r < rows) {
        const size_t off = (size_t)r * (size_t)words;
        for (int w = lane; w < words; w += 64) {
            const uint64_t a = any ? any[off + w] : 0, e = end ? end[off + w] : 0;
            const uint64_t u = a | e;
            if (out) out[off + w] = u;
            cnt += __popcll(u);
            only_any += __popcll(a & ~e);
            only_end += __popcll(e & ~a);
            both += __popcll(a & e);
        }
    }
    cnt = wave_sum(cnt);
    only_any = wave_sum(only_any);
    only_end = wave_sum(only_end);
    both = wave_sum(both);
    if (lane == 0) {
        if (r < rows) {
            if (row_conflicts && cnt) atomicAdd(&row_conflicts[r], cnt);
            if (row_count) row_count[r] = cnt;
        }
        s_kind[wave][0] = only_any;
        s_kind[wave][1] = only_end;
        s_kind[wave][2] = both;
    }
    __syncthreads();
    if (kind_counts && threadIdx.x < 3) {
        unsigned long long s = 0;
        for (int q = 0; q < kWavesPerBlock; ++q) s += s_kind[q][threadIdx.x];
        if (s) atomicAdd(&kind_counts[threadIdx.x], s);
    }
}

__global__ __launch_bounds__(kScanThreads) void k_graph_scan(const uint32_t *row_count, int rows,
                                                             unsigned long long *row_base, unsigned long long *total)
{
    __shared__ unsigned long long s_wave[kScanThreads / 64];
    __shared__ unsigned long long s_carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = *total;
    __syncthreads();
    for (int first = 0; first < rows; first += kScanThreads) {
        const int i = first + (int)threadIdx.x;
        const unsigned long long v = i < rows ? row_count[i] : 0;
        const unsigned long long x = wave_scan(v, lane);
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        unsigned long long before = 0, all = 0;
        for (int q = 0; q < kScanThreads / 64; ++q) {
            if (q < wave) before += s_wave[q];
            all += s_wave[q];
        }
        const unsigned long long carry = s_carry;
        if (i < rows) row_base[i] = carry + before + x - v;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = carry + all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = s_carry;
}

__global__ __launch_bounds__(256) void k_graph_emit(const uint64_t *any, const uint64_t *end, int rows, int words,
                                                    const uint32_t *row_count, const unsigned long long *row_base,
                                                    uint32_t row_first, uint32_t col_first, msspe_kind_edge *edges,
                                                    unsigned long long capacity)
{
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (r >= rows || row_count[r] == 0) return;   // whole waves
    unsigned long long base = row_base[r];
    if (base >= capacity) return;                 // the rest of the row is beyond the buffer
    const size_t off = (size_t)r * (size_t)words;
    for (int w0 = 0; w0 < words; w0 += 64) {
        const int w = w0 + lane;
        const uint64_t a = w < words && any ? any[off + w] : 0, e = w < words && end ? end[off + w] : 0;
        uint64_t u = a | e;
        const unsigned long long c = (unsigned long long)__popcll(u);
        const unsigned long long incl = wave_scan(c, lane);
        unsigned long long pos = base + incl - c;
        while (u) {
            const int bit = __ffsll((unsigned long long)u) - 1;
            u &= u - 1;
            if (pos < capacity) {
                msspe_kind_edge rec;
                rec.a = row_first + (uint32_t)r;
                rec.b = col_first + (uint32_t)w * 64u + (uint32_t)bit;
                rec.kinds = (uint32_t)((a >> bit) & 1) * MSSPE_KIND_ANY | (uint32_t)((e >> bit) & 1) * MSSPE_KIND_END;
                rec.reserved = 0;
                edges[pos] = rec;
            }
            ++pos;
        }
        base += __shfl(incl, 63, 64);
    }
}

}  // namespace

int GraphScratch::ensure(int block_rows, int words, hipStream_t stream, std::string &err)
{
    const size_t need = (size_t)block_rows * (size_t)words;
    auto grow = [&](void **p, size_t bytes) -> int {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
        const hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();   // an allocation failure is reported, not left sticky for the next call
            err = std::string("hipMalloc (conflict graph, ") + std::to_string(bytes) + " bytes): " + hipGetErrorString(e);
            return MSSPE_ERR_DEVICE;
        }
        ++grows_;
        return MSSPE_OK;
    };
    if (need <= plane_words_ && (size_t)block_rows <= rows_cap_) return MSSPE_OK;
    if (hipStreamSynchronize(stream) != hipSuccess) {   // an earlier call may still read the old buffers
        err = "conflict graph: hipStreamSynchronize failed";
        return MSSPE_ERR_DEVICE;
    }
    int rc = MSSPE_OK;
    if (need > plane_words_) {
        plane_words_ = 0;
        if ((rc = grow((void **)&planes_, 2 * need * sizeof(uint64_t)))) return rc;
        plane_words_ = need;
    }
    if ((size_t)block_rows > rows_cap_) {
        rows_cap_ = 0;
        if ((rc = grow((void **)&row_count_, (size_t)block_rows * sizeof(uint32_t))) ||
            (rc = grow((void **)&row_base_, (size_t)block_rows * sizeof(unsigned long long))))
            return rc;
        rows_cap_ = (size_t)block_rows;
    }
    return MSSPE_OK;
}

void GraphScratch::release()
{
    for (void *p : {(void *)planes_, (void *)row_count_, (void *)row_base_})
        if (p) (void)hipFree(p);
    planes_ = nullptr;
    row_count_ = nullptr;
    row_base_ = nullptr;
    plane_words_ = rows_cap_ = 0;
}

hipError_t launch_graph_union(const uint64_t *any, const uint64_t *end, int rows, int words, uint64_t *out,
                              uint32_t *row_conflicts, uint32_t *row_count, unsigned long long *kind_counts,
                              hipStream_t stream)
{
    if (rows <= 0 || words <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_graph_union, dim3((rows + kWavesPerBlock - 1) / kWavesPerBlock), dim3(256), 0, stream, any, end,
                       rows, words, out, row_conflicts, row_count, kind_counts);
    return hipGetLastError();
}

hipError_t launch_graph_scan(const uint32_t *row_count, int rows, unsigned long long *row_base,
                             unsigned long long *total, hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_graph_scan, dim3(1), dim3(kScanThreads), 0, stream, row_count, rows, row_base, total);
    return hipGetLastError();
}

hipError_t launch_graph_emit(const uint64_t *any, const uint64_t *end, int rows, int words, const uint32_t *row_count,
                             const unsigned long long *row_base, uint32_t row_first, uint32_t col_first,
                             msspe_kind_edge *edges, unsigned long long capacity, hipStream_t stream)
{
    if (rows <= 0 || words <= 0 || capacity == 0) return hipSuccess;
    hipLaunchKernelGGL(k_graph_emit, dim3((rows + kWavesPerBlock - 1) / kWavesPerBlock), dim3(256), 0, stream, any, end,
                       rows, words, row_count, row_base, row_first, col_first, edges, capacity);
    return hipGetLastError();
}

}  // namespace msspe
