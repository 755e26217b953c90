// background_amplicons.hip -- the join behind msspe_background_amplicons* (engine extension, no reference
// counterpart): which pairs of stable off-target sites face each other closely enough to make a product.
//
// The scored pass leaves one key per stable site, pos << 32 | strand << 31 | primer (k_site_fold_keys in
// background_thal.hip).  Sorted as 64-bit numbers the keys are in stream order, and at one position the plus-strand
// keys come first; so the partners of a plus key -- minus keys at q in [p + min_len - k, p + max_len - k] of the
// same record -- all lie BEHIND it in the sorted array, in one contiguous window.
//
// k_key_records: one lane per sorted key, a binary search of its position in the record starts.
//
// k_amplicon_join: one block per tile of 256 consecutive sorted keys, one lane per key.  Neighbouring plus keys share
// almost all of their window, so the block stages the array from its tile onwards through LDS, 1024 keys (and
// their record ids) at a time, until a chunk starts beyond the window of the tile's last key.  Every wave walks the
// staged chunk in step, from its own first key on: the entry is read once per wave (an LDS broadcast), plus-strand
// entries are skipped wave-uniformly, and each lane tests its own plus key against it.  The entry's primer is the same for the whole
// wave, so its "as reverse" count is one LDS atomic per wave (the ballot's popcount), flushed to global memory once
// per chunk; a lane's "as forward" count stays in a register until the end; the caller's list takes one global atomic
// per wave and entry for the places.  LDS: 1024 x (8 + 4 + 4) bytes = 16 KB in one array.
#include "background_amplicons.hpp"

#include <rocprim/device/device_radix_sort.hpp>

namespace msspe {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 1024;

__global__ void __launch_bounds__(kThreads) k_key_records(const uint64_t *sorted, uint32_t m, const uint64_t *starts,
                                                          int n_records, uint32_t *rec)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    const uint64_t pos = sorted[i] >> 32;
    int lo = 0, hi = n_records;   // the first record that starts behind pos
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= pos) lo = mid + 1;
        else hi = mid;
    }
    rec[i] = (uint32_t)lo - 1u;
}

__global__ void __launch_bounds__(kThreads) k_amplicon_join(const uint64_t *sorted, const uint32_t *rec, uint32_t m,
                                                            uint32_t k, uint32_t min_len, uint32_t max_len,
                                                            unsigned long long *counts, msspe_amplicon *out,
                                                            unsigned long long capacity,
                                                            unsigned long long *out_count)
{
    __shared__ uint64_t s_mem[kChunk * 2];   // keys, then record ids, then the hits of each entry
    uint64_t *s_key = s_mem;
    uint32_t *s_rec = (uint32_t *)(s_mem + kChunk);
    uint32_t *s_hits = s_rec + kChunk;

    const uint32_t tile0 = blockIdx.x * kThreads;   // < m by the grid's size; m < 2^31, so no index below wraps
    const uint32_t a = tile0 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = a < m;
    const uint64_t key_a = live ? sorted[a] : 0ull;
    const uint32_t rec_a = live ? rec[a] : 0u;
    const bool plus = live && !((key_a >> 31) & 1ull);
    const uint64_t p = key_a >> 32;
    const uint32_t fwd = (uint32_t)key_a & 0x7fffffffu;
    const uint64_t q_lo = p + (min_len - k), q_hi = p + (max_len - k);   // k <= min_len <= max_len
    const uint32_t last = min(tile0 + (uint32_t)kThreads, m) - 1u;
    const uint64_t limit = (sorted[last] >> 32) + (max_len - k);         // no partner of the tile lies behind it
    uint32_t mine = 0;

    for (uint32_t c0 = tile0; c0 < m; c0 += kChunk) {
        const uint32_t cnt = min((uint32_t)kChunk, m - c0);
        __syncthreads();   // the flush of the chunk before
        for (uint32_t i = threadIdx.x; i < cnt; i += kThreads) {
            s_key[i] = sorted[c0 + i];
            s_rec[i] = rec[c0 + i];
            s_hits[i] = 0u;
        }
        __syncthreads();
        if ((s_key[0] >> 32) > limit) break;   // block-uniform
        // in the tile's own chunk the entries before the wave's first key are smaller than all its keys: no partners
        for (uint32_t i = c0 == tile0 ? (threadIdx.x & ~63u) : 0u; i < cnt; ++i) {
            const uint64_t key_b = s_key[i];
            if (!((key_b >> 31) & 1ull)) continue;   // a plus-strand entry: wave-uniform
            const uint64_t q = key_b >> 32;
            if (q > limit) break;                     // wave-uniform
            const bool hit = plus && q >= q_lo && q <= q_hi && s_rec[i] == rec_a;
            const unsigned long long m_hit = __ballot(hit);
            if (!m_hit) continue;
            if (lane == 0) atomicAdd(&s_hits[i], (uint32_t)__popcll(m_hit));
            mine += hit ? 1u : 0u;
            if (out) {
                unsigned long long base = 0;
                if (lane == 0) base = atomicAdd(out_count, (unsigned long long)__popcll(m_hit));
                base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
                       (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                const unsigned long long at = base + (unsigned long long)__popcll(m_hit & ((1ull << lane) - 1ull));
                if (hit && at < capacity) {
                    msspe_amplicon r;
                    r.fwd = fwd;
                    r.rev = (uint32_t)key_b & 0x7fffffffu;
                    r.pos = (uint32_t)p;
                    r.len = (uint32_t)(q + k - p);
                    out[at] = r;
                }
            }
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < cnt; i += kThreads)
            if (s_hits[i])
                atomicAdd(&counts[2 * (size_t)((uint32_t)s_key[i] & 0x7fffffffu) + 1], (unsigned long long)s_hits[i]);
    }
    if (mine) atomicAdd(&counts[2 * (size_t)fwd], (unsigned long long)mine);
}

}  // namespace

size_t amplicon_sort_temp_bytes(size_t m, unsigned end_bit)
{
    size_t tmp = 0;
    uint64_t *nk = nullptr;
    (void)rocprim::radix_sort_keys(nullptr, tmp, nk, nk, m, 0u, end_bit, (hipStream_t) nullptr);
    return tmp;
}

hipError_t sort_amplicon_keys(const uint64_t *d_keys, uint64_t *d_sorted, size_t m, unsigned end_bit, void *d_temp,
                              size_t temp_bytes, hipStream_t stream)
{
    return rocprim::radix_sort_keys(d_temp, temp_bytes, d_keys, d_sorted, m, 0u, end_bit, stream);
}

hipError_t launch_key_records(const uint64_t *d_sorted, uint32_t m, const uint64_t *d_starts, int n_records,
                              uint32_t *d_rec, hipStream_t stream)
{
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(k_key_records, dim3((m + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, d_sorted, m,
                       d_starts, n_records, d_rec);
    return hipGetLastError();
}

hipError_t launch_amplicon_join(const uint64_t *d_sorted, const uint32_t *d_rec, uint32_t m, int k, uint32_t min_len,
                                uint32_t max_len, unsigned long long *counts, msspe_amplicon *d_out,
                                uint64_t capacity, uint64_t *d_count, hipStream_t stream)
{
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(k_amplicon_join, dim3((m + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, d_sorted,
                       d_rec, m, (uint32_t)k, min_len, max_len, counts, d_out, (unsigned long long)capacity,
                       (unsigned long long *)d_count);
    return hipGetLastError();
}

}  // namespace msspe
