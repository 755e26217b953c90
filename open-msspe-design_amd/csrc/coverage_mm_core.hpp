// coverage_mm_core.hpp -- what the kernels that compare window positions with primer words share (coverage_mm.hip,
// coverage_thal.hip): the lane mapping's constants, a base of the alignment in either SeqView form, the bit-plane
// words and their comparison, and the host's conversion of msspe_pack_oligos words into planes.  The comments of
// coverage_mm.hip explain the forms.  Device code only: include from a .hip file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "kmer_stage.hpp"

namespace msspe {
namespace mm_core {

constexpr int kThreads = 256;
constexpr int kItems = 8;                              // window positions per thread per round
constexpr int kRound = kThreads * kItems;              // positions per round
constexpr int kMaxSeg = 64;                            // segments per block (one bit each in the COUNTS words)

// base `col` of record `rec`: 0..3 (A C G T), or -1 for anything else (the validity rule of main.rs:167)
__device__ __forceinline__ int base_at(const SeqView &v, size_t rec, size_t col)
{
    if (v.ascii) {
        const uint8_t c = v.ascii[rec * v.seq_len + col];
        return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
    }
    const size_t bw = (v.seq_len + 31) / 32, rw = bw + (v.seq_len + 63) / 64;
    const uint64_t *row = v.packed + rec * rw;
    if (!((row[bw + (col >> 6)] >> (col & 63)) & 1ull)) return -1;
    return (int)((row[col >> 5] >> (2 * (col & 31))) & 3ull);
}

// A word as the comparison reads it: two 32-bit halves whose XORs, ORed together, give the mismatch mask.  32-bit
// form: (w, rotr(w, 16)) -- the mask then holds the per-base bits in both halves; 64-bit form: (low plane, high plane).
__device__ __forceinline__ uint2 rot_pair(uint32_t w) { return make_uint2(w, __builtin_amdgcn_alignbit(w, w, 16)); }
__device__ __forceinline__ uint2 make_word(uint32_t lo, uint32_t hi, uint32_t) { return rot_pair(lo | (hi << 16)); }
__device__ __forceinline__ uint2 make_word(uint32_t lo, uint32_t hi, uint2) { return make_uint2(lo, hi); }

// one bit per differing base (twice over for the 32-bit form): an XOR and a three-input bit operation
__device__ __forceinline__ uint32_t diff_mask(uint2 w, uint2 u) { return (w.x ^ u.x) | (w.y ^ u.y); }

// four consecutive tile primers (16-byte aligned: i is a multiple of 4)
__device__ __forceinline__ void load4(const uint32_t *tile, int i, uint2 (&u)[4])
{
    const uint4 v = *reinterpret_cast<const uint4 *>(tile + i);
    u[0] = rot_pair(v.x); u[1] = rot_pair(v.y); u[2] = rot_pair(v.z); u[3] = rot_pair(v.w);
}
__device__ __forceinline__ void load4(const uint2 *tile, int i, uint2 (&u)[4])
{
    const uint4 a = *reinterpret_cast<const uint4 *>(tile + i), b = *reinterpret_cast<const uint4 *>(tile + i + 2);
    u[0] = make_uint2(a.x, a.y); u[1] = make_uint2(a.z, a.w); u[2] = make_uint2(b.x, b.y); u[3] = make_uint2(b.z, b.w);
}

template <typename T>
void to_planes(const uint64_t *in, int n, std::vector<T> &out);

template <>
inline void to_planes<uint32_t>(const uint64_t *in, int n, std::vector<uint32_t> &out)
{
    for (int i = 0; i < n; ++i) {
        uint32_t lo = 0, hi = 0;
        for (int q = 0; q < 16; ++q) {
            lo |= (uint32_t)((in[i] >> (2 * q)) & 1ull) << q;
            hi |= (uint32_t)((in[i] >> (2 * q + 1)) & 1ull) << q;
        }
        out.push_back(lo | (hi << 16));
    }
}

template <>
inline void to_planes<uint2>(const uint64_t *in, int n, std::vector<uint2> &out)
{
    for (int i = 0; i < n; ++i) {
        uint32_t lo = 0, hi = 0;
        for (int q = 0; q < 32; ++q) {
            lo |= (uint32_t)((in[i] >> (2 * q)) & 1ull) << q;
            hi |= (uint32_t)((in[i] >> (2 * q + 1)) & 1ull) << q;
        }
        out.push_back(make_uint2(lo, hi));
    }
}

// largest mismatch mask with the primer's last E bases equal (the 3' end is the high plane bits)
template <typename T>
inline uint32_t exact_3p_limit(int k, int E)
{
    const int s = k - E;   // 3' bases start at plane bit s
    return sizeof(T) == 4 ? (s >= 16 ? 0xffffffffu : (1u << (16 + s)) - 1u) : (uint32_t)((1ull << s) - 1ull);
}

}  // namespace mm_core
}  // namespace msspe
