// coverage_mm.hip -- segment coverage of a primer set within max_mismatches, the primer's last exact_3p bases exact
// (engine extension; the exact rule it generalises is od-msspe/src/main.rs:518-594, k_segment_hits).
//
// Every valid window position is compared with every primer of its direction (head windows: forward primers;
// the reverse complement of tail windows: reverse primers), so the work is all-pairs integer VALU work.
// Words are held as two bit PLANES -- bit q of the low plane is bit 0 of base q, bit q of the high plane bit 1 --
// so the one-bit-per-base mismatch mask of a window word w and a primer word u is (w_lo ^ u_lo) | (w_hi ^ u_hi):
// no shift and no 0x55.. mask, as the 2-bit interleaved form would need.  k <= 16: both 16-bit planes in one 32-bit
// word (low plane in bits 0..15); the mask is (w ^ u) | (rotr(w, 16) ^ rotr(u, 16)), which holds it in both halves
// (its popcount is twice the mismatch count; the rotations are made once per window word and once per primer read).
// 17 <= k <= 31: the planes are the two halves of a 64-bit word.  Either way the mask is one v_xor and one
// three-input v_bitop3, then v_bcnt, the 3' compare, a select and half a v_min3.
// The primer's 3' end is its last bases, the high plane bits: "no mismatch in the last E bases" is mask <= lim.
//
// Lane mapping: a block takes S whole segments (S <= 64) and, for each direction, their S * (W - k + 1) window
// positions flattened over (segment, position); thread t holds the positions t + 256 j (j < kItems) of a round in
// registers, so all lanes work whatever W - k is.  The direction's primers are staged in LDS in tiles and read by all
// lanes at one address (an LDS broadcast, four 32-bit or two 64-bit primers per ds_read_b128).  Per-segment minima
// are reduced in LDS (a ds_min only for positions that matched) and written with one byte store per segment.
// COUNTS: per tile primer a 64-bit LDS word of the block's segments it matched in (ds_or by the matching lanes), then
// one global atomic per (block, primer) with a nonzero popcount.  Without counts that code is not compiled in.
// INCIDENCE (the panel thinning's first pass, panel_thin.hip): the same LDS words, stored instead of counted -- one plain
// 64-bit vector store per (block, primer) into the group-major matrix inc[block * n_pad + primer], every word once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "coverage_mm.hpp"
#include "coverage_mm_core.hpp"

namespace msspe {
namespace {

using namespace mm_core;   // the lane mapping's constants, base_at, the plane words, load4, to_planes

constexpr size_t kLdsBudget = 65536;                   // dynamic LDS per block: keeps two or more blocks per CU

// best[seg] = smallest mismatch count (scaled: x2 for the 32-bit form) of a match, 255 when none; counts[primer] +=
// segments it matched in.  lim: largest mask with the 3' bases equal; max_score: max_mismatches, scaled.
// INCIDENCE (with COUNTS): `counts` is the incidence matrix, 64-bit words, n_pad = n_fwd + n_rev rounded up to 64.
// k_coverage_mm_list (coverage_thal.hip) repeats this round body -- tile staging, window words, the 4 x 8 compare --
// with an append where COUNTS ORs a bit: a change to either loop belongs in both.
template <typename T, bool COUNTS, bool INCIDENCE = false>
__global__ void __launch_bounds__(kThreads) k_coverage_mm(const SeqView seqs, int n_seg, int P, int seg_size,
                                                          int stride, int W, int k, int S, const T *fwd, int n_fwd,
                                                          const T *rev, int n_rev, int tile_cap, uint32_t lim,
                                                          uint32_t max_score, int scale, uint8_t *best,
                                                          uint32_t *counts)
{
    extern __shared__ __align__(16) unsigned char smem[];
    T *tile = reinterpret_cast<T *>(smem);
    uint64_t *bits = reinterpret_cast<uint64_t *>(smem + (size_t)tile_cap * sizeof(T));
    uint32_t *sbest = reinterpret_cast<uint32_t *>(smem + (size_t)tile_cap * (sizeof(T) + (COUNTS ? 8 : 0)));
    const int tid = threadIdx.x;
    const int per = W - k + 1;
    const long seg0 = (long)blockIdx.x * S;
    const int n_blk = (int)std::min<long>(S, (long)n_seg - seg0);
    const int n_items = n_blk * per;
    for (int s = tid; s < kMaxSeg; s += kThreads) sbest[s] = 255u;
    if (COUNTS)
        for (int i = tid; i < tile_cap; i += kThreads) bits[i] = 0ull;

    for (int dir = 0; dir < 2; ++dir) {
        const T *src = dir ? rev : fwd;
        const int n_u = dir ? n_rev : n_fwd;
        for (int t0 = 0; t0 < n_u; t0 += tile_cap) {
            const int cnt = std::min(tile_cap, n_u - t0), cnt4 = (cnt + 3) & ~3;
            __syncthreads();   // the previous tile's readers are done (and sbest / bits are initialised)
            for (int i = tid; i < cnt4; i += kThreads) tile[i] = src[t0 + std::min(i, cnt - 1)];   // pad: repeats
            __syncthreads();
            for (int base = 0; base < n_items; base += kRound) {
                uint2 w[kItems];
                uint32_t b[kItems];
                int segl[kItems];
                uint32_t valid = 0;   // bit j: position j of this round exists and holds k bases
#pragma unroll
                for (int j = 0; j < kItems; ++j) {
                    const int item = base + j * kThreads + tid;
                    uint32_t lo = 0, hi = 0;
                    segl[j] = 0;
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
                            lo |= (uint32_t)(c & 1) << q;
                            hi |= (uint32_t)(c >> 1) << q;
                        }
                        segl[j] = sl;
                        valid |= (uint32_t)ok << j;
                    }
                    w[j] = make_word(lo, hi, T());
                    b[j] = 255u;
                }
                for (int i = 0; i < cnt4; i += 4) {
                    uint2 u[4];
                    load4(tile, i, u);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int j = 0; j < kItems; ++j) {
                            const uint32_t d = diff_mask(w[j], u[q]);
                            const uint32_t pc = (uint32_t)__popc(d);
                            const bool ok3 = d <= lim;
                            b[j] = std::min(b[j], ok3 ? pc : 255u);
                            if (COUNTS)
                                if (ok3 && pc <= max_score && ((valid >> j) & 1u))
                                    atomicOr((unsigned long long *)&bits[i + q], 1ull << segl[j]);
                        }
                }
#pragma unroll
                for (int j = 0; j < kItems; ++j)
                    if (((valid >> j) & 1u) && b[j] <= max_score) atomicMin(&sbest[segl[j]], b[j]);
            }
            if (COUNTS) {
                __syncthreads();
                const int out0 = (dir ? n_fwd : 0) + t0;
                if (INCIDENCE) {
                    const size_t n_pad = ((size_t)n_fwd + (size_t)n_rev + 63) & ~(size_t)63;
                    uint64_t *inc = reinterpret_cast<uint64_t *>(counts) + (size_t)blockIdx.x * n_pad + (size_t)out0;
                    for (int i = tid; i < cnt; i += kThreads) inc[i] = bits[i];
                } else {
                    for (int i = tid; i < cnt; i += kThreads) {
                        const int c = __popcll(bits[i]);
                        if (c) atomicAdd(&counts[out0 + i], (uint32_t)c);
                    }
                }
                for (int i = tid; i < cnt4; i += kThreads) bits[i] = 0ull;
            }
        }
    }
    __syncthreads();
    for (int s = tid; s < n_blk; s += kThreads) {
        const uint32_t v = sbest[s];
        best[seg0 + s] = v <= max_score ? (uint8_t)(v / (uint32_t)scale) : (uint8_t)255;
    }
}

#define MM_TRY(expr)                                                        \
    do {                                                                    \
        hipError_t e__ = (expr);                                            \
        if (e__ != hipSuccess) {                                            \
            err = std::string(#expr) + ": " + hipGetErrorString(e__);       \
            return MSSPE_ERR_DEVICE;                                        \
        }                                                                   \
    } while (0)

}  // namespace

int MismatchCoverage::ensure(int slot, size_t bytes, std::string &err)
{
    if (cap_[slot] >= bytes) return MSSPE_OK;
    if (buf_[slot]) (void)hipFree(buf_[slot]);
    buf_[slot] = nullptr;
    cap_[slot] = 0;
    const hipError_t e = hipMalloc(&buf_[slot], bytes ? bytes : 16);
    if (e != hipSuccess) {
        err = std::string("hipMalloc (mismatch coverage): ") + hipGetErrorString(e);
        return MSSPE_ERR_DEVICE;
    }
    cap_[slot] = bytes;
    return MSSPE_OK;
}

void MismatchCoverage::release()
{
    for (int s = 0; s < 3; ++s) {
        if (buf_[s]) (void)hipFree(buf_[s]);
        buf_[s] = nullptr;
        cap_[s] = 0;
    }
}

namespace {

template <typename T>
int launch(const SeqView &d_seqs, long n_seg, long P, const msspe_kmer_opt &opt, int M, int E, const uint64_t *fwd,
           int n_fwd, const uint64_t *rev, int n_rev, bool want_counts, uint64_t *d_inc, void *const *buf,
           hipStream_t stream, std::vector<T> &words, std::string &err)
{
    const int k = opt.kmer_size, W = opt.search_window_size;
    constexpr bool narrow = sizeof(T) == 4;
    const int scale = narrow ? 2 : 1;
    const uint32_t lim = exact_3p_limit<T>(k, E);
    words.clear();
    to_planes<T>(fwd, n_fwd, words);
    to_planes<T>(rev, n_rev, words);
    T *d_words = (T *)buf[0];
    uint32_t *d_counts = (uint32_t *)buf[1];
    uint8_t *d_best = (uint8_t *)buf[2];
    if (!words.empty())
        MM_TRY(hipMemcpyAsync(d_words, words.data(), sizeof(T) * words.size(), hipMemcpyHostToDevice, stream));
    const size_t per_word = sizeof(T) + (want_counts || d_inc ? 8 : 0);
    const int max_tile = (int)((kLdsBudget - kMaxSeg * sizeof(uint32_t)) / per_word) & ~3;
    const int tile_cap = std::max(4, std::min(max_tile, (std::max(n_fwd, n_rev) + 3) & ~3));
    const size_t lds = (size_t)tile_cap * per_word + kMaxSeg * sizeof(uint32_t);
    const int S = MismatchCoverage::group_size(opt);
    const long grid = (n_seg + S - 1) / S;
    const uint32_t max_score = (uint32_t)(M * scale);
    if (d_inc) {
        hipLaunchKernelGGL((k_coverage_mm<T, true, true>), dim3((unsigned)grid), dim3(kThreads), lds, stream, d_seqs,
                           (int)n_seg, (int)P, opt.segment_size, opt.overlap_size, W, k, S, d_words, n_fwd,
                           d_words + n_fwd, n_rev, tile_cap, lim, max_score, scale, d_best,
                           reinterpret_cast<uint32_t *>(d_inc));
    } else if (want_counts) {
        MM_TRY(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * (size_t)(n_fwd + n_rev), stream));
        hipLaunchKernelGGL((k_coverage_mm<T, true>), dim3((unsigned)grid), dim3(kThreads), lds, stream, d_seqs,
                           (int)n_seg, (int)P, opt.segment_size, opt.overlap_size, W, k, S, d_words, n_fwd,
                           d_words + n_fwd, n_rev, tile_cap, lim, max_score, scale, d_best, d_counts);
    } else {
        hipLaunchKernelGGL((k_coverage_mm<T, false>), dim3((unsigned)grid), dim3(kThreads), lds, stream, d_seqs,
                           (int)n_seg, (int)P, opt.segment_size, opt.overlap_size, W, k, S, d_words, n_fwd,
                           d_words + n_fwd, n_rev, tile_cap, lim, max_score, scale, d_best, (uint32_t *)nullptr);
    }
    MM_TRY(hipGetLastError());
    return MSSPE_OK;
}

}  // namespace

int MismatchCoverage::group_size(const msspe_kmer_opt &opt)
{
    return std::max(1, std::min(kMaxSeg, kRound / (opt.search_window_size - opt.kmer_size + 1)));
}

int MismatchCoverage::check(int n_seq, size_t seq_len, const msspe_kmer_opt &opt, int max_mismatches, int exact_3p,
                            const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev, long *P_out,
                            std::string &err)
{
    const int k = opt.kmer_size, W = opt.search_window_size;
    if (k < 1 || k > 31) {
        err = "coverage_mm: unsupported k (need 1 <= k <= 31)";
        return MSSPE_ERR_K;
    }
    if (max_mismatches < 0 || max_mismatches > k || exact_3p < 0 || exact_3p > k) {
        err = "coverage_mm: max_mismatches and exact_3p must lie in 0..k";
        return MSSPE_ERR_ARG;
    }
    if (W < k || opt.segment_size < W || opt.overlap_size < 1 || n_seq < 0 || n_fwd < 0 || n_rev < 0) {
        err = "coverage_mm: unsupported options (need k <= window <= segment, stride >= 1)";
        return MSSPE_ERR_ARG;
    }
    const uint64_t high = ~0ull << (2 * k);
    for (int i = 0; i < n_fwd + n_rev; ++i)
        if ((i < n_fwd ? fwd_words[i] : rev_words[i - n_fwd]) & high) {
            err = "coverage_mm: a primer word has bits above 2 k";
            return MSSPE_ERR_ARG;
        }
    const long P = seq_len < (size_t)opt.segment_size
                       ? 0
                       : (long)((seq_len - (size_t)opt.segment_size) / (size_t)opt.overlap_size) + 1;
    if (P * n_seq > 0x7fffffffL) {
        err = "coverage_mm: alignment too large for 32-bit segment indices";
        return MSSPE_ERR_ARG;
    }
    *P_out = P;
    return MSSPE_OK;
}

int MismatchCoverage::run(const SeqView &d_seqs, int n_seq, size_t seq_len, const msspe_kmer_opt &opt,
                          int max_mismatches, int exact_3p, const uint64_t *fwd_words, int n_fwd,
                          const uint64_t *rev_words, int n_rev, uint8_t *best_out, uint32_t *primer_segments_out,
                          hipStream_t stream, std::string &err)
{
    return run(d_seqs, n_seq, seq_len, opt, max_mismatches, exact_3p, fwd_words, n_fwd, rev_words, n_rev, best_out,
               primer_segments_out, nullptr, stream, err);
}

int MismatchCoverage::incidence(const SeqView &d_seqs, int n_seq, size_t seq_len, const msspe_kmer_opt &opt,
                                int max_mismatches, int exact_3p, const uint64_t *fwd_words, int n_fwd,
                                const uint64_t *rev_words, int n_rev, uint64_t *d_inc, hipStream_t stream,
                                std::string &err)
{
    return run(d_seqs, n_seq, seq_len, opt, max_mismatches, exact_3p, fwd_words, n_fwd, rev_words, n_rev, nullptr,
               nullptr, d_inc, stream, err);
}

int MismatchCoverage::run(const SeqView &d_seqs, int n_seq, size_t seq_len, const msspe_kmer_opt &opt,
                          int max_mismatches, int exact_3p, const uint64_t *fwd_words, int n_fwd,
                          const uint64_t *rev_words, int n_rev, uint8_t *best_out, uint32_t *primer_segments_out,
                          uint64_t *d_inc, hipStream_t stream, std::string &err)
{
    const int k = opt.kmer_size;
    long P = 0;
    int rc = check(n_seq, seq_len, opt, max_mismatches, exact_3p, fwd_words, n_fwd, rev_words, n_rev, &P, err);
    if (rc) return rc;
    const long n_seg = P * n_seq;
    if (primer_segments_out) std::fill(primer_segments_out, primer_segments_out + n_fwd + n_rev, 0u);
    if (n_seg == 0) return MSSPE_OK;
    const bool narrow = k <= 16;
    const size_t wbytes = (narrow ? 4 : 8) * (size_t)(n_fwd + n_rev);
    if ((rc = ensure(0, wbytes, err)) || (rc = ensure(1, sizeof(uint32_t) * (size_t)(n_fwd + n_rev), err)) ||
        (rc = ensure(2, (size_t)n_seg, err)))
        return rc;
    std::vector<uint32_t> w32;   // host copies: must outlive the uploads (synchronised below)
    std::vector<uint2> w64;
    rc = narrow ? launch<uint32_t>(d_seqs, n_seg, P, opt, max_mismatches, exact_3p, fwd_words, n_fwd, rev_words,
                                   n_rev, primer_segments_out != nullptr, d_inc, buf_, stream, w32, err)
                : launch<uint2>(d_seqs, n_seg, P, opt, max_mismatches, exact_3p, fwd_words, n_fwd, rev_words, n_rev,
                                primer_segments_out != nullptr, d_inc, buf_, stream, w64, err);
    if (rc) return rc;
    if (d_inc) {   // the thinning goes on in the stream; the primer words' host copies end here
        MM_TRY(hipStreamSynchronize(stream));
        return MSSPE_OK;
    }
    MM_TRY(hipMemcpyAsync(best_out, buf_[2], (size_t)n_seg, hipMemcpyDeviceToHost, stream));
    if (primer_segments_out && n_fwd + n_rev)
        MM_TRY(hipMemcpyAsync(primer_segments_out, buf_[1], sizeof(uint32_t) * (size_t)(n_fwd + n_rev),
                              hipMemcpyDeviceToHost, stream));
    MM_TRY(hipStreamSynchronize(stream));
    return MSSPE_OK;
}

}  // namespace msspe
