// background.hip -- where else do the primers land: every position of a background stream (unaligned records back to
// back, an invalid column between two records) against every primer, on both strands, within max_mismatches with the
// primer's last exact_3p bases exact (engine extension, no reference counterpart; the comparison is coverage_mm.hip's).
//
// Words are two bit PLANES (bit q of the low plane = bit 0 of base q), the mismatch mask of a window w and a primer u
// is (w_lo ^ u_lo) | (w_hi ^ u_hi): one v_xor and one v_bitop3, then v_bcnt.  k <= 16: both planes in one 32-bit word
// with its 16-bit rotation as the partner (the mask then sits in both halves, its popcount is twice the count);
// 17 <= k <= 31: the planes are the halves of a 64-bit word.  "Last E bases exact" is mask <= lim.
//
// Both strands from one primer read: a window's planes are cut out once per run of positions, and so is the window's
// reverse complement (plane bits reversed and inverted: two v_bfrev, shifts and nots per window, not per comparison).
// The minus strand is then the plus strand's test on that second register pair against the SAME primer word, so the
// tile holds n words, not 2 n, and a primer read from LDS (one address for all lanes: a broadcast, four 32-bit or two
// 64-bit primers per ds_read_b128) serves 2 x kItems comparisons.
//
// Lane mapping: the stream positions are cut into runs of kThreads x kItems; a block is persistent over a contiguous
// range of runs.  Per run, 65 threads turn the run's 2-bit words (+ a k - 1 halo) into plane bit streams in LDS, and
// thread t cuts its windows t + 256 j (j < kItems) out of them with one v_alignbit per plane.  A run starts at a
// multiple of 2048 columns, so word indices stay 32-bit up to 2^32 - 1 columns and no position is ever signed.
//
// Counting: sites are rare (13-mer, 2 mismatches, random sequence: 1.1e-5 per comparison), so the common path only
// keeps the per-lane MINIMUM popcount over the lane's kItems windows (half a v_min3 per comparison) and tests it once per
// (wave, primer, strand): one v_cmp and a scalar branch on the wave's mask.  Only a wave with a candidate re-compares
// its kItems windows with the validity bit and the 3' rule, adds the matching lanes to the primer's LDS counter and, when
// a list is wanted, appends one record per site.  LDS counters go out with one 64-bit global atomic per (block, tile
// primer, strand) that is nonzero, after the block's last run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "background.hpp"

namespace msspe {
namespace {

constexpr int kThreads = 256;
constexpr int kItems = 8;                      // window positions per thread per run
constexpr uint32_t kRun = kThreads * kItems;   // positions per run: a multiple of 64, so a run starts on a word
constexpr int kRunWords = kRun / 32 + 1;       // 32-column words a run reads: its own and one of halo (k - 1 <= 30)
constexpr size_t kTileBytes = 16384;           // LDS for the primer tile and its counters: several blocks per CU
constexpr int kBlocksPerCu = 4;

// the comparison of coverage_mm.hip (restated here: that translation unit stays as it is)
__device__ __forceinline__ uint2 rot_pair(uint32_t w) { return make_uint2(w, __builtin_amdgcn_alignbit(w, w, 16)); }
__device__ __forceinline__ uint2 make_word(uint32_t lo, uint32_t hi, uint32_t) { return rot_pair(lo | (hi << 16)); }
__device__ __forceinline__ uint2 make_word(uint32_t lo, uint32_t hi, uint2) { return make_uint2(lo, hi); }
__device__ __forceinline__ uint32_t diff_mask(uint2 w, uint2 u) { return (w.x ^ u.x) | (w.y ^ u.y); }
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

// the even bits of x, packed: bit q of the result is bit 2 q of x
__device__ __forceinline__ uint32_t even_bits(uint64_t x)
{
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull;
    x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
    x = (x | (x >> 16)) & 0x00000000ffffffffull;
    return (uint32_t)x;
}

// counts[2 i + s] += sites of primer i on strand s (0 plus, 1 minus); sites / capacity / count: the list (LIST only).
// lim: largest mask with the 3' bases equal; max_score: max_mismatches, scaled (x2 for the 32-bit form).
template <typename T, bool LIST>
__global__ void __launch_bounds__(kThreads) k_background_sites(const uint64_t *packed, size_t total_len, int k,
                                                               const T *words, int n, int tile_cap, uint32_t lim,
                                                               uint32_t max_score, int scale, uint32_t n_runs,
                                                               unsigned long long *counts, msspe_site *sites,
                                                               unsigned long long capacity, unsigned long long *count)
{
#define BG_RUN_BASE
#define BG_PRIMER_BASE
#include "background_sites_body.inc"
#undef BG_RUN_BASE
#undef BG_PRIMER_BASE
}

// One slab for msspe_background_thal*: the runs [run_base, run_base + n_runs) against the n words at `words`, which
// are the primers primer_base .. of the caller's list (a record carries the caller's index); always with the list,
// whose counter says whether the slab fitted.
template <typename T, bool LIST>
__global__ void __launch_bounds__(kThreads) k_background_slab(const uint64_t *packed, size_t total_len, int k,
                                                              const T *words, int n, int tile_cap, uint32_t lim,
                                                              uint32_t max_score, int scale, uint32_t n_runs,
                                                              unsigned long long *counts, msspe_site *sites,
                                                              unsigned long long capacity, unsigned long long *count,
                                                              uint32_t run_base, uint32_t primer_base)
{
#define BG_RUN_BASE run_base +
#define BG_PRIMER_BASE primer_base +
#include "background_sites_body.inc"
#undef BG_RUN_BASE
#undef BG_PRIMER_BASE
}

// one thread per output word: 32 columns of bases or 64 of validity
__global__ void __launch_bounds__(256) k_pack_stream(const uint8_t *ascii, size_t n_cols, uint64_t *bases,
                                                     uint64_t *valid)
{
    const size_t nb = (n_cols + 31) / 32, nv = (n_cols + 63) / 64;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nb + nv) return;
    const bool is_base = t < nb;
    const size_t c0 = is_base ? t * 32 : (t - nb) * 64;
    const int width = is_base ? 32 : 64;
    uint64_t out = 0;
    for (int q = 0; q < width && c0 + (size_t)q < n_cols; ++q) {
        const uint8_t c = ascii[c0 + (size_t)q];
        const int b = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
        if (is_base)
            out |= (uint64_t)(b >= 0 ? b : 0) << (2 * q);   // columns without a base: bits 00, validity 0
        else
            out |= (uint64_t)(b >= 0) << q;
    }
    (is_base ? bases : valid)[is_base ? t : t - nb] = out;
}

template <typename T>
void to_planes(const uint64_t *in, int n, std::vector<T> &out);

template <>
void to_planes<uint32_t>(const uint64_t *in, int n, std::vector<uint32_t> &out)
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
void to_planes<uint2>(const uint64_t *in, int n, std::vector<uint2> &out)
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

#define BG_TRY(expr)                                                        \
    do {                                                                    \
        hipError_t e__ = (expr);                                            \
        if (e__ != hipSuccess) {                                            \
            err = std::string(#expr) + ": " + hipGetErrorString(e__);       \
            return MSSPE_ERR_DEVICE;                                        \
        }                                                                   \
    } while (0)

template <typename T>
int launch(const uint64_t *d_packed, size_t total_len, int k, int M, int E, const uint64_t *words, int n,
           void *const *buf, msspe_site *d_sites, uint64_t capacity, uint64_t *d_count, int n_cu, hipStream_t stream,
           std::vector<T> &planes, std::string &err)
{
    constexpr bool narrow = sizeof(T) == 4;
    const int scale = narrow ? 2 : 1;
    const int s = k - E;   // 3' bases start at plane bit s
    const uint32_t lim = narrow ? (s >= 16 ? 0xffffffffu : (1u << (16 + s)) - 1u) : (uint32_t)((1ull << s) - 1ull);
    planes.clear();
    to_planes<T>(words, n, planes);
    T *d_words = (T *)buf[0];
    unsigned long long *d_counts = (unsigned long long *)buf[1];
    BG_TRY(hipMemcpyAsync(d_words, planes.data(), sizeof(T) * planes.size(), hipMemcpyHostToDevice, stream));
    BG_TRY(hipMemsetAsync(d_counts, 0, sizeof(uint64_t) * 2 * (size_t)n, stream));
    const size_t per_word = sizeof(T) + 2 * sizeof(uint32_t);
    const int tile_cap = std::max(4, std::min((int)(kTileBytes / per_word) & ~3, (n + 3) & ~3));
    const size_t lds = (size_t)tile_cap * per_word;
    const uint64_t n_pos = (uint64_t)total_len - (uint64_t)k + 1;   // positions 0 .. L - k (L >= k: the caller)
    const uint32_t n_runs = (uint32_t)((n_pos + kRun - 1) / kRun);
    const unsigned grid = (unsigned)std::min<uint64_t>(n_runs, (uint64_t)std::max(1, n_cu) * kBlocksPerCu);
    const uint32_t max_score = (uint32_t)(M * scale);
    if (d_sites)
        hipLaunchKernelGGL((k_background_sites<T, true>), dim3(grid), dim3(kThreads), lds, stream, d_packed, total_len,
                           k, d_words, n, tile_cap, lim, max_score, scale, n_runs, d_counts, d_sites,
                           (unsigned long long)capacity, (unsigned long long *)d_count);
    else
        hipLaunchKernelGGL((k_background_sites<T, false>), dim3(grid), dim3(kThreads), lds, stream, d_packed,
                           total_len, k, d_words, n, tile_cap, lim, max_score, scale, n_runs, d_counts,
                           (msspe_site *)nullptr, 0ull, (unsigned long long *)nullptr);
    BG_TRY(hipGetLastError());
    return MSSPE_OK;
}

template <typename T>
void launch_slab(const uint64_t *d_packed, size_t total_len, int k, int M, int E, const T *d_words, int n,
                 uint32_t primer_base, uint32_t run_base, uint32_t n_runs, unsigned long long *d_counts,
                 msspe_site *d_sites, uint64_t capacity, uint64_t *d_count, int n_cu, hipStream_t stream)
{
    constexpr bool narrow = sizeof(T) == 4;
    const int scale = narrow ? 2 : 1;
    const int s = k - E;
    const uint32_t lim = narrow ? (s >= 16 ? 0xffffffffu : (1u << (16 + s)) - 1u) : (uint32_t)((1ull << s) - 1ull);
    const size_t per_word = sizeof(T) + 2 * sizeof(uint32_t);
    const int tile_cap = std::max(4, std::min((int)(kTileBytes / per_word) & ~3, (n + 3) & ~3));
    const size_t lds = (size_t)tile_cap * per_word;
    const unsigned grid = (unsigned)std::min<uint64_t>(n_runs, (uint64_t)std::max(1, n_cu) * kBlocksPerCu);
    hipLaunchKernelGGL((k_background_slab<T, true>), dim3(grid), dim3(kThreads), lds, stream, d_packed, total_len, k,
                       d_words + primer_base, n, tile_cap, lim, (uint32_t)(M * scale), scale, n_runs, d_counts,
                       d_sites, (unsigned long long)capacity, (unsigned long long *)d_count, run_base, primer_base);
}

}  // namespace

hipError_t launch_pack_stream(const uint8_t *d_ascii, size_t n_cols, uint64_t *bases, uint64_t *valid,
                              hipStream_t stream)
{
    const size_t words = (n_cols + 31) / 32 + (n_cols + 63) / 64;
    if (!words) return hipSuccess;
    hipLaunchKernelGGL(k_pack_stream, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, d_ascii, n_cols,
                       bases, valid);
    return hipGetLastError();
}

int BackgroundSites::ensure(int slot, size_t bytes, std::string &err)
{
    if (cap_[slot] >= bytes) return MSSPE_OK;
    if (buf_[slot]) (void)hipFree(buf_[slot]);
    buf_[slot] = nullptr;
    cap_[slot] = 0;
    const hipError_t e = hipMalloc(&buf_[slot], bytes ? bytes : 16);
    if (e != hipSuccess) {
        err = std::string("hipMalloc (background sites): ") + hipGetErrorString(e);
        return MSSPE_ERR_DEVICE;
    }
    cap_[slot] = bytes;
    return MSSPE_OK;
}

void BackgroundSites::release()
{
    for (int s = 0; s < 2; ++s) {
        if (buf_[s]) (void)hipFree(buf_[s]);
        buf_[s] = nullptr;
        cap_[s] = 0;
    }
}

uint32_t BackgroundSites::n_runs(size_t total_len, int k)
{
    return (uint32_t)(((uint64_t)total_len - (uint64_t)k + 1 + kRun - 1) / kRun);
}

int BackgroundSites::check(size_t total_len, int k, int max_mismatches, int exact_3p, const uint64_t *words, int n,
                           std::string &err)
{
    if (k < 1 || k > 31) {
        err = "background_sites: unsupported k (need 1 <= k <= 31)";
        return MSSPE_ERR_K;
    }
    if (max_mismatches < 0 || max_mismatches > k || exact_3p < 0 || exact_3p > k) {
        err = "background_sites: max_mismatches and exact_3p must lie in 0..k";
        return MSSPE_ERR_ARG;
    }
    if ((uint64_t)total_len >= (1ull << 32)) {
        err = "background_sites: the stream must be shorter than 2^32 columns";
        return MSSPE_ERR_ARG;
    }
    if (n < 0) {
        err = "background_sites: null argument";
        return MSSPE_ERR_ARG;
    }
    const uint64_t high = ~0ull << (2 * k);
    for (int i = 0; i < n; ++i)
        if (words[i] & high) {
            err = "background_sites: a primer word has bits above 2 k";
            return MSSPE_ERR_ARG;
        }
    return MSSPE_OK;
}

int BackgroundSites::prepare(int k, const uint64_t *words, int n, hipStream_t stream, std::string &err)
{
    const bool narrow = k <= 16;
    int rc;
    if ((rc = ensure(0, (narrow ? 4 : 8) * (size_t)n, err)) || (rc = ensure(1, sizeof(uint64_t) * 2 * (size_t)n, err)))
        return rc;
    w32_.clear();
    w64_.clear();
    if (narrow) {
        to_planes<uint32_t>(words, n, w32_);
        BG_TRY(hipMemcpyAsync(buf_[0], w32_.data(), sizeof(uint32_t) * w32_.size(), hipMemcpyHostToDevice, stream));
    } else {
        to_planes<uint2>(words, n, w64_);
        BG_TRY(hipMemcpyAsync(buf_[0], w64_.data(), sizeof(uint2) * w64_.size(), hipMemcpyHostToDevice, stream));
    }
    return MSSPE_OK;
}

int BackgroundSites::list_slab(const uint64_t *d_packed, size_t total_len, int k, int max_mismatches, int exact_3p,
                               int p0, int p1, uint32_t run0, uint32_t run1, msspe_site *d_sites, uint64_t capacity,
                               uint64_t *d_count, int n_cu, hipStream_t stream, std::string &err)
{
    if (p1 <= p0 || run1 <= run0) return MSSPE_OK;
    unsigned long long *scratch = (unsigned long long *)buf_[1] + 2 * (size_t)p0;   // per-slab counts: not read
    if (k <= 16)
        launch_slab<uint32_t>(d_packed, total_len, k, max_mismatches, exact_3p, (const uint32_t *)buf_[0], p1 - p0,
                              (uint32_t)p0, run0, run1 - run0, scratch, d_sites, capacity, d_count, n_cu, stream);
    else
        launch_slab<uint2>(d_packed, total_len, k, max_mismatches, exact_3p, (const uint2 *)buf_[0], p1 - p0,
                           (uint32_t)p0, run0, run1 - run0, scratch, d_sites, capacity, d_count, n_cu, stream);
    BG_TRY(hipGetLastError());
    return MSSPE_OK;
}

int BackgroundSites::run(const uint64_t *d_packed, size_t total_len, int k, int max_mismatches, int exact_3p,
                         const uint64_t *words, int n, uint64_t *sites_out, msspe_site *d_sites, uint64_t capacity,
                         uint64_t *d_count, int n_cu, hipStream_t stream, std::string &err)
{
    if (k < 1 || k > 31) {
        err = "background_sites: unsupported k (need 1 <= k <= 31)";
        return MSSPE_ERR_K;
    }
    if (max_mismatches < 0 || max_mismatches > k || exact_3p < 0 || exact_3p > k) {
        err = "background_sites: max_mismatches and exact_3p must lie in 0..k";
        return MSSPE_ERR_ARG;
    }
    if ((uint64_t)total_len >= (1ull << 32)) {
        err = "background_sites: the stream must be shorter than 2^32 columns";
        return MSSPE_ERR_ARG;
    }
    if (n < 0 || (d_sites && !d_count)) {
        err = "background_sites: null argument";
        return MSSPE_ERR_ARG;
    }
    const uint64_t high = ~0ull << (2 * k);
    for (int i = 0; i < n; ++i)
        if (words[i] & high) {
            err = "background_sites: a primer word has bits above 2 k";
            return MSSPE_ERR_ARG;
        }
    std::fill(sites_out, sites_out + 2 * (size_t)n, (uint64_t)0);
    if (n == 0 || total_len < (size_t)k) return MSSPE_OK;
    const bool narrow = k <= 16;
    int rc;
    if ((rc = ensure(0, (narrow ? 4 : 8) * (size_t)n, err)) || (rc = ensure(1, sizeof(uint64_t) * 2 * (size_t)n, err)))
        return rc;
    rc = narrow ? launch<uint32_t>(d_packed, total_len, k, max_mismatches, exact_3p, words, n, buf_, d_sites, capacity,
                                   d_count, n_cu, stream, w32_, err)
                : launch<uint2>(d_packed, total_len, k, max_mismatches, exact_3p, words, n, buf_, d_sites, capacity,
                                d_count, n_cu, stream, w64_, err);
    if (rc) return rc;
    BG_TRY(hipMemcpyAsync(sites_out, buf_[1], sizeof(uint64_t) * 2 * (size_t)n, hipMemcpyDeviceToHost, stream));
    BG_TRY(hipStreamSynchronize(stream));   // sites_out is host memory: the call returns with it filled
    return MSSPE_OK;
}

}  // namespace msspe
