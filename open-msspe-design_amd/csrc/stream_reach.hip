// stream_reach.hip -- what turns the stable-site bit planes into reach (engine extension, no reference counterpart:
// include/msspe_hip.h msspe_stream_reach*).
//
// The scored pass leaves two bit planes over the stream's columns (k_site_fold_planes in background_thal.hip): bit p of
// the plus plane for a stable plus-strand site at p, bit q of the minus plane for a stable minus-strand site at q.  A
// plus site reaches the columns [p, p + D - 1]; a minus site reaches DOWN from its window's last column,
// [q + k - D, q + k - 1].  Every kernel here therefore reads the minus plane moved up by k - 1 columns -- the END plane,
// bit e = q + k - 1 -- and the two strands become mirror images: a column b is plus-reached iff the nearest plus bit at
// or below it lies within D - 1 columns (and in b's record), minus-reached iff the nearest end bit at or above it does.
//
// One lane holds one 64-column word, one wave one tile of 4096 columns; "the nearest bit below my word" is a wave prefix
// inside the tile and the tile's carry outside it.
//   k_reach_tiles     the last plus bit and the first end bit of every tile;
//   k_reach_scan      one block, 1024 tiles per step: exclusive running maximum from the left, exclusive running
//                     minimum from the right;
//   k_reach_masks     per word: the masks from the word's own bits smeared by min(D, 64) and from the two carried
//                     neighbours, cut to the record's columns; popcounts; the plane "in a record, reached by neither".
//                     Per-strand gaps need no second pass: on the plus strand every site bit closes the unreached run
//                     below it and the record's end closes the last one, on the minus strand every end bit closes the
//                     run above it and the record's start the first one; a run's other end follows from the carried
//                     neighbour.  A run folds into its record with one 64-bit atomicMax on len << 32 | ~pos, which
//                     orders by length and then by the LOWEST position.
//                     A word that lies in one record is one segment; a word that holds a record boundary walks its
//                     records and handles one segment per record with the same code (empty records have no segment).
//                     A wave that lies in one record adds its sums with one atomic per field; otherwise every lane
//                     (every segment) adds its own.
//   k_reach_gap_tiles / k_reach_gaps   the same carry on the "neither" plane: the last ZERO below a word.  A maximal
//                     run of ones lies in one record (the separator between two records is never set), is seen by the
//                     lane that holds its last bit, and starts behind the last zero below it.
// Positions and sums with D are 64-bit; a tile value is a position + 1 (0: none) or a position (0xffffffff: none), both
// of which fit 32 bits because total_len < 2^32.
#include "stream_reach.hpp"

namespace msspe {
namespace {

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;
constexpr uint32_t kNone = 0xffffffffu;

__device__ __forceinline__ uint64_t low_bits(int n) { return n >= 64 ? ~0ull : (n <= 0 ? 0ull : (1ull << n) - 1ull); }

// the minus plane's word w moved up by k - 1 columns (2 <= k <= 31)
__device__ __forceinline__ uint64_t end_word(const uint64_t *minus, size_t w, int k)
{
    const int sh = k - 1;
    const uint64_t below = w ? minus[w - 1] : 0ull;
    return (minus[w] << sh) | (below >> (64 - sh));
}

// x | x << 1 | ... | x << (n - 1), 1 <= n <= 64 (wave-uniform n)
__device__ __forceinline__ uint64_t smear_up(uint64_t x, int n)
{
    int s = 1;
    for (; 2 * s <= n; s *= 2) x |= x << s;
    if (n > s) x |= x << (n - s);
    return x;
}

__device__ __forceinline__ uint64_t smear_down(uint64_t x, int n)
{
    int s = 1;
    for (; 2 * s <= n; s *= 2) x |= x >> s;
    if (n > s) x |= x >> (n - s);
    return x;
}

// the maximum over the lanes below this one, and the carry
__device__ __forceinline__ uint32_t prefix_max_left(uint32_t v, uint32_t carry, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d);
        if (lane >= d) v = max(v, o);
    }
    const uint32_t ex = (uint32_t)__shfl_up((int)v, 1);
    return lane ? max(ex, carry) : carry;
}

// the minimum over the lanes above this one, and the carry
__device__ __forceinline__ uint32_t suffix_min_right(uint32_t v, uint32_t carry, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_down((int)v, d);
        if (lane + d < 64) v = min(v, o);
    }
    const uint32_t ex = (uint32_t)__shfl_down((int)v, 1);
    return lane < 63 ? min(ex, carry) : carry;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    for (int d = 32; d; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
    for (int d = 32; d; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int d = 32; d; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v)
{
    for (int d = 32; d; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(v >> 32), d);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// the last record that starts at or before pos (starts[0] == 0)
__device__ __forceinline__ int record_of(const uint64_t *starts, int n_records, uint64_t pos)
{
    int lo = 0, hi = n_records;   // the first record that starts behind pos
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= pos) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

__device__ __forceinline__ uint64_t record_end(const uint64_t *starts, int n_records, int r, uint64_t total_len)
{
    return r + 1 < n_records ? starts[r + 1] - 1ull : total_len;
}

__device__ __forceinline__ uint64_t valid_bits(size_t w, size_t total_len)
{
    const uint64_t left = (uint64_t)total_len - 64ull * w;
    return left >= 64 ? ~0ull : low_bits((int)left);
}

__global__ void __launch_bounds__(kThreads) k_reach_tiles(const uint64_t *plus, const uint64_t *minus, size_t nw, int k,
                                                          uint32_t *tile_plus, uint32_t *tile_minus)
{
    const size_t w = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const bool live = w < nw;
    const uint64_t base = 64ull * w;
    const uint64_t p = live ? plus[w] : 0ull, e = live ? end_word(minus, w, k) : 0ull;
    const uint32_t last1 = p ? (uint32_t)(base + 63 - __clzll((long long)p)) + 1u : 0u;
    const uint32_t first = e ? (uint32_t)(base + (__ffsll((unsigned long long)e) - 1)) : kNone;
    const uint32_t tmax = wave_max(last1), tmin = wave_min(first);
    if ((threadIdx.x & 63) == 0 && live) {   // a wave's first word is live where any of its words is
        tile_plus[w >> 6] = tmax;
        tile_minus[w >> 6] = tmin;
    }
}

__global__ void __launch_bounds__(kThreads) k_reach_gap_tiles(const uint64_t *neither, size_t nw, size_t total_len,
                                                              uint32_t *tile_zero)
{
    const size_t w = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const bool live = w < nw;
    const uint64_t base = 64ull * w;
    const uint64_t z = live ? ~neither[w] & valid_bits(w, total_len) : 0ull;
    const uint32_t last1 = z ? (uint32_t)(base + 63 - __clzll((long long)z)) + 1u : 0u;
    const uint32_t tmax = wave_max(last1);
    if ((threadIdx.x & 63) == 0 && live) tile_zero[w >> 6] = tmax;
}

// One pass of k_reach_scan over v[0 .. n) in place.  kMin false: v[i] = max(v[0 .. i)), identity 0; kMin true, walked
// from the right end: v[i] = min(v(i .. n)), identity kNone.  The block takes 1024 elements per step, coalesced, the
// next step's load in flight while this one is scanned: a wave prefix by shuffles, the 16 wave totals through LDS, the
// running carry in a register of every thread.
template <bool kMin>
__device__ __forceinline__ void scan_pass(uint32_t *v, size_t n, uint32_t *s_wave)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t ident = kMin ? kNone : 0u;
    auto op = [](uint32_t x, uint32_t y) { return kMin ? min(x, y) : max(x, y); };
    auto at = [&](size_t g) { return kMin ? n - 1 - g : g; };   // the g-th element in walking order
    uint32_t carry = ident;
    uint32_t cur = (size_t)tid < n ? v[at((size_t)tid)] : ident;
    for (size_t base = 0; base < n; base += kScanThreads) {
        const size_t g = base + (size_t)tid, g_next = g + kScanThreads;
        const uint32_t nxt = g_next < n ? v[at(g_next)] : ident;
        uint32_t incl = cur;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= d) incl = op(incl, o);
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = carry, total = carry;
        for (int i = 0; i < kScanThreads / 64; ++i) {
            const uint32_t t = s_wave[i];
            if (i < wave) before = op(before, t);
            total = op(total, t);
        }
        const uint32_t ex = (uint32_t)__shfl_up((int)incl, 1);
        if (g < n) v[at(g)] = lane ? op(before, ex) : before;
        carry = total;
        cur = nxt;
        __syncthreads();   // s_wave is written again in the next step
    }
}

// in place: a[i] = max(a[0 .. i)), and with b, b[i] = min(b(i .. n_tiles))
__global__ void __launch_bounds__(kScanThreads) k_reach_scan(uint32_t *a, uint32_t *b, size_t n_tiles)
{
    __shared__ uint32_t s_wave[kScanThreads / 64];
    scan_pass<false>(a, n_tiles, s_wave);
    if (b) scan_pass<true>(b, n_tiles, s_wave);
}

// what one segment adds to its record
struct Part {
    uint32_t c[6];   // sites plus / minus, reached plus / minus / either / both
    unsigned long long gap_plus, gap_minus;
};

__device__ __forceinline__ void fold_gap(unsigned long long &key, uint64_t len, uint64_t pos)
{
    const unsigned long long v = ((unsigned long long)len << 32) | (unsigned long long)(uint32_t)~(uint32_t)pos;
    key = v > key ? v : key;
}

__device__ __forceinline__ void flush(const Part &p, ReachAccum *acc)
{
    uint32_t *c = &acc->sites_plus;
    for (int i = 0; i < 6; ++i)
        if (p.c[i]) atomicAdd(&c[i], p.c[i]);
    if (p.gap_plus) atomicMax(&acc->gap_plus, p.gap_plus);
    if (p.gap_minus) atomicMax(&acc->gap_minus, p.gap_minus);
}

// Columns [base + lo, base + hi) of one word, all of them columns of the record [s, e): pw / ew are the word's plus and
// end bits, prev1 the last plus bit below the word (position + 1, 0: none), next the first end bit above it.
__device__ __forceinline__ void reach_segment(uint64_t base, int lo, int hi, uint64_t s, uint64_t e, uint64_t pw,
                                              uint64_t ew, uint32_t prev1, uint32_t next, uint64_t D, int dm,
                                              Part &out, uint64_t &neither)
{
    const uint64_t seg = low_bits(hi) & ~low_bits(lo);
    const uint64_t ps = pw & seg, es = ew & seg;
    const bool starts_here = base + (uint64_t)lo == s, ends_here = base + (uint64_t)hi == e;
    // a carried neighbour counts when it lies in this record: the segment then runs to the word's edge on that side
    const bool have_prev = lo == 0 && (uint64_t)prev1 > s;
    const bool have_next = !ends_here && next != kNone && (uint64_t)next < e;
    uint64_t plus = smear_up(ps, dm), minus = smear_down(es, dm);
    if (have_prev) {   // columns up to prev + D - 1
        const long long c = (long long)prev1 - 1 + (long long)D - (long long)base;
        plus |= low_bits(c > 64 ? 64 : (c < 0 ? 0 : (int)c));
    }
    if (have_next) {   // columns from next - D + 1 on
        const long long f = (long long)next - (long long)D + 1 - (long long)base;
        minus |= ~low_bits(f > 64 ? 64 : (f < 0 ? 0 : (int)f));
    }
    plus &= seg;
    minus &= seg;
    out.c[0] += (uint32_t)__popcll(ps);
    out.c[1] += (uint32_t)__popcll(es);
    out.c[2] += (uint32_t)__popcll(plus);
    out.c[3] += (uint32_t)__popcll(minus);
    out.c[4] += (uint32_t)__popcll(plus | minus);
    out.c[5] += (uint32_t)__popcll(plus & minus);
    neither |= seg & ~(plus | minus);
    {   // plus strand: a site at p closes the run [last + D, p) (from s without a site before it), the record's end the last
        bool have = have_prev;
        uint64_t last = (uint64_t)prev1 - 1ull;
        for (uint64_t m = ps; m; m &= m - 1ull) {
            const uint64_t p = base + (uint64_t)(__ffsll((unsigned long long)m) - 1);
            const uint64_t from = have ? last + D : s;
            if (p > from) fold_gap(out.gap_plus, p - from, from);
            last = p;
            have = true;
        }
        if (ends_here) {
            const uint64_t from = have ? last + D : s;
            if (e > from) fold_gap(out.gap_plus, e - from, from);
        }
    }
    {   // minus strand: an end at q closes the run (q, nxt - D] above it (up to e without an end above), the record's
        // start the first
        bool have = have_next;
        long long nxt = (long long)next;
        for (uint64_t m = es; m;) {
            const int j = 63 - __clzll((long long)m);
            m &= ~(1ull << j);
            const long long q = (long long)(base + (uint64_t)j);
            const long long to = have ? nxt - (long long)D + 1 : (long long)e;   // the first column behind the run
            if (to > q + 1) fold_gap(out.gap_minus, (uint64_t)(to - q - 1), (uint64_t)(q + 1));
            nxt = q;
            have = true;
        }
        if (starts_here) {
            const long long to = have ? nxt - (long long)D + 1 : (long long)e;
            if (to > (long long)s) fold_gap(out.gap_minus, (uint64_t)(to - (long long)s), s);
        }
    }
}

__global__ void __launch_bounds__(kThreads) k_reach_masks(const uint64_t *plus, const uint64_t *minus, size_t nw,
                                                          size_t total_len, int k, uint64_t D, const uint64_t *starts,
                                                          int n_records, const uint32_t *tile_plus,
                                                          const uint32_t *tile_minus, ReachAccum *acc,
                                                          uint64_t *neither_plane)
{
    const size_t w = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = w < nw;
    if (!__ballot(live)) return;   // wave-uniform; below, lane 0 is live
    const size_t tile = w >> 6;    // the same for the whole wave
    const uint64_t base = 64ull * w;
    const uint64_t pw = live ? plus[w] : 0ull, ew = live ? end_word(minus, w, k) : 0ull;
    const uint32_t last1 = pw ? (uint32_t)(base + 63 - __clzll((long long)pw)) + 1u : 0u;
    const uint32_t first = ew ? (uint32_t)(base + (__ffsll((unsigned long long)ew) - 1)) : kNone;
    const uint32_t prev1 = prefix_max_left(last1, tile_plus[tile], lane);
    const uint32_t next = suffix_min_right(first, tile_minus[tile], lane);
    const int dm = D < 64 ? (int)D : 64;

    // The record of the wave's first column, searched once for the whole wave (a wave-uniform address: scalar loads).
    // Where the wave's last column lies in that record too, every word is one segment of it and no lane searches.
    const uint64_t wave_base = 64ull * ((uint64_t)blockIdx.x * kThreads +
                                        (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u)));
    const uint64_t wave_end = wave_base + kReachTileColumns < (uint64_t)total_len ? wave_base + kReachTileColumns
                                                                                  : (uint64_t)total_len;
    const int rw = record_of(starts, n_records, wave_base);
    const uint64_t rec_s = starts[rw], rec_e = record_end(starts, n_records, rw, total_len);
    int r0 = rw;
    uint64_t s0 = rec_s, e0 = rec_e, wend = 0;
    bool single = false;   // every column of the word is a column of record r0
    if (live) {
        wend = base + 64 < (uint64_t)total_len ? base + 64 : (uint64_t)total_len;
        if (wave_end > rec_e) {
            r0 = record_of(starts, n_records, base);
            s0 = starts[r0];
            e0 = record_end(starts, n_records, r0, total_len);
        }
        single = base < e0 && wend <= e0;
    }
    Part part = {};
    uint64_t neither = 0ull;
    if (single) reach_segment(base, 0, (int)(wend - base), s0, e0, pw, ew, prev1, next, D, dm, part, neither);
    const int rf = __builtin_amdgcn_readfirstlane(r0);
    if (__all(!live || (single && r0 == rf))) {
        for (int i = 0; i < 6; ++i) part.c[i] = wave_sum(part.c[i]);
        part.gap_plus = wave_max64(part.gap_plus);
        part.gap_minus = wave_max64(part.gap_minus);
        if (lane == 0) flush(part, &acc[rf]);
    } else if (single) {
        flush(part, &acc[r0]);
    } else if (live) {   // a record boundary in the word: one segment per record that has columns here
        uint64_t col = base;
        int r = r0;
        while (col < wend) {
            const uint64_t s = starts[r], e = record_end(starts, n_records, r, total_len);
            if (col < e) {
                const uint64_t hi = e < wend ? e : wend;
                Part p = {};
                reach_segment(base, (int)(col - base), (int)(hi - base), s, e, pw, ew, prev1, next, D, dm, p, neither);
                flush(p, &acc[r]);
                col = hi;
            } else {   // col is the separator behind record r
                if (r + 1 >= n_records) break;
                ++r;
                col = starts[r];
            }
        }
    }
    if (live) neither_plane[w] = neither;
}

__global__ void __launch_bounds__(kThreads) k_reach_gaps(const uint64_t *neither, size_t nw, size_t total_len,
                                                         const uint64_t *starts, int n_records,
                                                         const uint32_t *tile_zero, ReachAccum *acc)
{
    const size_t w = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = w < nw;
    if (!__ballot(live)) return;   // wave-uniform
    const uint64_t base = 64ull * w;
    const uint64_t zw = live ? neither[w] : 0ull;
    const uint64_t above = (live && w + 1 < nw) ? neither[w + 1] & 1ull : 0ull;
    const uint64_t zeros = live ? ~zw & valid_bits(w, total_len) : 0ull;
    const uint32_t last1 = zeros ? (uint32_t)(base + 63 - __clzll((long long)zeros)) + 1u : 0u;
    const uint64_t from_below = prefix_max_left(last1, tile_zero[w >> 6], lane);   // the column behind the last zero below
    for (uint64_t ends = zw & ~((zw >> 1) | (above << 63)); ends; ends &= ends - 1ull) {
        const int j = __ffsll((unsigned long long)ends) - 1;
        const uint64_t zb = ~zw & low_bits(j + 1);
        const uint64_t from = zb ? base + (uint64_t)(63 - __clzll((long long)zb)) + 1ull : from_below;
        const uint64_t len = base + (uint64_t)j + 1ull - from;
        unsigned long long key = 0ull;
        fold_gap(key, len, from);
        atomicMax(&acc[record_of(starts, n_records, from)].gap_either, key);
    }
}

inline unsigned grid_for(size_t nw) { return (unsigned)((nw + kThreads - 1) / kThreads); }

}  // namespace

hipError_t launch_reach_tiles(const uint64_t *d_plus, const uint64_t *d_minus, size_t total_len, int k,
                              uint32_t *d_tile_plus, uint32_t *d_tile_minus, hipStream_t stream)
{
    const size_t nw = reach_plane_words(total_len);
    if (!nw) return hipSuccess;
    hipLaunchKernelGGL(k_reach_tiles, dim3(grid_for(nw)), dim3(kThreads), 0, stream, d_plus, d_minus, nw, k,
                       d_tile_plus, d_tile_minus);
    return hipGetLastError();
}

hipError_t launch_reach_scan(uint32_t *d_tile_max, uint32_t *d_tile_min, size_t n_tiles, hipStream_t stream)
{
    if (!n_tiles) return hipSuccess;
    hipLaunchKernelGGL(k_reach_scan, dim3(1), dim3(kScanThreads), 0, stream, d_tile_max, d_tile_min, n_tiles);
    return hipGetLastError();
}

hipError_t launch_reach_masks(const uint64_t *d_plus, const uint64_t *d_minus, size_t total_len, int k, uint64_t reach,
                              const uint64_t *d_starts, int n_records, const uint32_t *d_tile_plus,
                              const uint32_t *d_tile_minus, ReachAccum *d_acc, uint64_t *d_neither,
                              hipStream_t stream)
{
    const size_t nw = reach_plane_words(total_len);
    if (!nw) return hipSuccess;
    hipLaunchKernelGGL(k_reach_masks, dim3(grid_for(nw)), dim3(kThreads), 0, stream, d_plus, d_minus, nw, total_len, k,
                       reach, d_starts, n_records, d_tile_plus, d_tile_minus, d_acc, d_neither);
    return hipGetLastError();
}

hipError_t launch_reach_gap_tiles(const uint64_t *d_neither, size_t total_len, uint32_t *d_tile_zero,
                                  hipStream_t stream)
{
    const size_t nw = reach_plane_words(total_len);
    if (!nw) return hipSuccess;
    hipLaunchKernelGGL(k_reach_gap_tiles, dim3(grid_for(nw)), dim3(kThreads), 0, stream, d_neither, nw, total_len,
                       d_tile_zero);
    return hipGetLastError();
}

hipError_t launch_reach_gaps(const uint64_t *d_neither, size_t total_len, const uint64_t *d_starts, int n_records,
                             const uint32_t *d_tile_zero, ReachAccum *d_acc, hipStream_t stream)
{
    const size_t nw = reach_plane_words(total_len);
    if (!nw) return hipSuccess;
    hipLaunchKernelGGL(k_reach_gaps, dim3(grid_for(nw)), dim3(kThreads), 0, stream, d_neither, nw, total_len, d_starts,
                       n_records, d_tile_zero, d_acc);
    return hipGetLastError();
}

}  // namespace msspe
