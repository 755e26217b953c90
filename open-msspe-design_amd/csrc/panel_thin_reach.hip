// panel_thin_reach.hip -- a primer panel thinned on target reach (engine extension, no reference counterpart:
// include/msspe_hip.h msspe_panel_thin_reach*).
//
// The scored pass leaves one key per stable site, pos << 32 | strand << 31 | primer (k_site_fold_keys in
// background_thal.hip).  R_p, the columns primer p reaches, is the union over p's keys of [pos, min(pos + D, e_r) - 1]
// (plus) and [max(pos + k - D, s_r), pos + k - 1] (minus); the rule here is the greedy set cover over those column sets.
//
// Prepare, once per call.
//   k_key_intervals   one lane per key: its record by binary search, the clipped interval as primer << 32 | lo with hi
//                     as the value; rocPRIM's radix sort orders the pairs by (primer, lo).
//   k_max_tiles / k_tile_scan<MaxOp> / k_clip   an exclusive running maximum of primer << 32 | (hi + 1): where its top
//                     half is the lane's own primer, its low half is the first column no earlier interval of the primer
//                     has taken, and lo' = max(lo, that).  hi is NOT monotone in the sorted order (a plus interval cut
//                     at its record's end can hold a later minus interval), hence the maximum and not the neighbour.
//   k_flag_tiles / k_tile_scan<SumOp> / k_compact   intervals with lo' > hi leave, the others keep their order;
//   k_primer_first    one lane per primer: where its run starts.
// After it every R_p is a disjoint union of [lo', hi], |R_p| is a sum of lengths, and with the covered columns C as a
// bit plane, |R_p \ C| = sum of len - (rank_C(hi + 1) - rank_C(lo')).
//
// A round is five launches behind a done word, 16 rounds per read of it (panel_thin.hip's form):
//   k_reach_pick      one block: the live primer of greatest gain << 32 | ~p; below min_gain the loop is done;
//   k_reach_apply     C |= the pick's intervals, a wave per interval with lanes over words; the gains are zeroed;
//   k_plane_tiles     per word the popcounts before it in its tile of 1024 words, per tile its sum;
//   k_tile_scan<SumOp>  one block: the exclusive sums of the tiles;
//   k_reach_gain      one lane per interval: two rank reads, two edge words, a segmented wave sum by primer, one
//                     atomic per (wave, primer).  gain[p] == |R_p \ C| for every live p before every pick.
// The same gain kernel without a plane gives |R_p|; k_reach_apply_flagged ORs the forced primers' intervals first and
// everybody's last (|union of all R_p|), and the last tile scan's total is the popcount of the plane either time.
// k_keys_to_planes ORs the kept primers' keys into the two site planes the reach report starts from.
// Every column and count fits 32 bits because total_len < 2^32; no kernel here uses scratch.
#include "panel_thin_reach.hpp"

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <vector>

namespace msspe {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;            // elements per block of the tile kernels and per step of the one-block scan
constexpr int kRoundsPerBatch = 16;    // rounds enqueued between two reads of the "done" word
constexpr unsigned kApplyBlocks = 512;

struct ReachThinState {
    uint32_t done;       // 1: a round found no gain of min_gain or more (the launches that follow return at once)
    uint32_t rounds;     // rounds that ran: the picks and the one that stopped
    uint32_t n_picked;
    uint32_t pick;       // of the current round
};

struct SumOp {
    using T = uint32_t;
    __device__ static T id() { return 0u; }
    __device__ static T op(T a, T b) { return a + b; }
    __device__ static T up(T v, int d) { return (T)__shfl_up((int)v, d); }
};

struct MaxOp {
    using T = unsigned long long;
    __device__ static T id() { return 0ull; }
    __device__ static T op(T a, T b) { return a > b ? a : b; }
    __device__ static T up(T v, int d)
    {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d), hi = (uint32_t)__shfl_up((int)(v >> 32), d);
        return ((T)hi << 32) | lo;
    }
};

__device__ __forceinline__ uint64_t low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }

// The exclusive prefix of v over the block's kTile threads, and the block's total.  Every thread calls it.
template <class Op>
__device__ __forceinline__ typename Op::T block_exclusive(typename Op::T v, typename Op::T *s_wave,
                                                          typename Op::T &total)
{
    using T = typename Op::T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const T o = Op::up(incl, d);
        if (lane >= d) incl = Op::op(incl, o);
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T before = Op::id();
    total = Op::id();
    for (int i = 0; i < kTile / 64; ++i) {
        const T t = s_wave[i];
        if (i < wave) before = Op::op(before, t);
        total = Op::op(total, t);
    }
    const T ex = Op::up(incl, 1);
    __syncthreads();   // s_wave is written again by the caller's next step
    return lane ? Op::op(before, ex) : before;
}

// One block, in place: v[i] = op over v[0 .. i), and v[n] = op over all of them.
template <class Op>
__global__ void __launch_bounds__(kTile) k_tile_scan(typename Op::T *v, size_t n, const ReachThinState *st)
{
    using T = typename Op::T;
    if (st && st->done) return;
    __shared__ T s_wave[kTile / 64];
    T carry = Op::id();
    for (size_t base = 0; base < n; base += kTile) {
        const size_t i = base + threadIdx.x;
        const T x = i < n ? v[i] : Op::id();
        T total;
        const T ex = block_exclusive<Op>(x, s_wave, total);
        if (i < n) v[i] = Op::op(carry, ex);
        carry = Op::op(carry, total);
    }
    if (threadIdx.x == 0) v[n] = carry;
}

// ---- prepare ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_key_intervals(const uint64_t *keys, uint32_t m, const uint64_t *starts,
                                                            int n_records, uint64_t total_len, uint32_t k, uint64_t D,
                                                            uint64_t *skey, uint32_t *shi)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    const uint64_t key = keys[i], pos = key >> 32;
    int lo = 0, hi = n_records;   // the first record that starts behind pos
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= pos) lo = mid + 1;
        else hi = mid;
    }
    const int r = lo - 1;         // starts[0] == 0: r >= 0
    const uint64_t s = starts[r], e = r + 1 < n_records ? starts[r + 1] - 1ull : total_len;
    uint64_t a, b;
    if (!((key >> 31) & 1ull)) {
        a = pos;
        b = (pos + D < e ? pos + D : e) - 1ull;
    } else {
        const uint64_t end = pos + k;
        a = end > s + D ? end - D : s;
        b = end - 1ull;
    }
    skey[i] = ((key & 0x7fffffffull) << 32) | a;
    shi[i] = (uint32_t)b;
}

__global__ void __launch_bounds__(kTile) k_max_tiles(const uint64_t *skey, const uint32_t *shi, uint32_t m,
                                                     unsigned long long *excl, unsigned long long *tiles)
{
    __shared__ unsigned long long s_wave[kTile / 64];
    const uint32_t i = blockIdx.x * kTile + threadIdx.x;
    const unsigned long long v = i < m ? (skey[i] & 0xffffffff00000000ull) | ((unsigned long long)shi[i] + 1ull) : 0ull;
    unsigned long long total;
    const unsigned long long ex = block_exclusive<MaxOp>(v, s_wave, total);
    if (i < m) excl[i] = ex;
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kThreads) k_clip(const uint64_t *skey, uint32_t m, const unsigned long long *excl,
                                                   const unsigned long long *tiles, uint32_t *lo2)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    const uint64_t key = skey[i];
    const unsigned long long a = excl[i], b = tiles[i / kTile], before = a > b ? a : b;
    uint32_t lo = (uint32_t)key;
    if ((before >> 32) == (key >> 32)) lo = max(lo, (uint32_t)before);   // an earlier interval of the same primer
    lo2[i] = lo;
}

__global__ void __launch_bounds__(kTile) k_flag_tiles(const uint32_t *lo2, const uint32_t *shi, uint32_t m,
                                                      uint32_t *within, uint32_t *tiles)
{
    __shared__ uint32_t s_wave[kTile / 64];
    const uint32_t i = blockIdx.x * kTile + threadIdx.x;
    const uint32_t v = i < m && lo2[i] <= shi[i] ? 1u : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive<SumOp>(v, s_wave, total);
    if (i < m) within[i] = ex;
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kThreads) k_compact(const uint64_t *skey, const uint32_t *lo2, const uint32_t *shi,
                                                      uint32_t m, const uint32_t *within, const uint32_t *tiles,
                                                      uint32_t *prim, uint32_t *iv_lo, uint32_t *iv_hi)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    const uint32_t lo = lo2[i], hi = shi[i];
    if (lo > hi) return;
    const uint32_t at = tiles[i / kTile] + within[i];   // at <= i
    prim[at] = (uint32_t)(skey[i] >> 32);
    iv_lo[at] = lo;
    iv_hi[at] = hi;
}

// first[p] = the first interval of a primer >= p, for p in [0, n]
__global__ void __launch_bounds__(kThreads) k_primer_first(const uint32_t *prim, uint32_t mi, int n, uint32_t *first)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p > n) return;
    uint32_t lo = 0, hi = mi;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (prim[mid] < (uint32_t)p) lo = mid + 1;
        else hi = mid;
    }
    first[p] = lo;
}

// ---- the cover -------------------------------------------------------------------------------------------------------
// C |= [lo, hi]: the wave's lanes over the interval's words
__device__ __forceinline__ void or_interval(uint64_t *C, uint32_t lo, uint32_t hi, int lane)
{
    const uint32_t wl = lo >> 6, wh = hi >> 6;   // < 2^26
    for (uint32_t w = wl + (uint32_t)lane; w <= wh; w += 64) {
        uint64_t mask = ~0ull;
        if (w == wl) mask &= ~low_bits((int)(lo & 63));
        if (w == wh) mask &= low_bits((int)(hi & 63) + 1);
        atomicOr((unsigned long long *)&C[w], (unsigned long long)mask);
    }
}

// the intervals of the primers whose flag is set (all of them without flags): a wave per interval
__global__ void __launch_bounds__(kThreads) k_reach_apply_flagged(const uint32_t *prim, const uint32_t *iv_lo,
                                                                  const uint32_t *iv_hi, uint32_t mi,
                                                                  const uint8_t *flag, uint64_t *C)
{
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * (kThreads / 64);
    for (uint32_t i = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); i < mi; i += waves)   // wave-uniform
        if (!flag || flag[prim[i]]) or_interval(C, iv_lo[i], iv_hi[i], lane);
}

// One block: the live primer of greatest (gain, lowest index).  Below min_gain (or nobody live) the loop is done.
__global__ void __launch_bounds__(kThreads) k_reach_pick(const uint32_t *gain, uint8_t *live, int n, uint32_t min_gain,
                                                         uint32_t *order, uint32_t *gains, ReachThinState *st)
{
    if (st->done) return;
    __shared__ unsigned long long skey[kThreads / 64];
    const int tid = threadIdx.x;
    unsigned long long key = 0;   // a live primer's key is never 0: its low half is 0xFFFFFFFF - p with p < 2^31
    for (int p = tid; p < n; p += kThreads)
        if (live[p]) key = MaxOp::op(key, (unsigned long long)gain[p] << 32 | (0xFFFFFFFFu - (uint32_t)p));
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, o), hi = (uint32_t)__shfl_xor((int)(key >> 32), o);
        key = MaxOp::op(key, ((unsigned long long)hi << 32) | lo);
    }
    if ((tid & 63) == 0) skey[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kThreads / 64; ++w) key = MaxOp::op(key, skey[w]);
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
        }
    }
}

// C |= the pick's intervals; the gains are zeroed for the gain kernel that follows
__global__ void __launch_bounds__(kThreads) k_reach_apply(const uint32_t *first, const uint32_t *iv_lo,
                                                          const uint32_t *iv_hi, uint64_t *C, uint32_t *gain, int n,
                                                          const ReachThinState *st)
{
    if (st->done) return;
    const int threads = (int)(gridDim.x * kThreads);
    for (int p = (int)(blockIdx.x * kThreads + threadIdx.x); p < n; p += threads) gain[p] = 0u;
    const int lane = threadIdx.x & 63;
    const uint32_t pick = st->pick, end = first[pick + 1], waves = gridDim.x * (kThreads / 64);
    for (uint32_t i = first[pick] + blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); i < end; i += waves)
        or_interval(C, iv_lo[i], iv_hi[i], lane);
}

// within[w] = the set bits of the tile's words before w, tiles[t] = the set bits of tile t
__global__ void __launch_bounds__(kTile) k_plane_tiles(const uint64_t *C, uint32_t nw, uint32_t *within,
                                                       uint32_t *tiles, const ReachThinState *st)
{
    if (st && st->done) return;
    __shared__ uint32_t s_wave[kTile / 64];
    const uint32_t w = blockIdx.x * kTile + threadIdx.x;
    const uint32_t v = w < nw ? (uint32_t)__popcll(C[w]) : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive<SumOp>(v, s_wave, total);
    if (w < nw) within[w] = ex;
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// out[p] += the columns of p's intervals that C does not hold (kPlain: all of them): one lane per interval, the sums
// of a wave's lanes with one primer -- a run, the intervals are in primer order -- through one atomic
template <bool kPlain>
__global__ void __launch_bounds__(kThreads) k_reach_gain(const uint32_t *prim, const uint32_t *iv_lo,
                                                         const uint32_t *iv_hi, uint32_t mi, const uint64_t *C,
                                                         const uint32_t *within, const uint32_t *tiles,
                                                         const uint8_t *live, uint32_t *out, const ReachThinState *st)
{
    if (!kPlain && st->done) return;
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = i < mi;
    const uint32_t p = in ? prim[i] : 0xffffffffu;
    uint32_t v = 0;
    if (in && (kPlain || live[p])) {
        const uint32_t lo = iv_lo[i], hi = iv_hi[i];
        v = hi - lo + 1u;
        if (!kPlain) {
            const uint32_t wl = lo >> 6, wh = hi >> 6;
            const uint32_t below = tiles[wl / kTile] + within[wl] + (uint32_t)__popcll(C[wl] & low_bits((int)(lo & 63)));
            const uint32_t upto = tiles[wh / kTile] + within[wh] +
                                  (uint32_t)__popcll(C[wh] & low_bits((int)(hi & 63) + 1));
            v -= upto - below;
        }
    }
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d), op = (uint32_t)__shfl_up((int)p, d);
        if (lane >= d && op == p) v += o;
    }
    const uint32_t next = (uint32_t)__shfl_down((int)p, 1);
    if (in && v && (lane == 63 || next != p)) atomicAdd(&out[p], v);
}

// the kept primers' keys into the site planes
__global__ void __launch_bounds__(kThreads) k_keys_to_planes(const uint64_t *keys, uint32_t m, const uint8_t *keep,
                                                             uint64_t *plus, uint64_t *minus)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    const uint64_t key = keys[i], pos = key >> 32;
    if (!keep[(uint32_t)key & 0x7fffffffu]) return;
    uint64_t *plane = (key >> 31) & 1ull ? minus : plus;
    atomicOr((unsigned long long *)&plane[pos >> 6], 1ull << (pos & 63));
}

inline unsigned blocks_of(size_t n, int per) { return (unsigned)((n + (size_t)per - 1) / (size_t)per); }

#define REACH_TRY(expr)                                                                   \
    do {                                                                                  \
        hipError_t e__ = (expr);                                                          \
        if (e__ != hipSuccess) {                                                          \
            err = std::string("panel thin reach, " #expr ": ") + hipGetErrorString(e__);  \
            return MSSPE_ERR_DEVICE;                                                      \
        }                                                                                 \
    } while (0)

}  // namespace

int PanelThinReach::ensure(int slot, size_t bytes, std::string &err)
{
    if (cap_[slot] >= bytes && buf_[slot]) return MSSPE_OK;
    if (buf_[slot]) (void)hipFree(buf_[slot]);
    buf_[slot] = nullptr;
    cap_[slot] = 0;
    const hipError_t e = hipMalloc(&buf_[slot], bytes ? bytes : 16);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        buf_[slot] = nullptr;
        err = std::string("hipMalloc (panel thin reach): ") + hipGetErrorString(e);
        return MSSPE_ERR_NOMEM;
    }
    cap_[slot] = bytes;
    return MSSPE_OK;
}

void PanelThinReach::release()
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
}

void PanelThinReach::reset()
{
    sites_ = intervals_ = rounds_ = 0;
    for (auto &p : phase_us_) p = 0;
    reported_ = false;
}

int PanelThinReach::run(const uint64_t *d_keys, uint32_t m, int n, size_t total_len, int k, uint64_t reach,
                        const uint64_t *d_starts, int n_records, uint64_t *d_cover, uint64_t *d_plus,
                        uint64_t *d_minus, uint32_t min_gain, uint8_t *keep_out, uint32_t *order_out,
                        uint32_t *gain_out, int *n_picked_out, uint32_t *reach_out, long long *reached_all_out,
                        long long *reached_kept_out, hipStream_t stream, std::string &err)
{
    reset();
    sites_ = m;
    const size_t nw = (total_len + 63) / 64;
    const size_t nt_plane = (nw + kTile - 1) / kTile, nt_iv = ((size_t)m + kTile - 1) / kTile;
    const size_t mm = std::max<size_t>(m, 1);
    unsigned end_bit = 33;   // lo, then the primer's bits
    while (end_bit < 63 && ((uint64_t)(n - 1) >> (end_bit - 32))) ++end_bit;
    size_t temp_bytes = 0;
    if (m) {
        uint64_t *nk = nullptr;
        uint32_t *nv = nullptr;
        REACH_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, nk, nk, nv, nv, (size_t)m, 0u, end_bit, stream));
    }
    // a buffer is freed only with the stream idle: every call returns behind a synchronisation
    int rc;
    if ((rc = ensure(kSortIn, sizeof(uint64_t) * mm, err)) || (rc = ensure(kSortOut, sizeof(uint64_t) * mm, err)) ||
        (rc = ensure(kHiIn, sizeof(uint32_t) * mm, err)) || (rc = ensure(kHiOut, sizeof(uint32_t) * mm, err)) ||
        (rc = ensure(kExcl, sizeof(uint64_t) * mm, err)) || (rc = ensure(kLo, sizeof(uint32_t) * mm, err)) ||
        (rc = ensure(kWithin, sizeof(uint32_t) * std::max(mm, nw), err)) ||
        (rc = ensure(kTiles, sizeof(uint64_t) * (std::max(nt_plane, nt_iv) + 2), err)) ||
        (rc = ensure(kPrim, sizeof(uint32_t) * mm, err)) || (rc = ensure(kIvLo, sizeof(uint32_t) * mm, err)) ||
        (rc = ensure(kIvHi, sizeof(uint32_t) * mm, err)) ||
        (rc = ensure(kFirst, sizeof(uint32_t) * ((size_t)n + 1), err)) ||
        (rc = ensure(kGain, sizeof(uint32_t) * (size_t)n, err)) ||
        (rc = ensure(kReach, sizeof(uint32_t) * (size_t)n, err)) || (rc = ensure(kLive, (size_t)n, err)) ||
        (rc = ensure(kFlag, (size_t)n, err)) || (rc = ensure(kOrder, 2 * sizeof(uint32_t) * (size_t)n, err)) ||
        (rc = ensure(kState, sizeof(ReachThinState), err)) || (rc = ensure(kTemp, temp_bytes, err)))
        return rc;
    for (auto &e : ev_)
        if (!e) REACH_TRY(hipEventCreate(&e));
    uint64_t *skey_in = (uint64_t *)buf_[kSortIn], *skey = (uint64_t *)buf_[kSortOut];
    uint32_t *shi_in = (uint32_t *)buf_[kHiIn], *shi = (uint32_t *)buf_[kHiOut], *lo2 = (uint32_t *)buf_[kLo];
    unsigned long long *excl = (unsigned long long *)buf_[kExcl], *tiles64 = (unsigned long long *)buf_[kTiles];
    uint32_t *within = (uint32_t *)buf_[kWithin], *tiles32 = (uint32_t *)buf_[kTiles];
    uint32_t *prim = (uint32_t *)buf_[kPrim], *iv_lo = (uint32_t *)buf_[kIvLo], *iv_hi = (uint32_t *)buf_[kIvHi];
    uint32_t *first = (uint32_t *)buf_[kFirst], *d_gain = (uint32_t *)buf_[kGain], *d_reach = (uint32_t *)buf_[kReach];
    uint32_t *d_order = (uint32_t *)buf_[kOrder], *d_gains = d_order + n;
    uint8_t *d_live = (uint8_t *)buf_[kLive], *d_flag = (uint8_t *)buf_[kFlag];
    ReachThinState *st = (ReachThinState *)buf_[kState];

    // (1) prepare: the keys' intervals, sorted, made disjoint within each primer, compacted
    REACH_TRY(hipEventRecord(ev_[0], stream));
    uint32_t mi = 0;
    if (m) {
        hipLaunchKernelGGL(k_key_intervals, dim3(blocks_of(m, kThreads)), dim3(kThreads), 0, stream, d_keys, m, d_starts,
                           n_records, (uint64_t)total_len, (uint32_t)k, reach, skey_in, shi_in);
        REACH_TRY(hipGetLastError());
        REACH_TRY(rocprim::radix_sort_pairs(buf_[kTemp], temp_bytes, skey_in, skey, shi_in, shi, (size_t)m, 0u, end_bit,
                                            stream));
        hipLaunchKernelGGL(k_max_tiles, dim3((unsigned)nt_iv), dim3(kTile), 0, stream, skey, shi, m, excl, tiles64);
        hipLaunchKernelGGL(k_tile_scan<MaxOp>, dim3(1), dim3(kTile), 0, stream, tiles64, nt_iv,
                           (const ReachThinState *)nullptr);
        hipLaunchKernelGGL(k_clip, dim3(blocks_of(m, kThreads)), dim3(kThreads), 0, stream, skey, m, excl, tiles64, lo2);
        hipLaunchKernelGGL(k_flag_tiles, dim3((unsigned)nt_iv), dim3(kTile), 0, stream, lo2, shi, m, within, tiles32);
        hipLaunchKernelGGL(k_tile_scan<SumOp>, dim3(1), dim3(kTile), 0, stream, tiles32, nt_iv,
                           (const ReachThinState *)nullptr);
        REACH_TRY(hipGetLastError());
        REACH_TRY(hipMemcpyAsync(&mi, tiles32 + nt_iv, sizeof mi, hipMemcpyDeviceToHost, stream));
        REACH_TRY(hipStreamSynchronize(stream));
        if (mi == 0 || mi > m) {
            err = "panel thin reach: the intervals do not add up";
            return MSSPE_ERR_DEVICE;
        }
        hipLaunchKernelGGL(k_compact, dim3(blocks_of(m, kThreads)), dim3(kThreads), 0, stream, skey, lo2, shi, m, within,
                           tiles32, prim, iv_lo, iv_hi);
        hipLaunchKernelGGL(k_primer_first, dim3(blocks_of((size_t)n + 1, kThreads)), dim3(kThreads), 0, stream, prim, mi,
                           n, first);
        REACH_TRY(hipGetLastError());
    }
    intervals_ = mi;
    REACH_TRY(hipEventRecord(ev_[1], stream));

    // (2) |R_p|, the forced primers' columns, the first gains
    std::vector<uint8_t> live((size_t)n), flag((size_t)n);
    bool any_forced = false;
    for (int p = 0; p < n; ++p) {
        flag[(size_t)p] = keep_out[p] ? 1 : 0;
        live[(size_t)p] = keep_out[p] ? 0 : 1;
        any_forced = any_forced || keep_out[p];
    }
    REACH_TRY(hipMemsetAsync(d_reach, 0, sizeof(uint32_t) * (size_t)n, stream));
    REACH_TRY(hipMemsetAsync(d_gain, 0, sizeof(uint32_t) * (size_t)n, stream));
    REACH_TRY(hipMemsetAsync(d_cover, 0, sizeof(uint64_t) * nw, stream));
    REACH_TRY(hipMemsetAsync(st, 0, sizeof(ReachThinState), stream));
    REACH_TRY(hipMemcpyAsync(d_live, live.data(), (size_t)n, hipMemcpyHostToDevice, stream));
    REACH_TRY(hipMemcpyAsync(d_flag, flag.data(), (size_t)n, hipMemcpyHostToDevice, stream));
    const unsigned g_iv = blocks_of(mi, kThreads);
    auto ranks = [&](const ReachThinState *s) {
        hipLaunchKernelGGL(k_plane_tiles, dim3((unsigned)nt_plane), dim3(kTile), 0, stream, d_cover, (uint32_t)nw,
                           within, tiles32, s);
        hipLaunchKernelGGL(k_tile_scan<SumOp>, dim3(1), dim3(kTile), 0, stream, tiles32, nt_plane, s);
    };
    uint32_t kept = 0, all = 0;
    ReachThinState hs{};
    if (mi) {
        hipLaunchKernelGGL(k_reach_gain<true>, dim3(g_iv), dim3(kThreads), 0, stream, prim, iv_lo, iv_hi, mi,
                           (const uint64_t *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr,
                           (const uint8_t *)nullptr, d_reach, (const ReachThinState *)nullptr);
        if (any_forced)
            hipLaunchKernelGGL(k_reach_apply_flagged, dim3(kApplyBlocks), dim3(kThreads), 0, stream, prim, iv_lo, iv_hi,
                               mi, d_flag, d_cover);
        ranks(nullptr);
        hipLaunchKernelGGL(k_reach_gain<false>, dim3(g_iv), dim3(kThreads), 0, stream, prim, iv_lo, iv_hi, mi, d_cover,
                           within, tiles32, d_live, d_gain, st);
        REACH_TRY(hipGetLastError());
    }
    REACH_TRY(hipEventRecord(ev_[2], stream));

    // (3) rounds, kRoundsPerBatch per read of the state; every round but the last picks a primer, so there are at
    // most n + 1 of them
    if (mi) {
        for (int batch = 0;; ++batch) {
            for (int b = 0; b < kRoundsPerBatch; ++b) {
                hipLaunchKernelGGL(k_reach_pick, dim3(1), dim3(kThreads), 0, stream, d_gain, d_live, n, min_gain,
                                   d_order, d_gains, st);
                hipLaunchKernelGGL(k_reach_apply, dim3(kApplyBlocks), dim3(kThreads), 0, stream, first, iv_lo, iv_hi,
                                   d_cover, d_gain, n, st);
                ranks(st);
                hipLaunchKernelGGL(k_reach_gain<false>, dim3(g_iv), dim3(kThreads), 0, stream, prim, iv_lo, iv_hi, mi,
                                   d_cover, within, tiles32, d_live, d_gain, st);
            }
            REACH_TRY(hipGetLastError());
            REACH_TRY(hipMemcpyAsync(&hs, st, sizeof hs, hipMemcpyDeviceToHost, stream));
            REACH_TRY(hipStreamSynchronize(stream));
            if (hs.done) break;
            if (batch + 1 >= n / kRoundsPerBatch + 2) {
                err = "panel thin reach: more rounds than primers";
                return MSSPE_ERR_DEVICE;
            }
        }
        // the ranks of the last round that ran stand behind its apply: their total is |C|
        REACH_TRY(hipMemcpyAsync(&kept, tiles32 + nt_plane, sizeof kept, hipMemcpyDeviceToHost, stream));
    }
    REACH_TRY(hipEventRecord(ev_[3], stream));
    reported_ = true;

    // (4) the picks, the columns of the whole panel, the kept primers' site planes
    const int n_picked = (int)hs.n_picked;
    if (n_picked > n) {
        err = "panel thin reach: more picks than primers";
        return MSSPE_ERR_DEVICE;
    }
    if (n_picked) {
        REACH_TRY(hipMemcpyAsync(order_out, d_order, sizeof(uint32_t) * (size_t)n_picked, hipMemcpyDeviceToHost, stream));
        REACH_TRY(hipMemcpyAsync(gain_out, d_gains, sizeof(uint32_t) * (size_t)n_picked, hipMemcpyDeviceToHost, stream));
    }
    if (reach_out)
        REACH_TRY(hipMemcpyAsync(reach_out, d_reach, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
    REACH_TRY(hipStreamSynchronize(stream));
    for (int i = 0; i < n_picked; ++i) {
        if (order_out[i] >= (uint32_t)n) {
            err = "panel thin reach: a pick outside the panel";
            return MSSPE_ERR_DEVICE;
        }
        keep_out[order_out[i]] = 1;
    }
    for (int p = 0; p < n; ++p) flag[(size_t)p] = keep_out[p] ? 1 : 0;
    REACH_TRY(hipMemcpyAsync(d_flag, flag.data(), (size_t)n, hipMemcpyHostToDevice, stream));
    if (mi) {
        hipLaunchKernelGGL(k_reach_apply_flagged, dim3(kApplyBlocks), dim3(kThreads), 0, stream, prim, iv_lo, iv_hi, mi,
                           (const uint8_t *)nullptr, d_cover);
        ranks(nullptr);
        REACH_TRY(hipGetLastError());
        REACH_TRY(hipMemcpyAsync(&all, tiles32 + nt_plane, sizeof all, hipMemcpyDeviceToHost, stream));
    }
    if (m && d_plus) {
        hipLaunchKernelGGL(k_keys_to_planes, dim3(blocks_of(m, kThreads)), dim3(kThreads), 0, stream, d_keys, m, d_flag,
                           d_plus, d_minus);
        REACH_TRY(hipGetLastError());
    }
    REACH_TRY(hipStreamSynchronize(stream));
    rounds_ = hs.rounds;
    *n_picked_out = n_picked;
    if (reached_all_out) *reached_all_out = (long long)all;
    if (reached_kept_out) *reached_kept_out = (long long)kept;
    for (int ph = 0; ph < 3; ++ph) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev_[ph], ev_[ph + 1]);
        phase_us_[ph] = (long long)(ms * 1000.0f);
    }
    return MSSPE_OK;
}

int PanelThinReach::end_report(hipStream_t stream, std::string &err)
{
    if (!reported_) return MSSPE_OK;
    REACH_TRY(hipEventRecord(ev_[4], stream));
    REACH_TRY(hipEventSynchronize(ev_[4]));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev_[3], ev_[4]);
    phase_us_[3] = (long long)(ms * 1000.0f);
    reported_ = false;
    return MSSPE_OK;
}

}  // namespace msspe
