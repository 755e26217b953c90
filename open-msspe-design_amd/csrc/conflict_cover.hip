// conflict_cover.hip -- the greedy minimum vertex cover of the conflict graph on the device
// (od-msspe/src/main.rs:754-798).
//
// The reference deletes, one at a time, the primer with the most live conflicts (ties: the lexicographically greatest
// string) until no live primer conflicts with a live one; conflicts are symmetrised and a self conflict counts.  Here
// the same set comes from rounds: with key(v) = (live degree, lexicographic rank), a node whose key exceeds that of
// every live neighbour (a local maximum) is deleted by the sequential rule with its degree unchanged, two local maxima
// are never adjacent, and the sequential choice is always one of them -- so deleting every local maximum at once, round
// after round, ends in the sequential rule's set.
//
// Phases: keys (rocPRIM radix sort of the oligos' lexicographic keys: ranks, duplicates, reverse-complement partners),
// S = B | B^T into a buffer of its own, the live degrees once, then rounds of three plain launches (the local-maximum
// test over the active list, compacting it; the winners' live neighbours lose one degree each; the winners leave the
// live set).  A device word says when no active node is left; later launches of the batch return at once, and the host
// reads the word once per batch of rounds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/msspe_hip.h"
#include "conflict_cover.hpp"

namespace msspe {

namespace {

constexpr int kRoundsPerBatch = 16;   // rounds enqueued between two reads of the "done" word
constexpr int kWavesPerBlock = 4;

struct CoverState {
    uint32_t done;        // 1: no active node left (the rounds that follow return at once)
    uint32_t rounds;      // rounds that deleted nodes
    uint32_t n_deleted;
    uint32_t act_n[2];    // lengths of the two active lists (read by one round, written by the next)
    uint32_t win_n;       // winners of the current round
    uint32_t err;         // 1 duplicate oligo, 2 bits above 2 k
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
{
    for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// lexicographic key of oligo i (base 0 most significant: A < C < G < T as in ASCII) and its index
__global__ void k_cover_keys(const uint64_t *pool, int n, int k, uint64_t *keys, uint32_t *vals, CoverState *st)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t w = pool[i];
    if (k < 32 && (w >> (2 * k)) != 0) atomicOr(&st->err, 2u);
    uint64_t key = 0;
    for (int p = 0; p < k; ++p) key = (key << 2) | ((w >> (2 * p)) & 3);
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

// rank[v] = position of oligo v in lexicographic order; equal neighbours in that order are duplicates.  drop: partner[v]
// = the oligo equal to revcomp(v), or -1.  The key of revcomp(w) is the complement of the packed word w: base p of the
// reverse complement is 3 - base (k-1-p) of w, and the key puts base p at bits 2 (k-1-p).
__global__ void k_cover_rank(const uint64_t *pool, const uint64_t *sorted, const uint32_t *perm, int n, int k, int drop,
                             uint32_t *rank, int32_t *partner, CoverState *st)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint32_t v = perm[r];
    rank[v] = (uint32_t)r;
    if (r > 0 && sorted[r] == sorted[r - 1]) atomicOr(&st->err, 1u);
    if (!drop) return;
    const uint64_t mask = k == 32 ? ~0ull : (1ull << (2 * k)) - 1;
    const uint64_t want = ~pool[v] & mask;
    int lo = 0, hi = n;   // first position with sorted[pos] >= want
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sorted[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    partner[v] = lo < n && sorted[lo] == want ? (int32_t)perm[lo] : -1;
}

// S = B | B^T over [0, n)^2, one wave per 64 x 64 bit tile (row block R, word column J); padding bits beyond n cleared.
// Lane l holds row J*64+l of B at word R; bit l of ballot(bit b of it) is B[J*64+l][R*64+b] = B^T[R*64+b][J*64+l].
__global__ __launch_bounds__(256) void k_cover_symmetrise(const uint64_t *B, int n, int W, uint64_t *S)
{
    const int lane = threadIdx.x & 63;
    const long tile = (long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (tile >= (long)W * W) return;   // whole waves
    const int R = (int)(tile / W), J = (int)(tile % W);
    const int c = J * 64 + lane, r = R * 64 + lane;
    const uint64_t t = c < n ? B[(size_t)c * W + R] : 0;
    uint64_t mine = 0;
    for (int b = 0; b < 64; ++b) {
        const uint64_t col = __ballot((t >> b) & 1);
        if (lane == b) mine = col;
    }
    if (r >= n) return;
    uint64_t s = B[(size_t)r * W + J] | mine;
    if (J == W - 1 && (n & 63)) s &= (1ull << (n & 63)) - 1;
    S[(size_t)r * W + J] = s;
}

// --check-self-dimers false: the pairs (a, a) and (a, revcomp(a)) are never edges (od-msspe/src/delta_g.rs:64-69)
__global__ void k_cover_drop_self(uint64_t *S, int n, int W, const int32_t *partner)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    uint64_t *row = S + (size_t)v * W;
    row[v >> 6] &= ~(1ull << (v & 63));
    const int32_t p = partner[v];
    if (p >= 0) row[p >> 6] &= ~(1ull << (p & 63));
}

// every node alive, nothing deleted yet
__global__ void k_cover_init(int W, uint64_t *alive, uint64_t *kill, int n, CoverState *st)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < W) {
        alive[i] = i == W - 1 && (n & 63) ? (1ull << (n & 63)) - 1 : ~0ull;
        kill[i] = 0;
    }
    if (i == 0) {
        st->done = 0;
        st->rounds = 0;
        st->n_deleted = 0;
        st->act_n[0] = 0;
        st->act_n[1] = 0;
        st->win_n = 0;
    }
}

// Live degrees before the first round (every node alive; the self bit counts: the host's rule), kept as key = degree <<
// 32 | rank; the nodes with live neighbours form active list 0.
__global__ __launch_bounds__(256) void k_cover_degree(const uint64_t *S, int n, int W, const uint32_t *rank,
                                                      uint64_t *key, uint32_t *act0, CoverState *st)
{
    const int lane = threadIdx.x & 63;
    const int waves = gridDim.x * kWavesPerBlock;
    for (int v = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); v < n; v += waves) {
        const uint64_t *row = S + (size_t)v * W;
        uint32_t d = 0;
        for (int w = lane; w < W; w += 64) d += (uint32_t)__popcll(row[w]);
        d = wave_sum(d);
        if (lane == 0) {
            key[v] = (uint64_t)d << 32 | rank[v];
            if (d) act0[atomicAdd(&st->act_n[0], 1u)] = (uint32_t)v;
        }
    }
}

// Round, step 1: every live node of list cur with live neighbours goes on to list cur ^ 1 (degrees only fall, so a
// node that leaves the list never returns); one whose key exceeds every live neighbour's (itself excepted) is deleted --
// marked in kill (applied by step 3, so that every test of the round sees the same live set), in the output and in
// the round's winner list.  The neighbours of an active node are active themselves (conflicts are symmetric).
__global__ __launch_bounds__(256) void k_cover_pick(const uint64_t *S, int W, const uint64_t *alive,
                                                    const uint64_t *key, const uint32_t *act, uint32_t *act_next,
                                                    CoverState *st, int cur, uint64_t *kill, uint8_t *deleted,
                                                    uint32_t *win)
{
    if (st->done) return;
    const uint32_t cnt = st->act_n[cur];
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * kWavesPerBlock;
    for (uint32_t i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); i < cnt; i += waves) {
        const uint32_t v = act[i];
        const uint64_t kv = key[v];
        if (!((alive[v >> 6] >> (v & 63)) & 1) || (kv >> 32) == 0) continue;   // whole waves
        if (lane == 0) act_next[atomicAdd(&st->act_n[cur ^ 1], 1u)] = v;
        const uint64_t *row = S + (size_t)v * W;
        bool lose = false;
        for (int w0 = 0; w0 < W; w0 += 64) {
            const int w = w0 + lane;
            uint64_t m = w < W ? row[w] & alive[w] : 0;
            if (w == (int)(v >> 6)) m &= ~(1ull << (v & 63));
            while (m && !lose) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                lose = key[(size_t)w * 64 + b] > kv;
            }
            if (__any(lose)) {
                lose = true;
                break;
            }
        }
        if (!lose && lane == 0) {
            atomicOr((unsigned long long *)&kill[v >> 6], 1ull << (v & 63));
            deleted[v] = 1;
            atomicAdd(&st->n_deleted, 1u);
            win[atomicAdd(&st->win_n, 1u)] = v;
        }
    }
}

// Round, step 2: each winner's live neighbours lose one degree (the key's upper half).  Winners are never adjacent, so
// the live set before step 3 is the right one.  No winner means no active node was left: the cover is done.
__global__ __launch_bounds__(256) void k_cover_update(const uint64_t *S, int W, const uint64_t *alive,
                                                      const uint32_t *win, CoverState *st, uint64_t *key)
{
    if (st->done) return;
    const uint32_t nw = st->win_n;
    if (nw == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) st->done = 1;
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) st->rounds += 1;
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * kWavesPerBlock;
    for (uint32_t i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); i < nw; i += waves) {
        const uint32_t v = win[i];
        const uint64_t *row = S + (size_t)v * W;
        for (int w = lane; w < W; w += 64) {
            uint64_t m = row[w] & alive[w];
            if (w == (int)(v >> 6)) m &= ~(1ull << (v & 63));
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                atomicAdd((unsigned long long *)&key[(size_t)w * 64 + b], ~0ull << 32);   // degree - 1
            }
        }
    }
}

// Round, step 3: the winners leave the live set; list cur (read by step 1) and the winner list are emptied
__global__ void k_cover_apply(uint64_t *alive, uint64_t *kill, int W, CoverState *st, int cur)
{
    if (st->done) return;
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < W) {
        alive[w] &= ~kill[w];
        kill[w] = 0;
    }
    if (w == 0) {
        st->act_n[cur] = 0;
        st->win_n = 0;
    }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

int CoverStage::ensure(int slot, size_t bytes, std::string &err)
{
    if (cap_[slot] >= bytes) return MSSPE_OK;
    if (buf_[slot]) (void)hipFree(buf_[slot]);
    buf_[slot] = nullptr;
    cap_[slot] = 0;
    const hipError_t e = hipMalloc(&buf_[slot], bytes ? bytes : 16);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // an allocation failure is reported, not left sticky for the next call
        err = std::string("hipMalloc (conflict cover, ") + std::to_string(bytes) + " bytes): " + hipGetErrorString(e);
        return MSSPE_ERR_DEVICE;
    }
    cap_[slot] = bytes;
    return MSSPE_OK;
}

void CoverStage::release()
{
    for (int s = 0; s < 11; ++s) {
        if (buf_[s]) (void)hipFree(buf_[s]);
        buf_[s] = nullptr;
        cap_[s] = 0;
    }
    for (auto &e : ev_) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

int CoverStage::begin(int n, int k, hipStream_t stream, std::string &err)
{
    const int W = (n + 63) / 64;
    sort_tmp_ = 0;
    {
        uint64_t *nk = nullptr;
        uint32_t *nv = nullptr;
        if (rocprim::radix_sort_pairs(nullptr, sort_tmp_, nk, nk, nv, nv, (size_t)n, 0u, 2u * k, stream) != hipSuccess) {
            err = "conflict cover: rocPRIM radix sort sizing failed";
            return MSSPE_ERR_DEVICE;
        }
    }
    // 0 S, 1 keys in, 2 keys sorted, 3 vals in, 4 perm, 5 sort scratch, 6 rank + partner, 7 key64 (per round),
    // 8 two active lists, 9 alive + kill + state, 10 the round's winners
    int rc;
    if ((rc = ensure(0, sizeof(uint64_t) * (size_t)n * (size_t)W, err)) || (rc = ensure(1, 8 * (size_t)n, err)) ||
        (rc = ensure(2, 8 * (size_t)n, err)) || (rc = ensure(3, 4 * (size_t)n, err)) ||
        (rc = ensure(4, 4 * (size_t)n, err)) || (rc = ensure(5, sort_tmp_, err)) ||
        (rc = ensure(6, 8 * (size_t)n, err)) || (rc = ensure(7, 8 * (size_t)n, err)) ||
        (rc = ensure(8, 8 * (size_t)n, err)) ||
        (rc = ensure(9, align256(16 * (size_t)W) + sizeof(CoverState), err)) || (rc = ensure(10, 4 * (size_t)n, err)))
        return rc;
    for (auto &e : ev_)
        if (!e && hipEventCreate(&e) != hipSuccess) {
            err = "conflict cover: hipEventCreate failed";
            return MSSPE_ERR_DEVICE;
        }
    (void)hipEventRecord(ev_[0], stream);
    return MSSPE_OK;
}

int CoverStage::prepare(const uint64_t *d_pool, int n, int k, const uint64_t *d_bitmap, bool drop_self_pairs,
                        hipStream_t stream, std::string &err)
{
    const int W = (n + 63) / 64;
    uint64_t *S = (uint64_t *)buf_[0], *keys_in = (uint64_t *)buf_[1], *keys = (uint64_t *)buf_[2];
    uint32_t *vals = (uint32_t *)buf_[3], *perm = (uint32_t *)buf_[4];
    uint32_t *rank = (uint32_t *)buf_[6];
    int32_t *partner = (int32_t *)((uint32_t *)buf_[6] + n);
    CoverState *st = (CoverState *)((char *)buf_[9] + align256(16 * (size_t)W));
    auto launched = [&](const char *what) -> int {
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return MSSPE_OK;
        err = std::string("conflict cover, ") + what + ": " + hipGetErrorString(e);
        return MSSPE_ERR_DEVICE;
    };
    int rc;

    // keys: ranks, duplicates, partners
    if (hipMemsetAsync(&st->err, 0, sizeof(uint32_t), stream) != hipSuccess) {
        err = "conflict cover: hipMemsetAsync failed";
        return MSSPE_ERR_DEVICE;
    }
    hipLaunchKernelGGL(k_cover_keys, dim3((n + 255) / 256), dim3(256), 0, stream, d_pool, n, k, keys_in, vals, st);
    if (rocprim::radix_sort_pairs(buf_[5], sort_tmp_, keys_in, keys, vals, perm, (size_t)n, 0u, 2u * k, stream) !=
        hipSuccess) {
        err = "conflict cover: rocPRIM radix sort failed";
        return MSSPE_ERR_DEVICE;
    }
    hipLaunchKernelGGL(k_cover_rank, dim3((n + 255) / 256), dim3(256), 0, stream, d_pool, keys, perm, n, k,
                       drop_self_pairs ? 1 : 0, rank, partner, st);
    if ((rc = launched("keys"))) return rc;
    (void)hipEventRecord(ev_[1], stream);

    uint32_t herr = 0;
    if (hipMemcpyAsync(&herr, &st->err, sizeof herr, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) {
        err = "conflict cover: reading the key check failed";
        return MSSPE_ERR_DEVICE;
    }
    if (herr & 2u) {
        err = "conflict cover: a pool word has bits above 2 k";
        return MSSPE_ERR_ARG;
    }
    if (herr & 1u) {
        err = "conflict cover: the pool holds duplicate oligos (the graph's nodes are distinct primers)";
        return MSSPE_ERR_ARG;
    }

    (void)hipEventRecord(ev_[2], stream);

    // S = B | B^T (and the self pairs dropped)
    const long tiles = (long)W * W;
    hipLaunchKernelGGL(k_cover_symmetrise, dim3((unsigned)((tiles + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(256), 0,
                       stream, d_bitmap, n, W, S);
    if (drop_self_pairs)
        hipLaunchKernelGGL(k_cover_drop_self, dim3((n + 255) / 256), dim3(256), 0, stream, S, n, W, partner);
    if ((rc = launched("symmetrise"))) return rc;
    (void)hipEventRecord(ev_[3], stream);
    return MSSPE_OK;
}

void CoverStage::prepare_us(long long &keys_us, long long &symmetrise_us) const
{
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev_[0], ev_[1]);
    keys_us = (long long)(ms * 1000.0f);
    ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev_[2], ev_[3]);
    symmetrise_us = (long long)(ms * 1000.0f);
}

int CoverStage::run(const uint64_t *d_pool, int n, int k, const uint64_t *d_bitmap, bool drop_self_pairs,
                    uint8_t *d_deleted, int *n_deleted, int n_cu, hipStream_t stream, std::string &err)
{
    rounds_ = 0;
    for (auto &p : phase_us_) p = 0;
    if (n_deleted) *n_deleted = 0;
    if (n == 0) return MSSPE_OK;
    const int W = (n + 63) / 64;
    int rc;
    if ((rc = begin(n, k, stream, err))) return rc;
    uint64_t *S = (uint64_t *)buf_[0];
    uint32_t *rank = (uint32_t *)buf_[6];
    uint64_t *key64 = (uint64_t *)buf_[7];
    uint32_t *act[2] = {(uint32_t *)buf_[8], (uint32_t *)buf_[8] + n}, *win = (uint32_t *)buf_[10];
    uint64_t *alive = (uint64_t *)buf_[9], *kill = alive + W;
    CoverState *st = (CoverState *)((char *)buf_[9] + align256(16 * (size_t)W));
    auto launched = [&](const char *what) -> int {
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return MSSPE_OK;
        err = std::string("conflict cover, ") + what + ": " + hipGetErrorString(e);
        return MSSPE_ERR_DEVICE;
    };
    hipLaunchKernelGGL(k_cover_init, dim3((n + 255) / 256), dim3(256), 0, stream, W, alive, kill, n, st);
    if (hipMemsetAsync(d_deleted, 0, (size_t)n, stream) != hipSuccess) {
        err = "conflict cover: hipMemsetAsync failed";
        return MSSPE_ERR_DEVICE;
    }
    if ((rc = prepare(d_pool, n, k, d_bitmap, drop_self_pairs, stream, err))) return rc;
    CoverState hs{};

    // rounds, kRoundsPerBatch per read of the done word; each round deletes at least the global maximum, so there are
    // at most n
    const int blocks = std::max(1, std::min((n + kWavesPerBlock - 1) / kWavesPerBlock, 8 * n_cu));
    const int gw = (W + 255) / 256;
    hipLaunchKernelGGL(k_cover_degree, dim3(blocks), dim3(256), 0, stream, S, n, W, rank, key64, act[0], st);
    for (long r = 0;;) {
        for (int b = 0; b < kRoundsPerBatch; ++b, ++r) {
            const int cur = (int)(r & 1);
            hipLaunchKernelGGL(k_cover_pick, dim3(blocks), dim3(256), 0, stream, S, W, alive, key64, act[cur],
                               act[cur ^ 1], st, cur, kill, d_deleted, win);
            hipLaunchKernelGGL(k_cover_update, dim3(blocks), dim3(256), 0, stream, S, W, alive, win, st, key64);
            hipLaunchKernelGGL(k_cover_apply, dim3(gw), dim3(256), 0, stream, alive, kill, W, st, cur);
        }
        if ((rc = launched("rounds"))) return rc;
        if (hipMemcpyAsync(&hs, st, sizeof hs, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) {
            err = "conflict cover: reading the round state failed";
            return MSSPE_ERR_DEVICE;
        }
        if (hs.done) break;
        if (r > (long)n + kRoundsPerBatch) {
            err = "conflict cover: more rounds than nodes";
            return MSSPE_ERR_DEVICE;
        }
    }
    (void)hipEventRecord(ev_[4], stream);
    if (hipEventSynchronize(ev_[4]) != hipSuccess) {
        err = "conflict cover: hipEventSynchronize failed";
        return MSSPE_ERR_DEVICE;
    }
    prepare_us(phase_us_[0], phase_us_[1]);   // keys, symmetrise (the key check's read between), rounds
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev_[3], ev_[4]);
    phase_us_[2] = (long long)(ms * 1000.0f);
    rounds_ = hs.rounds;
    if (n_deleted) *n_deleted = (int)hs.n_deleted;
    return MSSPE_OK;
}

}  // namespace msspe
