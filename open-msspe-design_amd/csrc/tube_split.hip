// tube_split.hip -- the conflict graph split into reaction tubes on the device (engine extension).
//
// Where the vertex cover deletes primers until no two survivors conflict, a bench scientist splits the multiplex into a
// few tubes so that no two primers of one tube conflict, and keeps nearly all of them.  The rule is a greedy colouring:
// visit the nodes by descending key(v) = (degree, lexicographic rank) -- the degree is static -- and give v the lowest
// tube in [0, max_tubes) that holds no neighbour placed before it; with no such tube v stays unplaced
// (MSSPE_TUBE_NONE) and constrains nobody.  A node that conflicts with itself fits in no tube: it is unplaced from the
// start, constrains nobody and nobody waits for it.  Largest degree first, because the hard nodes must choose while
// tubes are free: on a random graph of 2,000 nodes at 8 tubes it leaves 92 unplaced where ascending order leaves 218.
// It is no substitute for the cover at one tube: --tubes 1 keeps fewer primers than the cover does.
//
// The device computes the same assignment in rounds.  wait(v) = the neighbours with a greater key that are not self-
// conflicting; a node decides in the round after its wait reaches 0.  Two nodes of one round are never adjacent (the
// lower would still wait for the higher), and when v decides, its decided neighbours are exactly those with greater
// keys: v sees the tubes the sequential visit would show it.
//
// Phases: the cover's (ranks, duplicate check, partners, S = B | B^T, self pairs dropped; CoverStage::prepare), the
// keys, the waits and ready list 0, then rounds of one plain launch each over the round's ready list: one walk over the
// node's row of S that takes one off the wait of every undecided neighbour (the lane that takes the last one appends
// the neighbour to the next list) and collects the tubes of the placed ones.  Every row is walked three times in all.
// Three list counters rotate: a round reads one, fills the next and clears the third.  A round that finds its list
// empty sets a device word; later launches of the batch return at once, and the host reads the word once per batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/msspe_hip.h"
#include "tube_split.hpp"

namespace msspe {

namespace {

constexpr int kRoundsPerBatch = 16;   // rounds enqueued between two reads of the "done" word
constexpr int kWavesPerBlock = 4;
constexpr uint8_t kUndecided = 254;   // never a result: tubes are 0..63, MSSPE_TUBE_NONE is 255

struct TubeState {
    uint32_t done;        // 1: a round found its ready list empty (the rounds that follow return at once)
    uint32_t rounds;      // rounds that decided nodes
    uint32_t unplaced;    // self-conflicting nodes and nodes with a neighbour in every tube
    uint32_t used;        // highest tube in use + 1
    uint32_t list_n[3];   // round r reads list_n[r % 3], fills list_n[(r + 1) % 3], clears list_n[(r + 2) % 3]
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
{
    for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__device__ __forceinline__ uint64_t wave_or(uint64_t x)
{
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    for (int o = 32; o; o >>= 1) {
        lo |= __shfl_xor(lo, o, 64);
        hi |= __shfl_xor(hi, o, 64);
    }
    return (uint64_t)hi << 32 | lo;
}

// key = degree << 32 | rank, the degree static: the neighbours other than the node itself, self-conflicting ones
// included.  A self-conflicting node gets key 0, which is greater than no key: nobody waits for it.
__global__ __launch_bounds__(256) void k_tube_keys(const uint64_t *S, int n, int W, const uint32_t *rank, uint64_t *key)
{
    const int lane = threadIdx.x & 63;
    const int waves = gridDim.x * kWavesPerBlock;
    for (int v = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); v < n; v += waves) {
        const uint64_t *row = S + (size_t)v * W;
        uint32_t d = 0;
        for (int w = lane; w < W; w += 64) d += (uint32_t)__popcll(row[w]);
        d = wave_sum(d);
        if (lane == 0) {
            const uint32_t self = (uint32_t)(row[v >> 6] >> (v & 63)) & 1u;
            key[v] = self ? 0 : (uint64_t)d << 32 | rank[v];   // no own bit to take off
        }
    }
}

// wait[v] = neighbours with a greater key (self-conflicting ones have key 0 and never count).  A self-conflicting node
// is unplaced at once; a node that waits for nobody goes on ready list 0; every other node is undecided.
__global__ __launch_bounds__(256) void k_tube_wait(const uint64_t *S, int n, int W, const uint64_t *key, uint32_t *wait,
                                                   uint8_t *tube, uint32_t *list0, TubeState *st)
{
    const int lane = threadIdx.x & 63;
    const int waves = gridDim.x * kWavesPerBlock;
    for (int v = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); v < n; v += waves) {
        const uint64_t *row = S + (size_t)v * W;
        if ((row[v >> 6] >> (v & 63)) & 1) {   // whole waves
            if (lane == 0) {
                tube[v] = MSSPE_TUBE_NONE;
                atomicAdd(&st->unplaced, 1u);
            }
            continue;
        }
        const uint64_t kv = key[v];
        uint32_t c = 0;
        for (int w = lane; w < W; w += 64) {
            uint64_t m = row[w];
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                c += key[(size_t)w * 64 + b] > kv;
            }
        }
        c = wave_sum(c);
        if (lane == 0) {
            wait[v] = c;
            tube[v] = kUndecided;
            if (c == 0) list0[atomicAdd(&st->list_n[0], 1u)] = (uint32_t)v;
        }
    }
}

// One round: every node of the ready list decides.  Nothing a ready node reads is written in its round: its undecided
// neighbours have smaller keys and wait (for it, at least), its decided ones decided in earlier rounds.
__global__ __launch_bounds__(256) void k_tube_round(const uint64_t *S, int W, const uint32_t *ready, uint32_t *next,
                                                    uint32_t *wait, uint8_t *tube, TubeState *st, int cur,
                                                    uint64_t tubes_mask)
{
    if (st->done) return;
    const uint32_t cnt = st->list_n[cur];
    const int nxt = cur == 2 ? 0 : cur + 1, clr = nxt == 2 ? 0 : nxt + 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (cnt == 0) st->done = 1;
        else {
            st->rounds += 1;
            st->list_n[clr] = 0;
        }
    }
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * kWavesPerBlock;
    for (uint32_t i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); i < cnt; i += waves) {
        const uint32_t v = ready[i];
        const uint64_t *row = S + (size_t)v * W;
        uint64_t taken = 0;
        for (int w0 = 0; w0 < W; w0 += 64) {
            const int w = w0 + lane;
            uint64_t m = w < W ? row[w] : 0;
            if (w == (int)(v >> 6)) m &= ~(1ull << (v & 63));
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                const size_t u = (size_t)w * 64 + b;
                const uint8_t t = tube[u];
                if (t == kUndecided) {
                    if (atomicSub(&wait[u], 1u) == 1u) next[atomicAdd(&st->list_n[nxt], 1u)] = (uint32_t)u;
                } else if (t < kTubeMax) {
                    taken |= 1ull << t;
                }
            }
        }
        taken = wave_or(taken);
        if (lane == 0) {
            const uint64_t open = ~taken & tubes_mask;
            if (open) {
                const uint32_t t = (uint32_t)__builtin_ctzll(open);
                tube[v] = (uint8_t)t;
                atomicMax(&st->used, t + 1);
            } else {
                tube[v] = MSSPE_TUBE_NONE;
                atomicAdd(&st->unplaced, 1u);
            }
        }
    }
}

}  // namespace

void TubeStage::release()
{
    if (state_) (void)hipFree(state_);
    state_ = nullptr;
    for (auto &e : ev_) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

int TubeStage::run(CoverStage &cover, const uint64_t *d_pool, int n, int k, const uint64_t *d_bitmap,
                   bool drop_self_pairs, int max_tubes, uint8_t *d_tube, int *n_tubes_used, int *n_unplaced, int n_cu,
                   hipStream_t stream, std::string &err)
{
    rounds_ = 0;
    for (auto &p : phase_us_) p = 0;
    if (n_tubes_used) *n_tubes_used = 0;
    if (n_unplaced) *n_unplaced = 0;
    if (n == 0) return MSSPE_OK;
    const int W = (n + 63) / 64;
    if (!state_) {
        const hipError_t e = hipMalloc(&state_, sizeof(TubeState));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            state_ = nullptr;
            err = std::string("hipMalloc (tube split state): ") + hipGetErrorString(e);
            return MSSPE_ERR_DEVICE;
        }
    }
    for (auto &e : ev_)
        if (!e && hipEventCreate(&e) != hipSuccess) {
            err = "tube split: hipEventCreate failed";
            return MSSPE_ERR_DEVICE;
        }
    int rc;
    if ((rc = cover.begin(n, k, stream, err)) || (rc = cover.prepare(d_pool, n, k, d_bitmap, drop_self_pairs, stream, err)))
        return rc;
    const uint64_t *S = cover.symmetrised();
    uint64_t *key = cover.round_keys();
    uint32_t *list[2] = {cover.round_lists(), cover.round_lists() + n}, *wait = cover.round_counters();
    TubeState *st = (TubeState *)state_;
    auto launched = [&](const char *what) -> int {
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return MSSPE_OK;
        err = std::string("tube split, ") + what + ": " + hipGetErrorString(e);
        return MSSPE_ERR_DEVICE;
    };

    (void)hipEventRecord(ev_[0], stream);
    if (hipMemsetAsync(st, 0, sizeof(TubeState), stream) != hipSuccess) {
        err = "tube split: hipMemsetAsync failed";
        return MSSPE_ERR_DEVICE;
    }
    const int blocks = std::max(1, std::min((n + kWavesPerBlock - 1) / kWavesPerBlock, 8 * n_cu));
    hipLaunchKernelGGL(k_tube_keys, dim3(blocks), dim3(256), 0, stream, S, n, W, cover.ranks(), key);
    hipLaunchKernelGGL(k_tube_wait, dim3(blocks), dim3(256), 0, stream, S, n, W, key, wait, d_tube, list[0], st);
    if ((rc = launched("keys"))) return rc;

    // rounds, kRoundsPerBatch per read of the done word; every round with a list decides at least one node, so there
    // are at most n of them and one that finds its list empty
    const uint64_t tubes_mask = max_tubes >= 64 ? ~0ull : (1ull << max_tubes) - 1;
    TubeState hs{};
    long r = 0;
    for (int batch = 0;; ++batch) {
        for (int b = 0; b < kRoundsPerBatch; ++b, ++r)
            hipLaunchKernelGGL(k_tube_round, dim3(blocks), dim3(256), 0, stream, S, W, list[r & 1], list[(r + 1) & 1],
                               wait, d_tube, st, (int)(r % 3), tubes_mask);
        if ((rc = launched("rounds"))) return rc;
        if (hipMemcpyAsync(&hs, st, sizeof hs, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) {
            err = "tube split: reading the round state failed";
            return MSSPE_ERR_DEVICE;
        }
        if (hs.done) break;
        if (batch + 1 >= n / kRoundsPerBatch + 2) {
            err = "tube split: more rounds than nodes";
            return MSSPE_ERR_DEVICE;
        }
    }
    (void)hipEventRecord(ev_[1], stream);
    if (hipEventSynchronize(ev_[1]) != hipSuccess) {
        err = "tube split: hipEventSynchronize failed";
        return MSSPE_ERR_DEVICE;
    }
    cover.prepare_us(phase_us_[0], phase_us_[1]);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev_[0], ev_[1]);
    phase_us_[2] = (long long)(ms * 1000.0f);
    rounds_ = hs.rounds;
    if (n_tubes_used) *n_tubes_used = (int)hs.used;
    if (n_unplaced) *n_unplaced = (int)hs.unplaced;
    return MSSPE_OK;
}

}  // namespace msspe
