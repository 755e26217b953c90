// screen_plan.hpp -- how a pair screen's block is cut into first-stage launches and where the hand-over lists are
// flushed between them.  Plain integer arithmetic (C++17, no HIP): capi.cpp run_chain executes the plan, and
// msspe_host_screen_plan hands it to the CPU tests (tests/test_screen_plan_model.py) as it stands.
#pragma once

#include <algorithm>
#include <vector>

namespace msspe {

constexpr long kChunkPairs = 1L << 29;   // pairs per launch of the all-pairs kernel (a launch's tail: 2.4 % at 2^24, 1.4 % at 2^26; a 65,536-primer
                                         // pool: 1850 ms at 2^27, 1822 at 2^29, 1819 at 2^30 -- and a hand-over list of as many entries, 4 GB, twice)
constexpr long kRowGroup = 24;           // rows per group of the first-stage kernels (12 or 8 waves per block)

// What runs first over a block.  Dense: the dense kernel takes the whole block, no hand-over lists.  Wave: one wave
// per pair over pool columns.  Every other stage screens composition-sorted columns; BoundMirror: the bound stage of
// a square same-pool block, each unordered pair once.
enum class FirstStage { Dense, Wave, Split, Fast, Int, Row, Bound, BoundMirror };

// One first-stage launch: rows [row0, row1) x columns [col0, col1), the pairs it processes, the most entries it can
// append to hand-over list 0, and whether the lists are flushed before it.  (After the last launch they are flushed
// whenever a launch has run since the last flush.)
struct Launch {
    int row0, row1, col0, col1;
    long pairs;
    long list_entries;
    bool flush_before;
};

struct ScreenPlan {
    std::vector<Launch> launches;
    long mirrored = 0;   // BoundMirror: ordered pairs that get no fill of their own, n (n - 1) / 2
};

// The mirrored launches append a pair in both orders: each stays within half a list and kChunkPairs.
inline long mirror_launch_cap(long list_cap) { return std::min(kChunkPairs, list_cap / 2); }

// Rows [row0, row1) against ncols columns that start at pool column col0, under hand-over lists of list_cap entries.
// BoundMirror wants the square block (row0 == col0, row1 - row0 == ncols) with ncols <= mirror_launch_cap(list_cap).
inline ScreenPlan plan_screen(FirstStage first, int row0, int row1, int col0, int ncols, long list_cap)
{
    ScreenPlan plan;
    // Overflow pairs are collected over several launches and finished together: the list kernels have a fixed latency
    // floor, and list_cap entries cannot be overrun while the launches since the last flush could not have appended
    // more than that between them, even if every pair were handed on.
    long pending = 0;   // worst-case entries the list may hold
    auto add = [&](long r0, long r1, long c0, long c1, long pairs, long entries) {
        const bool flush = pending + entries > list_cap;
        if (flush) pending = 0;
        plan.launches.push_back({(int)r0, (int)r1, (int)c0, (int)c1, pairs, entries, flush});
        pending += entries;
    };
    if (first == FirstStage::BoundMirror) {
        // Rows are taken in the columns' sorted order: row p is sorted[p] (pool index perm[p]) and screens the sorted
        // columns q >= p; a pair that is not culled is appended in both orders, so a launch that processes P pairs may
        // append 2 P entries.  The row ranges are cut so that the launches process near-equal pair counts (earlier rows
        // have longer suffixes).
        const long mirror_cap = mirror_launch_cap(list_cap);
        const long n = ncols;
        auto processed = [&](long p0, long p1) { return (p1 - p0) * n - (p1 * (p1 - 1) - p0 * (p0 - 1)) / 2; };   // sum of n - p
        const long total = processed(0, n);
        const long n_launch = (total + mirror_cap - 1) / mirror_cap;
        const long target = (total + n_launch - 1) / n_launch;
        for (long p0 = 0; p0 < n;) {
            // the first row count that reaches the target, in whole groups of 24 rows, within the cap (one row always is)
            long lo = p0 + 1, hi = n;
            while (lo < hi) {
                const long mid = lo + (hi - lo) / 2;
                if (processed(p0, mid) >= target) hi = mid;
                else lo = mid + 1;
            }
            long p1 = std::min(n, p0 + (lo - p0 + kRowGroup - 1) / kRowGroup * kRowGroup);
            while (p1 > p0 + 1 && processed(p0, p1) > mirror_cap) --p1;
            const long launch_pairs = processed(p0, p1);
            add(p0, p1, 0, n, launch_pairs, 2 * launch_pairs);
            p0 = p1;
        }
        plan.mirrored = n * (n - 1) / 2;
        return plan;
    }
    // A launch covers at most kChunkPairs pairs, and never more than one hand-over list holds (a fixed
    // list_cap_log2 below 29, or lists shrunk because the card is short of memory): even a launch that handed
    // every pair on cannot overrun its list.
    const long chunk_pairs = std::min(kChunkPairs, list_cap);
    // The block's rows are split evenly over as few launches as the limit allows (a 65,536-row block: nine launches of
    // about 7,296 rows rather than eight of 8,184 and one of 64; the 8,192 rows a rank of eight owns: one launch, not
    // 8,184 + 8), in whole row groups of the first-stage kernels (no idle waves in the last tile row of a launch that is
    // not the block's last).
    const long max_rows = std::max(1L, chunk_pairs / ncols), n_rows_all = (long)row1 - row0;
    long rows_per_chunk = max_rows;
    if (n_rows_all > max_rows) {
        const long cap_rows = max_rows > kRowGroup ? max_rows - max_rows % kRowGroup : max_rows;   // the largest whole-group launch
        const long n_launch = (n_rows_all + cap_rows - 1) / cap_rows;
        rows_per_chunk = (n_rows_all + n_launch - 1) / n_launch;
        if (rows_per_chunk > kRowGroup)
            rows_per_chunk = std::min(cap_rows, (rows_per_chunk + kRowGroup - 1) / kRowGroup * kRowGroup);
    } else if (n_rows_all > 0) {
        rows_per_chunk = n_rows_all;
    }
    if (rows_per_chunk < 1) rows_per_chunk = 1;
    for (long r = row0; r < row1; r += rows_per_chunk) {
        const long r_end = std::min<long>(row1, r + rows_per_chunk);
        if (first == FirstStage::Dense) {   // a band of rows and every column of the block; nothing is handed on
            add(r, r_end, col0, (long)col0 + ncols, (r_end - r) * ncols, 0);
            continue;
        }
        // sorted-column index range (one chunk unless a row is longer than a launch); the wave kernel: pool columns
        const long c_base = first == FirstStage::Wave ? col0 : 0;
        for (long q0 = 0; q0 < ncols; q0 += chunk_pairs) {
            const long q_end = std::min<long>(ncols, q0 + chunk_pairs);
            const long launch_pairs = (r_end - r) * (q_end - q0);
            add(r, r_end, c_base + q0, c_base + q_end, launch_pairs, launch_pairs);
        }
    }
    return plan;
}

}  // namespace msspe
