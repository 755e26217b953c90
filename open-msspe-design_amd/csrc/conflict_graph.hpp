// conflict_graph.hpp -- the conflict graph under a pair of rules (thal ANY on dG, thal END1 on t): the union of the two
// screens' bitmaps, its counts by kind and its ordered edge list (msspe_conflict_graph*).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/msspe_hip.h"

namespace msspe {

// Bytes the two per-rule planes of one row block may take together when option conflict_graph_block_rows is 0 (auto).
constexpr size_t kGraphPlaneBytes = 64u << 20;

// Rows per block: the option's value where it is positive, else as many as keep both planes within kGraphPlaneBytes
// (at least one); never more than the call has.
inline int graph_block_rows(int option, int n_rows, int words)
{
    long rows = option > 0 ? (long)option : (long)(kGraphPlaneBytes / (16u * (size_t)(words > 0 ? words : 1)));
    if (rows < 1) rows = 1;
    return (int)(rows < (long)n_rows ? rows : (long)n_rows);
}

// The context-owned scratch of a call: the two planes of a row block (block_rows x words each), and per row of the
// block the union's popcount and the position of the row's first edge in the list.
class GraphScratch {
public:
    int ensure(int block_rows, int words, hipStream_t stream, std::string &err);
    void release();
    uint64_t *plane(int which) const { return planes_ + (size_t)which * plane_words_; }
    uint32_t *row_count() const { return row_count_; }
    unsigned long long *row_base() const { return row_base_; }
    long long grows() const { return grows_; }   // allocations so far (msspe_get_info "conflict_graph_grows")

private:
    uint64_t *planes_ = nullptr;
    size_t plane_words_ = 0;
    uint32_t *row_count_ = nullptr;
    unsigned long long *row_base_ = nullptr;
    size_t rows_cap_ = 0;
    long long grows_ = 0;
};

// out[r][w] = any[r][w] | end[r][w] for the rows x words block (out optional; a null plane reads as zeros);
// row_conflicts[r] += popcount of row r (optional; the caller passes the pointer at the block's first row);
// row_count[r] = the same popcount (optional); kind_counts[0..2] += pairs that are ANY only, END only, both (optional).
hipError_t launch_graph_union(const uint64_t *any, const uint64_t *end, int rows, int words, uint64_t *out,
                              uint32_t *row_conflicts, uint32_t *row_count, unsigned long long *kind_counts,
                              hipStream_t stream);
// row_base[r] = *total + sum of row_count[0..r); *total += sum of row_count[0..rows): the running count of the list
// carries the scan from one row block to the next.
hipError_t launch_graph_scan(const uint32_t *row_count, int rows, unsigned long long *row_base,
                             unsigned long long *total, hipStream_t stream);
// The set bits of row r (none where row_count[r] is 0), in ascending column order, go to edges[row_base[r] ...] as (row_first + r, col_first + bit,
// kinds); positions from `capacity` on are dropped.
hipError_t launch_graph_emit(const uint64_t *any, const uint64_t *end, int rows, int words, const uint32_t *row_count,
                             const unsigned long long *row_base, uint32_t row_first, uint32_t col_first,
                             msspe_kind_edge *edges, unsigned long long capacity, hipStream_t stream);

}  // namespace msspe
