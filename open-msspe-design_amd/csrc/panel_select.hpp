// panel_select.hpp -- a conflict-free panel selected by coverage: the greedy set cover of panel_thin.hpp in which a
// pick bars its conflict neighbours from its tube (engine extension, no reference counterpart).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "conflict_cover.hpp"
#include "panel_thin.hpp"

namespace msspe {

class PanelSelect {
public:
    // begin: the buffers of a run over n primers and n_seg segments in groups of S, and the pool (forward words, then
    // reverse words: the order of the bitmap's rows) on the device for CoverStage::prepare; *d_pool_out is that pool.
    // The caller then lets the cover build S = B | B^T (CoverStage::begin / prepare) and writes the incidence matrix
    // (PanelThin::matrix made it) on `stream`, and calls rounds.
    int begin(int n, long n_seg, int S, const uint64_t *fwd_words, int n_fwd, const uint64_t *rev_words, int n_rev,
              const uint64_t **d_pool_out, hipStream_t stream, std::string &err);
    // rounds: the rule of msspe_panel_select* over inc (inc[g * n_pad + p], bit b = segment g * S + b) and sym (the
    // cover's symmetrised bitmap, n x ceil(n / 64) words).  keep_out holds the forced flags on entry.  Outputs as the
    // C call's; barred_out and covered_out are optional.  Returns an msspe_status with the stream idle; err says why.
    // wts (optional): the weighted rule of msspe_panel_select_weighted* (PanelWeights, panel_thin.hpp).  cst (optional):
    // the pick by gain per cost of msspe_panel_select_cost* (PanelCosts, panel_thin.hpp), with or without wts.
    int rounds(const uint64_t *inc, const uint64_t *sym, int n, long n_seg, int S, int min_gain, int max_tubes,
               uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out, uint8_t *tube_out,
               uint8_t *barred_out, uint8_t *covered_out, long long *covered_all_out, long long *covered_kept_out,
               int *n_tubes_used_out, int n_cu, hipStream_t stream, std::string &err,
               const PanelWeights *wts = nullptr, const PanelCosts *cst = nullptr);
    // rounds_depth: the layered rule of msspe_panel_select_depth*  over the same inc and sym: layer 1 is
    // rounds(), layer r then adds primers for the segments that still have fewer than r, the barring carried along.
    // depth is 1..255 (checked by the caller).  pick_layer_out (optional, per position of the order), depth_all_out /
    // depth_kept_out (optional, n_seg bytes, saturating at 255), counts_out[4] (optional): as the C call's.
    int rounds_depth(const uint64_t *inc, const uint64_t *sym, int n, long n_seg, int S, int min_gain, int max_tubes,
                     int depth, uint8_t *keep_out, uint32_t *order_out, uint32_t *gain_out, int *n_picked_out,
                     uint8_t *tube_out, uint8_t *barred_out, int *n_tubes_used_out, uint8_t *pick_layer_out,
                     uint8_t *depth_all_out, uint8_t *depth_kept_out, long long *counts_out, int n_cu,
                     hipStream_t stream, std::string &err);
    void release();
    // the last depth run: its layers, and device time of the column sums and of every layer's init and first gains
    long long depth_layers() const { return layers_; }
    long long depth_layer_us() const { return layer_us_; }
    // the last run: rounds enqueued that ran (the picks and the one that stopped), tubes in use, primers barred, and
    // device time in microseconds of the first state (forced rows, first barring, first gains) and of the rounds
    long long n_rounds() const { return rounds_; }
    long long tubes_used() const { return tubes_; }
    long long barred() const { return barred_; }
    const long long *phase_us() const { return phase_us_; }
    void reset_stats()
    {
        rounds_ = tubes_ = barred_ = layers_ = layer_us_ = 0;
        phase_us_[0] = phase_us_[1] = 0;
    }

private:
    enum { kSlots = 13 };
    void *buf_[kSlots] = {};
    size_t cap_[kSlots] = {};
    hipEvent_t ev_[3] = {};
    hipEvent_t ev_layer_[2] = {};   // around a layer's init and first gains; reused layer after layer
    long long rounds_ = 0, tubes_ = 0, barred_ = 0, layers_ = 0, layer_us_ = 0;
    long long phase_us_[2] = {};
    int ensure(int slot, size_t bytes, std::string &err);
};

}  // namespace msspe
