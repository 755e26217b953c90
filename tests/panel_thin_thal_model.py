"""Restatement of msspe_panel_thin_thal* (include/msspe_hip.h) for small inputs, from the two models it
joins: the scored matches of tests/coverage_thal_model.py and the greedy loop of tests/panel_thin_model.py.

Held incidence: H[p][s] is True when primer p (forward primers first, then reverse) has at least one STABLE match in
segment s = r * P + j -- a match of the mm rule whose thal score against the strand the primer anneals to gives
t_match = max(0, t) with not (round_fixed_f32(t_match, 2) < float32(tm_threshold)).  A row sum of H is
msspe_segment_coverage_thal's primer_held[p]; a threshold <= 0 makes H the string rule's incidence I.

Greedy: panel_thin_model.greedy over H, unchanged.  Also renders the block od-msspe-hip --thin-panel true --thin-tm T
prints."""
from __future__ import annotations

import numpy as np

import coverage_thal_model as ctm
import panel_thin_model as tm
from panel_thin_model import greedy, pack_rows  # noqa: F401  (the loop and the host hook's row form, as they stand)


def held_incidence(result: dict) -> np.ndarray:
    """bool (n primers, n_seq * P) from what coverage_thal_model.coverage_thal (or rethreshold) returns."""
    n = len(result["primer_held"])
    H = np.zeros((n, result["held"].size), dtype=bool)
    recs = result["matches"]
    st = recs["stable"] != 0
    H[recs["primer"][st].astype(np.int64), recs["segment"][st].astype(np.int64)] = True
    return H


def distinct_pairs(result: dict) -> int:
    """(primer, template oligo) pairs among the matches: what the call scores with thin_thal_unique 1."""
    return len(set(zip(result["matches"]["primer"].tolist(), result["templates"])))


def thin_thal(tables, seqs, seg: int, stride: int, W: int, k: int, fwd, rev, M: int, E: int, mode, tm_threshold: float,
              args=None, min_gain: int = 1, forced=None, chunk: int = 64, cache=None):
    """(H, panel_thin_model.greedy(H, min_gain, forced), the scored result)."""
    res = ctm.coverage_thal(tables, seqs, seg, stride, W, k, fwd, rev, M, E, mode, tm_threshold, args, chunk, cache)
    H = held_incidence(res)
    return H, tm.greedy(H, min_gain, forced), res


def render_block(mode, tm_threshold: float, M: int, E: int, G: int, kept_f: int, n_f: int, kept_r: int, n_r: int,
                 forced: int, held_all: int, held_kept: int, segments: int) -> str:
    """The text od-msspe-hip --thin-panel true --thin-tm T prints in place of panel_thin_model.render_block's: the
    primer figures leave the forced primers out, the segment figures include what they hold."""
    name = {1: "ANY", 2: "END1", "any": "ANY", "end1": "END1"}[mode]
    x, y = kept_f + kept_r, n_f + n_r
    return ("\nPanel thinning (thal %s, t >= %.2f C; matches within %d mismatches, last %d bases exact, gain >= %d):\n" % (
                name, float(np.float32(tm_threshold)), M, E, G) +
            "  Primers:  kept %d of %d (forward %d of %d, reverse %d of %d), %d forced\n" % (
                x, y, kept_f, n_f, kept_r, n_r, forced) +
            "  Segments: held %d/%d by all %d, %d/%d by the kept %d\n" % (
                held_all, segments, y, held_kept, segments, x))
