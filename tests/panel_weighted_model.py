"""numpy restatement of the weighted thinning and selection (msspe_panel_thin_weighted*, msspe_panel_select_weighted*,
include/msspe_hip.h) for small inputs.  The incidence, the graph and the text blocks are the unweighted
models' (panel_thin_model, panel_select_model), imported as they are.

Rule: gain(p) = the sum of w[s] over the segments s with I[p][s] set and covered[s] clear; the pick is the greatest gain,
ties to the lowest index; the loop ends when that gain is below min_gain (weight units).  Covering, forcing, barring and
the tubes are unchanged, so a segment of weight 0 never earns a pick and is still marked when a pick covers it.  With
w = 1 everything equals the unweighted models."""
from __future__ import annotations

import numpy as np

from panel_select_model import TUBE_NONE, check_independent, pack_bitmap, symmetrised, unpack_bitmap  # noqa: F401
from panel_thin_model import incidence, pack_rows  # noqa: F401

LIMIT = 2 ** 32 - 1   # the weights' total: a gain fits 32 bits


def _weights(w, n_seg: int) -> np.ndarray:
    w = np.asarray(w).reshape(-1).astype(object)      # exact integers, whatever the total
    assert w.size == n_seg and all(int(x) >= 0 for x in w)
    assert sum(int(x) for x in w) <= LIMIT
    return np.array([int(x) for x in w], dtype=np.int64)


def _gains(Iw: np.ndarray, covered: np.ndarray) -> np.ndarray:
    """Row sums of Iw = I * w over the uncovered segments.  In float64, which is exact here: every partial sum is a
    non-negative integer of at most 2^32 - 1, whatever the order of the additions."""
    return np.rint(Iw @ (~covered).astype(np.float64)).astype(np.int64)


def greedy_weighted(I, w, min_gain: int = 1, forced=None) -> dict:
    """I: bool (n, N_s); w: N_s non-negative integers.  Returns a dict: keep, order, gains (uint32, weights), covered
    (bool[N_s]), covered_all, covered_kept (segments), weight_all, weight_kept, rounds (the picks and the round that
    stopped)."""
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    w = _weights(w, n_seg)
    forced = np.zeros(n, dtype=bool) if forced is None else np.asarray(forced) != 0
    covered = I[forced].any(axis=0) if forced.any() else np.zeros(n_seg, dtype=bool)
    live = ~forced
    Iw = I.astype(np.float64) * w.astype(np.float64)
    order, gains = [], []
    rounds = 0
    while True:
        rounds += 1
        g = np.where(live, _gains(Iw, covered), -1) if n else np.zeros(0, dtype=np.int64)
        if n == 0 or g.max() < min_gain:   # nobody live: max is -1
            break
        p = int(np.argmax(g))              # the first maximum: the lowest index
        order.append(p)
        gains.append(int(g[p]))
        live[p] = False
        covered = covered | I[p]
    keep = forced.copy()
    keep[np.array(order, dtype=np.int64)] = True
    every = I.any(axis=0) if n else np.zeros(n_seg, dtype=bool)
    return {"keep": keep.astype(np.uint8), "order": np.array(order, dtype=np.uint32),
            "gains": np.array(gains, dtype=np.uint32), "covered": covered, "covered_all": int(every.sum()),
            "covered_kept": int(covered.sum()), "weight_all": int(w[every].sum()), "weight_kept": int(w[covered].sum()),
            "rounds": rounds}


def select_weighted(I, B, w, T: int = 1, min_gain: int = 1, forced=None, drop: bool = False, partner=None) -> dict:
    """panel_select_model.select with the weighted gain.  Returns its dict plus weight_all and weight_kept."""
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    assert 1 <= T <= 64
    w = _weights(w, n_seg)
    S = symmetrised(B, drop, partner)
    assert S.shape == (n, n)
    forced = np.zeros(n, dtype=bool) if forced is None else np.asarray(forced) != 0
    self_c = S.diagonal().copy() if n else np.zeros(0, dtype=bool)
    N = S.copy()
    if n:
        N[np.arange(n), np.arange(n)] = False          # neighbours: u != p
    covered = I[forced].any(axis=0) if forced.any() else np.zeros(n_seg, dtype=bool)
    barred_in = np.zeros((n, T), dtype=bool)           # mask[p], one column per tube
    if forced.any():
        barred_in[N[forced].any(axis=0)] = True
    picked = np.zeros(n, dtype=bool)
    tube = np.full(n, TUBE_NONE, dtype=np.uint8)
    Iw = I.astype(np.float64) * w.astype(np.float64)
    order, gains = [], []
    rounds = 0
    while True:
        rounds += 1
        live = ~forced & ~picked & ~self_c & ~barred_in.all(axis=1)
        g = np.where(live, _gains(Iw, covered), -1) if n else np.zeros(0, dtype=np.int64)
        if n == 0 or not live.any() or g.max() < min_gain:
            break
        p = int(np.argmax(g))                          # the first maximum: the lowest index
        t = int(np.argmin(barred_in[p]))               # the first False: the lowest tube left
        order.append(p)
        gains.append(int(g[p]))
        picked[p] = True
        tube[p] = t
        covered = covered | I[p]
        barred_in[N[p], t] = True
    keep = forced | picked
    barred = ~keep & (self_c | barred_in.all(axis=1))
    used = int(tube[picked].max()) + 1 if picked.any() else 0
    every = I.any(axis=0) if n else np.zeros(n_seg, dtype=bool)
    return {"order": np.array(order, dtype=np.uint32), "gains": np.array(gains, dtype=np.uint32),
            "keep": keep.astype(np.uint8), "tube": tube, "barred": barred.astype(np.uint8), "covered": covered,
            "covered_all": int(every.sum()), "covered_kept": int(covered.sum()), "weight_all": int(w[every].sum()),
            "weight_kept": int(w[covered].sum()), "tubes_used": used, "rounds": rounds}


def weight_line(weight_all: int, weight_kept: int, weight_total: int, n_all: int, n_kept: int) -> str:
    """The line od-msspe-hip --genome-weights adds after `  Segments:` in the thinning and selection blocks."""
    return "  Weight:   covered %d/%d by all %d, %d/%d by the kept %d\n" % (
        weight_all, weight_total, n_all, weight_kept, weight_total, n_kept)


def with_weight_line(block: str, line: str) -> str:
    """A thinning or selection block (render_block of the unweighted models) with the weight line put in."""
    out = []
    for l in block.splitlines(keepends=True):
        out.append(l)
        if l.startswith("  Segments:"):
            out.append(line)
    return "".join(out)
