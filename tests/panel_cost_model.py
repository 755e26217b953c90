"""Restatement of the thinning and selection by gain per cost (msspe_panel_thin_cost*, msspe_panel_select_cost*,
include/msspe_hip.h) for small inputs, in Python integers.  The incidence, the graph, the weights' checks
and the text blocks are the earlier models' (panel_thin_model, panel_select_model, panel_weighted_model), imported as
they are.

Rule: gain(p) is the weighted models' (with w = None every segment counts 1).  A round considers the live primers whose
gain is at least min_gain and picks the greatest gain(p) / cost(p), compared by cross products -- p beats q when
gain(p) * cost(q) > gain(q) * cost(p) -- then the greater gain, then the lowest index.  No quotient is ever formed.
Covering, forcing, barring and the tubes are unchanged.  With all costs equal everything equals the sibling models."""
from __future__ import annotations

import numpy as np

from panel_select_model import TUBE_NONE, check_independent, pack_bitmap, symmetrised, unpack_bitmap  # noqa: F401
from panel_thin_model import incidence, pack_rows  # noqa: F401
from panel_weighted_model import LIMIT, _weights, weight_line, with_weight_line  # noqa: F401


def _costs(costs, n: int) -> list:
    c = [int(x) for x in np.asarray(costs, dtype=object).reshape(-1)]
    assert len(c) == n and all(1 <= x <= LIMIT for x in c)
    return c


def _rows(I: np.ndarray, w) -> tuple:
    """Per primer the list of (segment, weight) it matches in: the gains below are plain integer sums."""
    n, n_seg = I.shape
    wl = [1] * n_seg if w is None else [int(x) for x in _weights(w, n_seg)]
    return [[(int(s), wl[int(s)]) for s in np.flatnonzero(I[p])] for p in range(n)], wl


def beats(gain_a: int, cost_a: int, gain_b: int, cost_b: int) -> bool:
    """a before b among equal indices' betters: the cross products, then the gain.  Python integers: exact."""
    ab, ba = gain_a * cost_b, gain_b * cost_a
    return ab > ba if ab != ba else gain_a > gain_b


def _pick(live, gains, costs, min_gain: int):
    best = -1
    for p in range(len(costs)):          # ascending, and "beats" is strict: the lowest index among equals
        if not live[p] or gains[p] < min_gain:
            continue
        if best < 0 or beats(gains[p], costs[p], gains[best], costs[best]):
            best = p
    return best


def greedy_cost(I, costs, w=None, min_gain: int = 1, forced=None) -> dict:
    """I: bool (n, N_s); costs: n integers >= 1; w: N_s non-negative integers or None.  Returns greedy_weighted's dict
    plus cost_all and cost_kept (without weights weight_all / weight_kept are the two covered counts)."""
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    costs = _costs(costs, n)
    rows, wl = _rows(I, w)
    forced = np.zeros(n, dtype=bool) if forced is None else np.asarray(forced) != 0
    covered = I[forced].any(axis=0) if forced.any() else np.zeros(n_seg, dtype=bool)
    live = [not f for f in forced]
    order, gains = [], []
    rounds = 0
    while True:
        rounds += 1
        g = [sum(x for s, x in rows[p] if not covered[s]) for p in range(n)]
        p = _pick(live, g, costs, min_gain)
        if p < 0:
            break
        order.append(p)
        gains.append(g[p])
        live[p] = False
        covered = covered | I[p]
    keep = forced.copy()
    keep[np.array(order, dtype=np.int64)] = True
    every = I.any(axis=0) if n else np.zeros(n_seg, dtype=bool)
    return {"keep": keep.astype(np.uint8), "order": np.array(order, dtype=np.uint32),
            "gains": np.array(gains, dtype=np.uint32), "covered": covered, "covered_all": int(every.sum()),
            "covered_kept": int(covered.sum()), "weight_all": sum(wl[s] for s in np.flatnonzero(every)),
            "weight_kept": sum(wl[s] for s in np.flatnonzero(covered)), "rounds": rounds,
            "cost_all": sum(costs), "cost_kept": sum(c for c, k in zip(costs, keep) if k)}


def select_cost(I, B, costs, w=None, T: int = 1, min_gain: int = 1, forced=None, drop: bool = False,
                partner=None) -> dict:
    """panel_select_model.select with the pick by gain per cost.  Returns select_weighted's dict plus cost_all and
    cost_kept."""
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    assert 1 <= T <= 64
    costs = _costs(costs, n)
    rows, wl = _rows(I, w)
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
    order, gains = [], []
    rounds = 0
    while True:
        rounds += 1
        live = ~forced & ~picked & ~self_c & ~barred_in.all(axis=1)
        g = [sum(x for s, x in rows[p] if not covered[s]) for p in range(n)]
        p = _pick(live, g, costs, min_gain)
        if p < 0:
            break
        t = int(np.argmin(barred_in[p]))               # the first False: the lowest tube left
        order.append(p)
        gains.append(g[p])
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
            "covered_all": int(every.sum()), "covered_kept": int(covered.sum()),
            "weight_all": sum(wl[s] for s in np.flatnonzero(every)),
            "weight_kept": sum(wl[s] for s in np.flatnonzero(covered)), "tubes_used": used, "rounds": rounds,
            "cost_all": sum(costs), "cost_kept": sum(c for c, k in zip(costs, keep) if k)}


def cost_line(cost_kept: int, cost_all: int, n_kept: int, n_all: int) -> str:
    """The line od-msspe-hip --primer-costs / --background-site-cost adds after `  Segments:` (after `  Weight:` when
    there is one) in the thinning and selection blocks; forced primers count in all four figures."""
    return "  Cost:     %d/%d by the kept %d of %d\n" % (cost_kept, cost_all, n_kept, n_all)


def with_cost_line(block: str, line: str, weight: str = "") -> str:
    """A thinning or selection block (render_block of the unweighted models) with the weight line, if any, and the
    cost line put in."""
    return with_weight_line(block, weight + line)


# the exactness case: two segments of weight 1 and 2^32 - 2; p0 covers both at cost 2^32 - 2, p1 the heavy one at cost
# 2^32 - 3.  The cross products differ by 1 (p1's is the greater) while the quotients are equal in binary64 and binary32.
EXACT_I = np.array([[True, True], [False, True]])
EXACT_W = [1, 2 ** 32 - 2]
EXACT_COSTS = [2 ** 32 - 2, 2 ** 32 - 3]
