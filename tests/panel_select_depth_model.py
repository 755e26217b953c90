"""numpy restatement of the selection to a coverage depth (msspe_panel_select_depth*, include/msspe_hip.h; DESIGN.md
4.16) for small inputs: the selection of tests/panel_select_model.py run in layers.

Graph, self-conflicting, mask, live and the tube choice are panel_select_model's.  State carried through the whole run:
depth_all[s] = primers with I[p][s] (conflicts ignored), cnt[s] = kept (forced or picked) primers with I[p][s], the
true count, starting from the forced rows.  Layers r = 1 .. L, L = min(R, max(1, max_s depth_all[s])).  In layer r a
segment is open while cnt[s] < min(r, depth_all[s]); a round takes the live p with the most open segments (ties: the
lowest index); nobody live, or that gain below min_gain, ends the layer (the stopping round counts).  A pick takes the
lowest tube its mask leaves, adds 1 to cnt on EVERY segment of its row, open or not, and bars its tube to its
neighbours.  Picks, barring and cnt carry over from layer to layer."""
from __future__ import annotations

import numpy as np

from panel_select_model import TUBE_NONE, render_block, symmetrised


def select_depth(I, B, R: int = 1, T: int = 1, min_gain: int = 1, forced=None, drop: bool = False,
                 partner=None) -> dict:
    """I: bool (n, N_s); B: bool (n, n) directed conflicts.  Returns a dict: order, gains (uint32), layer (uint8, the
    layer of every pick), keep, tube (255 = none), barred, depth_all, depth_kept (uint8[N_s], saturating at 255),
    counts (int64[4]: segments with depth_all >= 1, depth_kept >= 1, depth_all >= R, depth_kept >= R), tubes_used,
    rounds (picks + layers), layers, and layer_sums (per layer: the sum over the segments of the hits taken while
    open, which equals the sum of the layer's gains)."""
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    assert 1 <= T <= 64 and 1 <= R <= 255
    S = symmetrised(B, drop, partner)
    assert S.shape == (n, n)
    forced = np.zeros(n, dtype=bool) if forced is None else np.asarray(forced) != 0
    self_c = S.diagonal().copy() if n else np.zeros(0, dtype=bool)
    N = S.copy()
    if n:
        N[np.arange(n), np.arange(n)] = False
    depth_all = I.sum(axis=0).astype(np.int64)
    cnt = I[forced].sum(axis=0).astype(np.int64) if forced.any() else np.zeros(n_seg, dtype=np.int64)
    barred_in = np.zeros((n, T), dtype=bool)
    if forced.any():
        barred_in[N[forced].any(axis=0)] = True
    picked = np.zeros(n, dtype=bool)
    tube = np.full(n, TUBE_NONE, dtype=np.uint8)
    order, gains, layer, layer_sums = [], [], [], []
    D = int(depth_all.max()) if n and n_seg else 0
    layers = min(R, max(1, D))
    rounds = 0
    for r in range(1, layers + 1):
        need = np.minimum(r, depth_all)
        start = np.minimum(cnt, need)
        while True:
            rounds += 1
            live = ~forced & ~picked & ~self_c & ~barred_in.all(axis=1)
            is_open = cnt < need
            g = np.where(live, (I & is_open).sum(axis=1), -1) if n else np.zeros(0, dtype=np.int64)
            if n == 0 or not live.any() or g.max() < min_gain:
                break
            p = int(np.argmax(g))
            t = int(np.argmin(barred_in[p]))
            order.append(p)
            gains.append(int(g[p]))
            layer.append(r)
            picked[p] = True
            tube[p] = t
            cnt = cnt + I[p]
            barred_in[N[p], t] = True
        layer_sums.append(int((np.minimum(cnt, need) - start).sum()))
    keep = forced | picked
    barred = ~keep & (self_c | barred_in.all(axis=1))
    used = int(tube[picked].max()) + 1 if picked.any() else 0
    counts = np.array([(depth_all >= 1).sum(), (cnt >= 1).sum(), (depth_all >= R).sum(), (cnt >= R).sum()],
                      dtype=np.int64)
    return {"order": np.array(order, dtype=np.uint32), "gains": np.array(gains, dtype=np.uint32),
            "layer": np.array(layer, dtype=np.uint8), "keep": keep.astype(np.uint8), "tube": tube,
            "barred": barred.astype(np.uint8), "depth_all": np.minimum(depth_all, 255).astype(np.uint8),
            "depth_kept": np.minimum(cnt, 255).astype(np.uint8), "counts": counts, "tubes_used": used,
            "rounds": rounds, "layers": layers, "layer_sums": layer_sums}


def unlayered(I, B, R: int, T: int = 1, min_gain: int = 1) -> dict:
    """The rule the layers replace (the depth thinning's, with barring added): ONE loop in which a segment is open
    while cnt < min(R, depth_all).  Kept only to show what it costs: a pick made for its second-primer gains bars the
    only primer of other segments.  Returns order and counts as select_depth."""
    I = np.asarray(I, dtype=bool)
    n = I.shape[0]
    S = symmetrised(B)
    self_c = S.diagonal().copy()
    N = S.copy()
    N[np.arange(n), np.arange(n)] = False
    depth_all = I.sum(axis=0).astype(np.int64)
    need = np.minimum(R, depth_all)
    cnt = np.zeros_like(depth_all)
    barred_in = np.zeros((n, T), dtype=bool)
    picked = np.zeros(n, dtype=bool)
    order = []
    while True:
        live = ~picked & ~self_c & ~barred_in.all(axis=1)
        g = np.where(live, (I & (cnt < need)).sum(axis=1), -1)
        if not live.any() or g.max() < min_gain:
            break
        p = int(np.argmax(g))
        t = int(np.argmin(barred_in[p]))
        order.append(p)
        picked[p] = True
        cnt = cnt + I[p]
        barred_in[N[p], t] = True
    counts = np.array([(depth_all >= 1).sum(), (cnt >= 1).sum(), (depth_all >= R).sum(), (cnt >= R).sum()],
                      dtype=np.int64)
    return {"order": np.array(order, dtype=np.uint32), "counts": counts}


def render_depth_block(mode, tm_threshold: float, M: int, E: int, G: int, T: int, R: int, kept_f: int, n_f: int,
                       kept_r: int, n_r: int, forced: int, barred: int, counts, segments: int, per_tube=None) -> str:
    """The text od-msspe-hip --select-by-coverage true --select-depth R prints, R > 1: panel_select_model.render_block
    with ", depth R" closing the first line's bracket and the depth thinning's "Depth:" line after "Segments:"."""
    assert R > 1
    x, y = kept_f + kept_r, n_f + n_r
    base = render_block(mode, tm_threshold, M, E, G, T, kept_f, n_f, kept_r, n_r, forced, barred, int(counts[0]),
                        int(counts[1]), segments, None)
    head, rest = base.split("):\n", 1)
    s = head + ", depth %d):\n" % R + rest
    s += "  Depth:    at least %d primers on %d/%d segments by all %d, on %d/%d by the kept %d\n" % (
        R, int(counts[2]), segments, y, int(counts[3]), segments, x)
    for t, c in enumerate(per_tube if per_tube is not None else ()):
        s += "  Tube %d: %d primers\n" % (t + 1, c)
    return s
