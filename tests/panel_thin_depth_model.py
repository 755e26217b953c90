"""numpy restatement of the panel thinning to a depth (msspe_panel_thin_depth*, include/msspe_hip.h)
for small inputs.  The incidence I is panel_thin_model.incidence's (the thal forms: panel_thin_thal_model's held one).

Shadows: among primers of one direction with the same word, one is the representative -- the forced one of lowest
index if any is forced, otherwise the lowest index; the others are shadows, count in nothing and are never picked.

Greedy: depth_all[s] = representatives with I[p][s]; need[s] = min(R, depth_all[s]); cnt[s] starts as
min(need[s], forced representatives with I[p][s]); s is open while cnt[s] < need[s].  Every round takes the
representative that is neither forced nor picked with the most open segments, ties to the lowest index; below min_gain
the loop ends and nothing is picked in that round; otherwise cnt[s] += 1 on every open s the pick matches."""
from __future__ import annotations

import numpy as np


def shadows(fwd, rev, forced=None) -> np.ndarray:
    """uint8[len(fwd) + len(rev)]: 1 for a primer that repeats a word of its own direction and is not the word's
    representative.  fwd / rev: strings or packed words."""
    n = len(fwd) + len(rev)
    forced = np.zeros(n, dtype=bool) if forced is None else np.asarray(forced) != 0
    out = np.zeros(n, dtype=np.uint8)
    for words, base in ((list(fwd), 0), (list(rev), len(fwd))):
        groups = {}
        for i, w in enumerate(words):
            groups.setdefault(w if isinstance(w, str) else int(w), []).append(base + i)
        for members in groups.values():
            f = [p for p in members if forced[p]]
            rep = f[0] if f else members[0]
            for p in members:
                out[p] = p != rep
    return out


def greedy_depth(I: np.ndarray, depth: int, min_gain: int = 1, forced=None, shadow=None):
    """(keep uint8[n], order, gains, depth_all uint8[N_s], depth_kept uint8[N_s], counts int64[4], rounds, cnt0, cnt):
    keep is forced-or-picked (a shadow's is its forced flag); the depths saturate at 255; counts = segments with
    depth_all >= 1, depth_kept >= 1, depth_all >= depth, depth_kept >= depth; rounds counts the picks and the round
    that stopped; cnt0 / cnt: the counters before the first round and after the last."""
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    forced = np.zeros(n, dtype=bool) if forced is None else np.asarray(forced) != 0
    shadow = np.zeros(n, dtype=bool) if shadow is None else np.asarray(shadow) != 0
    rep = ~shadow
    all_ = I[rep].sum(axis=0, dtype=np.int64) if n else np.zeros(n_seg, dtype=np.int64)
    need = np.minimum(depth, all_)
    cnt = np.minimum(need, I[rep & forced].sum(axis=0, dtype=np.int64)) if n else np.zeros(n_seg, dtype=np.int64)
    cnt0 = cnt.copy()
    live = rep & ~forced
    order, gains = [], []
    rounds = 0
    while True:
        rounds += 1
        open_ = cnt < need
        g = np.where(live, (I & open_).sum(axis=1), -1) if n else np.zeros(0, dtype=np.int64)
        if n == 0 or g.max() < min_gain:   # nobody live: max is -1
            break
        p = int(np.argmax(g))              # the first maximum: the lowest index
        order.append(p)
        gains.append(int(g[p]))
        live[p] = False
        cnt = cnt + (I[p] & open_)
    keep = forced.copy()
    keep[np.array(order, dtype=np.int64)] = True
    kept = I[keep & rep].sum(axis=0, dtype=np.int64) if n else np.zeros(n_seg, dtype=np.int64)
    counts = np.array([(all_ >= 1).sum(), (kept >= 1).sum(), (all_ >= depth).sum(), (kept >= depth).sum()],
                      dtype=np.int64)
    return (keep.astype(np.uint8), np.array(order, dtype=np.uint32), np.array(gains, dtype=np.uint32),
            np.minimum(all_, 255).astype(np.uint8), np.minimum(kept, 255).astype(np.uint8), counts, rounds, cnt0, cnt)


def render_depth_line(depth: int, deep_all: int, deep_kept: int, segments: int, n_offered: int, n_kept: int) -> str:
    """The line od-msspe-hip --thin-depth R (R > 1) prints after "Segments:"."""
    return "  Depth:    at least %d primers on %d/%d segments by all %d, on %d/%d by the kept %d\n" % (
        depth, deep_all, segments, n_offered, deep_kept, segments, n_kept)
