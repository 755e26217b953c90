"""numpy restatement of the selection by coverage (msspe_panel_select*, include/msspe_hip.h) for small
inputs: the greedy set cover of tests/panel_thin_model.py in which a pick bars its conflict neighbours from its tube.

Graph: S = B | B^T over the primers' indices; with drop the diagonal is cleared first (and the pairs in `partner`, the
reverse-complement partners, when the caller names any -- the model knows no words).  p is self-conflicting when
S[p][p] is still set.
State: covered = OR of the forced rows; mask[p] = the tubes barred to p -- all T for every neighbour of a forced
primer, else none; p is live when it is not forced, not picked, not self-conflicting and has a tube left.
Rounds: the live p of greatest gain |I[p] & ~covered|, ties to the lowest index; below min_gain, or with nobody live,
the loop ends.  Otherwise p takes the lowest tube its mask leaves, covered |= I[p], and that tube is barred to every
u != p with S[p][u]."""
from __future__ import annotations

import numpy as np

TUBE_NONE = 255


def symmetrised(B, drop: bool = False, partner=None) -> np.ndarray:
    B = np.asarray(B, dtype=bool)
    n = B.shape[0]
    S = (B | B.T).copy() if n else np.zeros((0, 0), dtype=bool)
    if drop and n:
        S[np.arange(n), np.arange(n)] = False
        if partner is not None:
            for a, b in enumerate(partner):
                if b >= 0:
                    S[a, b] = S[b, a] = False
    return S


def select(I, B, T: int = 1, min_gain: int = 1, forced=None, drop: bool = False, partner=None) -> dict:
    """I: bool (n, N_s) incidence; B: bool (n, n), B[p][u] = the directed conflict p -> u.  Returns a dict: order,
    gains (uint32), keep, tube (uint8; 255 = none), barred (uint8), covered (bool[N_s]), covered_all, covered_kept,
    tubes_used, rounds (the picks and the round that stopped)."""
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    assert 1 <= T <= 64
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
        g = np.where(live, (I & ~covered).sum(axis=1), -1) if n else np.zeros(0, dtype=np.int64)
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
    return {"order": np.array(order, dtype=np.uint32), "gains": np.array(gains, dtype=np.uint32),
            "keep": keep.astype(np.uint8), "tube": tube, "barred": barred.astype(np.uint8), "covered": covered,
            "covered_all": int(I.any(axis=0).sum()) if n else 0, "covered_kept": int(covered.sum()),
            "tubes_used": used, "rounds": rounds}


def check_independent(res: dict, B, forced=None, drop: bool = False, partner=None) -> None:
    """The guarantees: no two picks of one tube are neighbours, no pick neighbours a forced primer or itself, the
    tubes in use are 0 .. used - 1 without gaps, and exactly the picks have a tube."""
    S = symmetrised(B, drop, partner)
    n = S.shape[0]
    forced = np.zeros(n, dtype=bool) if forced is None else np.asarray(forced) != 0
    tube, order = np.asarray(res["tube"]), np.asarray(res["order"], dtype=np.int64)
    picked = np.zeros(n, dtype=bool)
    picked[order] = True
    assert len(set(order.tolist())) == len(order) and not (picked & forced).any()
    assert ((tube != TUBE_NONE) == picked).all()
    assert not S.diagonal()[picked].any()
    if forced.any():
        assert not S[forced][:, picked].any()
    for t in range(res["tubes_used"]):
        members = np.flatnonzero(picked & (tube == t))
        assert members.size, "a gap among the tubes in use"
        assert not S[np.ix_(members, members)].any()
    assert not (picked & (tube >= max(res["tubes_used"], 0)) & (tube != TUBE_NONE)).any()


def pack_bitmap(B) -> np.ndarray:
    """bool (n, n) -> uint64 (n, ceil(n / 64)), bit u & 63 of word u >> 6 of row p: msspe_cross_dimer_dev's layout."""
    B = np.asarray(B, dtype=bool)
    n = B.shape[0]
    words = (n + 63) // 64
    padded = np.zeros((n, words * 64), dtype=np.uint8)
    padded[:, :n] = B
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(n, words))


def unpack_bitmap(words, n: int) -> np.ndarray:
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(n, (n + 63) // 64)
    bits = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little") if n else np.zeros((0, 0), dtype=np.uint8)
    return bits[:, :n].astype(bool)


def render_block(mode, tm_threshold: float, M: int, E: int, G: int, T: int, kept_f: int, n_f: int, kept_r: int,
                 n_r: int, forced: int, barred: int, covered_all: int, covered_kept: int, segments: int,
                 per_tube=None) -> str:
    """The text od-msspe-hip --select-by-coverage true prints after the coverage report(s).  mode 0: the string rule;
    1 / 2 (or "any" / "end1"): the held rule at tm_threshold.  The primer figures leave the forced primers out, the
    segment figures include what they cover; per_tube (with --tubes): the kept primers of tubes 0 .. used - 1, which
    the text numbers from 1."""
    mode = {0: 0, 1: 1, 2: 2, "any": 1, "end1": 2}[mode]
    x, y = kept_f + kept_r, n_f + n_r
    if mode:
        rule = "thal %s, t >= %.2f C; matches within %d mismatches, last " % (
            "END1" if mode == 2 else "ANY", float(np.float32(tm_threshold)), M)
    else:
        rule = "up to %d mismatches, last " % M
    s = ("\nPanel selection by coverage (%s%d bases exact, gain >= %d, tubes <= %d):\n" % (rule, E, G, T) +
         "  Rule:     each round keeps the primer with the most new segments and bars its conflict neighbours from its "
         "tube\n" +
         "  Primers:  kept %d of %d (forward %d of %d, reverse %d of %d), %d forced\n" % (
             x, y, kept_f, n_f, kept_r, n_r, forced) +
         "  Barred:   %d by conflicts\n" % barred +
         "  Segments: %s %d/%d by all %d, %d/%d by the kept %d\n" % (
             "held" if mode else "covered", covered_all, segments, y, covered_kept, segments, x))
    for t, c in enumerate(per_tube if per_tube is not None else ()):
        s += "  Tube %d: %d primers\n" % (t + 1, c)       # numbered from 1, as the CSV's column
    return s
