"""Plain-Python side of the WINDOWED packed bound first stage (csrc/thal_pairs_row.hip k_pairs_bound_window;
csrc/fast_tables.hpp BoundWindow): pair_bound_packed_model's recurrence on the same coarse tables, except that a cell of
row i visits only the predecessors of the rows i-F .. i-1 one by one.  Every row above them is ONE candidate

    farmin(i) + min(bfar, ifar + yTS(cell))

farmin(i): the smallest value of any cell of the rows <= i-1-F, whatever its column; ifar / bfar: the smallest finite
coarse table entry over l1 >= F with l2 >= 1 / l2 = 0 (msspe_host_bound_window).  A void yTS leaves bfar alone, a void
bfar the other branch, no cell up there no candidate.  The device may visit some of the far rows' slots exactly as well
(those that share a chunk with the window's first slot); their exact candidates are never below the far candidate, so
the value has no notion of chunks.

Test infrastructure: the constants beside the packed tables, the recurrence pair by pair with every cell's value kept,
and a numpy form over whole planes pinned to it."""
from __future__ import annotations

from int_dp_model import CODE, K_ROWS, cell_bases
from pair_bound_packed_model import NONE, packed_tables


def window_tables(m, path=None, chem=None, threshold: float = -9000.0) -> dict:
    """packed_tables' dict with the windowed instance's constants under "window" (host_bound_window's dict)."""
    pk = packed_tables(m, path, chem, threshold)
    pk["window"] = m.capi.host_bound_window(path, chem or m.Chem.ntthal(), threshold)
    return pk


def far_constants(pk: dict, F: int):
    """(ifar, bfar) restated from the exported coarse T: minima over the finite entries of the rows d = 16 l1 + l2 with
    l1 >= F; None where there is none."""
    T, void = pk["T"], pk["void"]
    ifar = bfar = None
    for d in range(K_ROWS):
        l1, l2 = d >> 4, d & 15
        if l1 < F:
            continue
        row = [int(v) for v in T[d * 64:d * 64 + 64] if v < void]
        if not row:
            continue
        if l2 == 0:
            bfar = min(row) if bfar is None else min(bfar, min(row))
        else:
            ifar = min(row) if ifar is None else min(ifar, min(row))
    return ifar, bfar


def _consts(pk: dict):
    w = pk["window"]
    assert w["usable"] == 1
    fin = lambda v: None if v >= w["void"] else int(v)
    return w["F"], fin(w["ifar"]), fin(w["bfar"])


def cells_and_pick(pk: dict, a: str, b: str):
    """pair_bound_packed_model.cells_and_pick under the window: (every cell's value in the kernel's order, the minimum
    over cells of value + right end term | None) in table units, before the initiation."""
    g, T, void = pk["g"], pk["T"], pk["void"]
    F, ifar, bfar = _consts(pk)
    s1 = [CODE[c] for c in a]
    s2 = [CODE[c] for c in reversed(b)]
    k = len(a)
    cells, values, pick = [], [], None
    for im1 in range(k):
        for jm1 in range(k):
            if s1[im1] + s2[jm1] != 3:
                continue
            cb = cell_bases(s1, s2, im1, jm1)
            a4 = cb["a"] << 2
            yTS, yMM = int(g[cb["yTS"]]), int(g[cb["yMM"]])
            best = int(g[cb["idxL"]])
            assert best < void
            farmin = None
            for pi, pj, Gp, po in cells:
                l1, l2 = im1 - 1 - pi, jm1 - 1 - pj
                if l1 >= F:      # above the window: whatever its column
                    farmin = Gp if farmin is None else min(farmin, Gp)
                    continue
                if l1 < 0 or l2 < 0:
                    continue
                d = l1 * 16 + l2
                if d == 0:
                    t, y = int(g[cb["wc"]]), 0
                else:
                    bulge = l1 == 0 or l2 == 0
                    t = int(T[min(d * 64 + (((po & 3) | a4) if bulge else po), K_ROWS * 64 - 1)])
                    y = yMM if d == 0x11 else (0 if bulge else yTS)
                if t >= void or y >= void:
                    continue
                best = min(best, t + y + Gp)
            if farmin is not None:
                steps = ([bfar] if bfar is not None else []) + ([ifar + yTS] if ifar is not None and yTS < void else [])
                if steps:
                    best = min(best, farmin + min(steps))
            cells.append((im1, jm1, best, cb["po"]))
            values.append(best)
            end = best + int(g[cb["idxR"]])
            pick = end if pick is None else min(pick, end)
    return values, pick


def window_bound_pair(pk: dict, a: str, b: str):
    """The windowed instance's bound of (a, b) in cal/mol (a multiple of the unit); None: no chain."""
    _, pick = cells_and_pick(pk, a, b)
    return None if pick is None else (pick + pk["init"]) * pk["unit"]


def plane_model(pk: dict, rows, cols):
    """cells_and_pick for every (row, column) pair at once: pair_bound_packed_model.plane_model under the window.
    (pick as int64 per pair with NONE where the pair has no cell, smallest and largest cell value over all pairs)."""
    import numpy as np
    import int_dp_model as im
    g, T, void = pk["g"].astype(np.int64), pk["T"].astype(np.int64), pk["void"]
    F, ifar, bfar = _consts(pk)
    k, R, Cn = len(rows[0]), len(rows), len(cols)
    S1 = np.array([[CODE[c] for c in a] for a in rows], dtype=np.int64)
    S2 = np.array([[CODE[c] for c in reversed(b)] for b in cols], dtype=np.int64)
    pad = lambda s: np.concatenate([np.full((len(s), 1), 4), s, np.full((len(s), 1), 4)], axis=1)   # [:, x] = base x - 1
    s1, s2 = np.repeat(pad(S1), Cn, axis=0), np.tile(pad(S2), (R, 1))
    P = R * Cn
    G = np.full((k, k, P), NONE, dtype=np.int64)
    PO = np.zeros((k, k, P), dtype=np.int64)
    pick = np.full(P, NONE, dtype=np.int64)
    vmin, vmax = NONE, -NONE
    for im1 in range(k):
        # the smallest value of the rows <= im1 - 1 - F (NONE: no cell there)
        farmin = G[:im1 - F].min(axis=(0, 1)) if im1 - F > 0 else np.full(P, NONE, dtype=np.int64)
        for jm1 in range(k):
            a = s1[:, im1 + 1]
            ok = a + s2[:, jm1 + 1] == 3
            if not ok.any():
                continue
            oaL, oaR, obL, obR = s1[:, im1], s1[:, im1 + 2], s2[:, jm1], s2[:, jm1 + 2]
            ci = (((3 - a) * 4 + (obL & 3)) * 4 + (oaL & 3)) & 63
            best = g[im.K_ENDL + a * 25 + oaL * 5 + obL].copy()
            assert (best[ok] < void).all()
            yTS, yMM, wc, a4 = g[im.K_TSC + ci], g[im.K_MMC + ci], g[im.K_WC + (oaL & 3) * 4 + a], a << 2
            for pi in range(max(0, im1 - F), im1):
                for pj in range(jm1):
                    l1, l2 = im1 - 1 - pi, jm1 - 1 - pj
                    d = l1 * 16 + l2
                    Gp = G[pi, pj]
                    if d == 0:
                        t, y = wc, 0
                    else:
                        bulge = l1 == 0 or l2 == 0
                        po = PO[pi, pj]
                        t = T[np.minimum(d * 64 + (((po & 3) | a4) if bulge else po), K_ROWS * 64 - 1)]
                        y = yMM if d == 0x11 else (0 if bulge else yTS)
                    bad = (Gp == NONE) | (t >= void) | (y >= void)
                    best = np.minimum(best, np.where(bad, NONE, t + y + Gp))
            step = np.full(P, NONE, dtype=np.int64)
            if bfar is not None:
                step = np.minimum(step, bfar)
            if ifar is not None:
                step = np.minimum(step, np.where(yTS >= void, NONE, ifar + yTS))
            best = np.minimum(best, np.where((farmin == NONE) | (step == NONE), NONE, farmin + step))
            G[im1, jm1] = np.where(ok, best, NONE)
            PO[im1, jm1] = a | ((oaR & 3) << 2) | ((obR & 3) << 4)
            vmin, vmax = min(vmin, int(best[ok].min())), max(vmax, int(best[ok].max()))
            end = best + g[im.K_ENDR + a * 25 + oaR * 5 + obR]
            pick = np.where(ok, np.minimum(pick, end), pick)
    return pick.reshape(R, Cn), vmin, vmax
