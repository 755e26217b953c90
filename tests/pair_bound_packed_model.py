"""Plain-Python side of the PACKED bound first stage (csrc/thal_pairs_row.hip k_pairs_bound_packed; csrc/fast_tables.hpp
BoundPacked): the recurrence is pair_bound_model's -- the minimum over all chains of integer terms -- run on the
coarse tables of msspe_host_bound_packed, whose terms are the exact-unit ones floored to 2**(shift - 6) cal/mol.
Integer addition is what the device does as well, so the device's value is this very integer times the unit.

Test infrastructure: the tables in the shape pair_bound_model's functions take, and the recurrence with every cell's
value kept (the slot word's 15-bit field must hold each of them)."""
from __future__ import annotations

import param_variants as pv
from int_dp_model import CODE, K_ROWS, cell_bases

VOID = 500000000   # fast_tables.hpp IntTables::kValid: entries at or above it are "not available"


def packed_tables(m, path=None, chem=None, threshold: float = -9000.0) -> dict:
    """host_bound_packed's tables as a dict pair_bound_model.bound_pair takes: unit_inv is units per cal/mol (1, 1/2,
    1/4), unit the cal/mol per unit."""
    p = m.capi.host_bound_packed(path, chem or m.Chem.ntthal(), threshold)
    if p["usable"]:
        p["unit"] = float(1 << (p["shift"] - 6))
        p["unit_inv"] = 1.0 / p["unit"]
    p["void"] = VOID
    return p


def cells_and_pick(bt: dict, a: str, b: str):
    """(the value of every complementary cell in the kernel's order, the minimum over cells of value + right end term |
    None: no cell) in table units, before the initiation.  pair_bound_model._min_chain without the trace."""
    g, T, void = bt["g"], bt["T"], bt["void"]
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
            for pi, pj, Gp, po in cells:
                l1, l2 = im1 - 1 - pi, jm1 - 1 - pj
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
            cells.append((im1, jm1, best, cb["po"]))
            values.append(best)
            end = best + int(g[cb["idxR"]])
            pick = end if pick is None else min(pick, end)
    return values, pick


def plane_model(bt: dict, rows, cols):
    """cells_and_pick for every (row, column) pair at once (numpy over the pairs; the Python loop takes 4 ms a pair):
    (pick as int64 per pair with NONE where the pair has no cell, smallest and largest cell value over all pairs).
    Works on the exact-unit tables and on the coarse ones alike.  Pinned to cells_and_pick by the CPU suite."""
    import numpy as np
    import int_dp_model as im
    g, T, void = bt["g"].astype(np.int64), bt["T"].astype(np.int64), bt["void"]
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
            for pi in range(im1):
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
            G[im1, jm1] = np.where(ok, best, NONE)
            PO[im1, jm1] = a | ((oaR & 3) << 2) | ((obR & 3) << 4)
            vmin, vmax = min(vmin, int(best[ok].min())), max(vmax, int(best[ok].max()))
            end = best + g[im.K_ENDR + a * 25 + oaR * 5 + obR]
            pick = np.where(ok, np.minimum(pick, end), pick)
    return pick.reshape(R, Cn), vmin, vmax


NONE = 1 << 40   # plane_model: no cell / no chain


def packed_bound_pair(pk: dict, a: str, b: str):
    """The packed instance's bound of (a, b) in cal/mol (an integer multiple of the unit); None: no chain."""
    _, pick = cells_and_pick(pk, a, b)
    return None if pick is None else (pick + pk["init"]) * pk["unit"]


def unpackable_sections():
    """The stock bundle with every terminal-mismatch enthalpy of tstack.dh lowered by 6000 cal/mol: interior loops and
    their cell-side terms get so cheap that 12 steps of the proven range pass 4 cal/mol x 2^15 -- the bound tables stay
    usable (and every route), the packed instance does not."""
    return pv._mapped(pv.stock_sections(), {"tstack.dh": lambda i, v: v - 6000})
