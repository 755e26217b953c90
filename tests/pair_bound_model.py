"""Plain-Python restatement of the bound first stage (csrc/thal_pairs_row.hip k_pairs_bound): the minimum over all
chains  left end term, (stacked pair | loop)*, right end term, initiation  of the rounded-down integer terms of
msspe_host_bound_tables.  Test infrastructure: lets the CPU suite check the tables and the lower-bound argument
against the oracle without a GPU.  Indices as in int_dp_model.py."""
from __future__ import annotations

from int_dp_model import CODE, K_ROWS, cell_bases


def bound_pair(bt: dict, a: str, b: str):
    """The bound of thal ANY's dG for (a, b) in cal/mol; None: no complementary cell (no chain)."""
    g, T, void = bt["g"], bt["T"], bt["void"]
    s1 = [CODE[c] for c in a]
    s2 = [CODE[c] for c in reversed(b)]
    k = len(a)
    cells = []   # (im1, jm1, value, po)
    pick = None
    for im1 in range(k):
        for jm1 in range(k):
            if s1[im1] + s2[jm1] != 3:
                continue
            cb = cell_bases(s1, s2, im1, jm1)
            a4 = cb["a"] << 2
            yTS, yMM = int(g[cb["yTS"]]), int(g[cb["yMM"]])
            best = int(g[cb["idxL"]])
            assert best < void
            for (pi, pj, Gp, po) in cells:
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
            end = best + int(g[cb["idxR"]])
            pick = end if pick is None else min(pick, end)
    if pick is None:
        return None
    return (pick + bt["init"]) / bt["unit_inv"]
