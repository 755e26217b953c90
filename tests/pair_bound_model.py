"""Plain-Python restatement of the bound first stage (csrc/thal_pairs_row.hip k_pairs_bound): the minimum over all
chains  left end term, (stacked pair | loop)*, right end term, initiation  of the rounded-down integer terms of
msspe_host_bound_tables.  Test infrastructure: lets the CPU suite check the tables and the lower-bound argument
against the oracle without a GPU, and gives the GPU suite the integer the device must report.  Indices as in
int_dp_model.py.

Also here: the sizing rule of wave_pairs_row<52, true> for a wave of one base composition (which pairs the stage hands
on unbounded), the constructed two-stem pairs whose winning chains take long loops, and a parameter bundle under which
they do."""
from __future__ import annotations

import numpy as np

import param_variants as pv
from int_dp_model import CODE, K_ROWS, cell_bases

SLOTS = 52   # thal_pairs_row.hip Row13::kRowSlots: the stored cells a lane's table holds


def rc(s: str) -> str:
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _min_chain(bt: dict, a: str, b: str):
    """(minimum in table units before the initiation | None: no complementary cell, loop shapes of the winning chain).
    Ties go to the first candidate met: the left end term before any predecessor, predecessors and picks in cell order."""
    g, T, void = bt["g"], bt["T"], bt["void"]
    s1 = [CODE[c] for c in a]
    s2 = [CODE[c] for c in reversed(b)]
    k = len(a)
    cells = []   # (im1, jm1, value, po, index of the predecessor cell | None, (l1, l2) of the step from it)
    pick = last = None
    for im1 in range(k):
        for jm1 in range(k):
            if s1[im1] + s2[jm1] != 3:
                continue
            cb = cell_bases(s1, s2, im1, jm1)
            a4 = cb["a"] << 2
            yTS, yMM = int(g[cb["yTS"]]), int(g[cb["yMM"]])
            best, pred, shape = int(g[cb["idxL"]]), None, None
            assert best < void
            for p, (pi, pj, Gp, po, _, _) in enumerate(cells):
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
                if t + y + Gp < best:
                    best, pred, shape = t + y + Gp, p, (l1, l2)
            cells.append((im1, jm1, best, cb["po"], pred, shape))
            end = best + int(g[cb["idxR"]])
            if pick is None or end < pick:
                pick, last = end, len(cells) - 1
    shapes = []
    while last is not None:
        _, _, _, _, last, shape = cells[last]
        if shape is not None and shape != (0, 0):
            shapes.append(shape)
    return pick, shapes[::-1]


def bound_pair(bt: dict, a: str, b: str):
    """The bound of thal ANY's dG for (a, b) in cal/mol; None: no complementary cell (no chain)."""
    pick, _ = _min_chain(bt, a, b)
    return None if pick is None else (pick + bt["init"]) / bt["unit_inv"]


def bound_pair_trace(bt: dict, a: str, b: str):
    """(bound_pair(bt, a, b), the loop shapes (l1, l2) != (0, 0) on the winning chain, 5' to 3' on a)."""
    pick, shapes = _min_chain(bt, a, b)
    return (None if pick is None else (pick + bt["init"]) / bt["unit_inv"]), shapes


# ---- the pools and chemistries the CPU and the GPU suite share --------------------------------------------------------
def mixed_pool(k: int, n_random: int, seed: int):
    """n_random seeded random oligos, the reverse complement of the first, the four homopolymers, GCGC... and ATAT..."""
    rng = np.random.default_rng(seed)
    pool = ["".join(r) for r in rng.choice(list("ACGT"), size=(n_random, k))]
    return pool + [rc(pool[0])] + [x * k for x in "ACGT"] + [("GC" * k)[:k], ("AT" * k)[:k]]


# the corners of what build_bound_tables admits (273.15 K <= temp_k <= 373.15 K, a finite salt term), as keyword
# arguments of Chem.ntthal / pyoracle.ntthal_args alike
EDGE_CHEMS = {
    "t0": {"temp_c": 0.0},
    "t100": {"temp_c": 100.0},
    "mv1_dv0": {"mv": 1.0, "dv": 0.0},
    "dv0_dntp1": {"dv": 0.0, "dntp": 1.0},
    "conc1": {"dna_conc": 1.0},
    "conc1e6": {"dna_conc": 1e6},
    "mv1000_dv100": {"mv": 1000.0, "dv": 100.0},
    "t70_mv5": {"temp_c": 70.0, "mv": 5.0},
}
UNUSABLE_CHEMS = {"t-1": {"temp_c": -1.0}, "t100.5": {"temp_c": 100.5}}


# ---- which pairs the stage bounds: wave_pairs_row<52, true> for a wave whose columns all have one base composition ----
def stored_cells(a: str, b: str) -> int:
    """The complementary cells of (a, b) but those of a's last row, which are nobody's predecessors: the slots the
    pair's table takes (n_cells of wave_pairs_row)."""
    c1 = [a.count(x) for x in "ACGT"]
    c2 = [b.count(x) for x in "ACGT"]
    n_all = sum(c1[x] * c2[3 - x] for x in range(4))
    return n_all - c2[3 - CODE[a[-1]]]


def bounded_in_uniform_wave(a: str, b: str) -> bool:
    """False: the stage hands (a, b) on unbounded (plane -inf) -- more stored cells than slots, or both oligos their own
    reverse complement.  In a wave of one composition nothing else sheds a lane: every active lane has the same cell
    count, so the drag rule finds no second party, and the wave's slot count is that same number."""
    return not (stored_cells(a, b) > SLOTS or (a == rc(a) and b == rc(b)))


# ---- constructed pairs whose best chain is two stems joined by one loop of a chosen shape ------------------------------
STEM_PAIRS = (("GCC", "CGC"), ("CCG", "GGC"), ("GC", "CG"), ("GCCG", "CGG"), ("G", "C"), ("GC", "C"))


def two_stem_family(k: int = 13, stems=STEM_PAIRS):
    """[(a, b)]: a = sA A^l1 sB A..., b = ...A rc(sB) A^l2 rc(sA) for every stem pair and every 0 <= l1, l2 <= 11 but
    (0, 0) that fits in k bases (536 pairs at k = 13).  A-A is never complementary: the filler adds no cells."""
    out = []
    for sA, sB in stems:
        for l1 in range(12):
            for l2 in range(12):
                if (l1, l2) == (0, 0) or len(sA) + len(sB) + max(l1, l2) > k:
                    continue
                out.append(((sA + "A" * l1 + sB).ljust(k, "A"), (rc(sB) + "A" * l2 + rc(sA)).rjust(k, "A")))
    return out


def long_loops_cheap_sections():
    """The stock bundle with the interior and bulge enthalpies of loops.dh lowered by 5000 cal/mol for loop sizes >= 6
    (rows of  size interior bulge hairpin): long loops win the minimum, so their table entries show in the bound."""
    cheap = lambda i, v: v - 5000 if i % 4 in (1, 2) and i // 4 + 1 >= 6 else v
    return pv._mapped(pv.stock_sections(), {"loops.dh": cheap})
