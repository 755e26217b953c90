"""Which pairs the bound LIST stage bounds (csrc/thal_pairs_bound_list.hip k_pairs_bound_list), and the pools its tests
share.  Test infrastructure beside pair_bound_model.py, whose bound_pair is the integer the stage must report: the list
stage runs the same recurrence on the same tables, so there is no second value model -- only the rule that says where a
value must stand.

The bound first stage (wave_pairs_row<52, true>) puts a lane on list U when it leaves its wave without a bound of its
own and the 64-slot list table holds it: 53..63 stored cells, or dragged / shed from a wave of mixed compositions with
at most 52.  A pair of two self-complementary oligos, and one with more than 63 stored cells, goes to list 0 as it is.
In the plane of msspe_cross_dimer_bound_list_dev every pair therefore has a value, whatever wave it sat in, except
those two kinds (-inf) and pairs without a complementary cell (+inf)."""
from __future__ import annotations

import numpy as np

from pair_bound_model import SLOTS, mixed_pool, rc, stored_cells

LIST_SLOTS = 63     # int_core.hpp kListStoredMax: stored cells the 64-slot list table holds (one slot stays free)
BATCH = 512         # thal_pairs_bound_list.hip kBLThreads: entries per pass; a batch is 512 x depth, depth <= 7


def n_cells(a: str, b: str) -> int:
    """Every complementary cell of (a, b), the last row's included."""
    return sum(a.count(x) * b.count(y) for x, y in zip("ACGT", "TGCA"))


def pair_class(a: str, b: str) -> str:
    """'sym': both oligos their own reverse complement (-inf); 'none': no complementary cell (+inf); 'over': more than 63
    stored cells (-inf); 'u': 53..63 stored cells -- list U whatever the wave; 'row': at most 52 -- the first stage bounds
    it unless its wave drags or sheds it, and then list U does."""
    if a == rc(a) and b == rc(b):
        return "sym"
    if n_cells(a, b) == 0:
        return "none"
    s = stored_cells(a, b)
    return "over" if s > LIST_SLOTS else ("u" if s > SLOTS else "row")


def class_plane(rows, cols):
    return np.array([[pair_class(a, b) for b in cols] for a in rows])


def skewed_pool(k: int, n_random: int, seed: int, n_rich: int = 8):
    """n_random seeded oligos drawn with P(A) = P(T) = 0.35, P(C) = P(G) = 0.15 (many pairs with 53..63 stored cells at
    13 bases), mixed_pool's extras (the reverse complement of oligo 0, the homopolymers, GCGC..., ATAT...), and n_rich
    A-rich and n_rich T-rich oligos (the other base at each position with probability 0.15): at 9 and 11 bases only
    such pairs reach 53 cells, and an A/T-rich oligo against itself is a diagonal pair of list U."""
    rng = np.random.default_rng(seed)
    pool = ["".join(r) for r in rng.choice(list("ACGT"), size=(n_random, k), p=[0.35, 0.15, 0.15, 0.35])]
    extras = mixed_pool(k, 1, seed)[1:]
    extras[0] = rc(pool[0])
    rich = ["".join(r) for r in rng.choice(list("AT"), size=(n_rich, k), p=[0.85, 0.15])]
    rich += ["".join(r) for r in rng.choice(list("AT"), size=(n_rich, k), p=[0.15, 0.85])]
    return pool + extras + rich
