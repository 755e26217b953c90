"""The ring of three row banks of the windowed bound first stage on the device (csrc/thal_pairs_row.hip
k_pairs_bound_window, the generated scans row_bound_ring_pinned.inc and row_bound_ring_pair_pinned.inc).

Row i of a table lives in bank i % 3 and a cell of row i scans rows i-2 and i-1 at their widths, so what can go wrong is
tied to the widths that follow each other in one bank and to the rotation: a bank taken by a narrower or a wider row than
the one three rows up, empty rows inside the window, every tail size behind a full chunk in every bank, a 13-wide row,
empty words inside a row's width (two compositions in one wave) and tables of fewer than three rows.

Every case is one row oligo against 65 columns of one composition -- a full and a partial wave -- or a small mixed
square, on the stock tables and on the bundle whose long loops are cheap: plane == tests/pair_bound_window_model.py on
float64, and the +-inf pattern is the packed plane's (check_planes)."""
import numpy as np
import pytest

from pair_bound_model import mixed_pool
from test_gpu_pair_bound_window import (check_planes, cheap, device_planes, eng, m, model_values, pk, row_starts,      # noqa: F401
                                        uniform_columns)

pytestmark = pytest.mark.gpu

N_COLS = 65


def widths_of(row, col):
    """The stored rows' widths (the last row is stored nowhere)."""
    starts, total = row_starts(row, col)
    return [b - a for a, b in zip(starts, starts[1:] + [total])]


def wide_over_narrow(w):
    assert w == [1, 3, 4, 5] * 3 and sum(w) == 39
    # every bank is taken again by a row narrower and by a row wider than the one three rows up
    for b in range(3):
        d = [w[i] - w[i - 3] for i in range(3, 12) if i % 3 == b]
        assert min(d) < 0 < max(d), (b, d)


def narrow_over_wide(w):
    assert w == [5, 4, 3, 1] * 3
    for b in range(3):
        d = [w[i] - w[i - 3] for i in range(3, 12) if i % 3 == b]
        assert min(d) < 0 < max(d), (b, d)


def windows(w):
    """(far width, near width, rows above the window hold cells) of every row i >= 2 that has cells or is the last."""
    full = w + [1]      # the last row's cells scan too
    return [(full[i - 2], full[i - 1], sum(full[:i - 2]) > 0) for i in range(2, 13) if full[i]]


def near_row_empty(w):
    win = windows(w)
    assert any(f > 0 and n == 0 and above for f, n, above in win)
    assert not any(f == 0 and above for f, n, above in win)


def far_row_empty(w):
    win = windows(w)
    assert any(f == 0 and n > 0 and above for f, n, above in win)


def both_rows_empty(w):
    assert any(f == 0 and n == 0 and above for f, n, above in windows(w))


def tail_in_every_bank(size):
    def check(w):
        # a row of one full chunk and `size` more slots in each of the three banks, each scanned as near and as far row
        assert {i % 3 for i, x in enumerate(w) if x == 4 + size} == {0, 1, 2}
        assert all(w[i + 1] > 0 and w[i + 2] > 0 for i, x in enumerate(w[:10]) if x == 4 + size)
        assert sum(w) <= 52
    return check


def thirteen_wide(w):
    assert w == [0] * 8 + [13] * 4      # banks 2, 0, 1, 2; rows 10, 11 and the last row scan them


#         name                 row oligo        columns' (A, C, G, T)   the widths it is about
CASES = [("wide_over_narrow", "ACGTACGTACGTA", (5, 4, 3, 1), wide_over_narrow),
         ("narrow_over_wide", "TGCATGCATGCAT", (5, 4, 3, 1), narrow_over_wide),
         ("near_row_empty", "ACGACGACGACTG", (0, 4, 4, 5), near_row_empty),
         ("far_row_empty", "ACGACTGACGACG", (0, 4, 4, 5), far_row_empty),
         ("both_rows_empty", "ACGATTGACGACG", (0, 4, 4, 5), both_rows_empty),
         ("tail_1", "ACCCACCCACCCC", (0, 7, 1, 5), tail_in_every_bank(1)),
         ("tail_2", "ACCCACCCACCCC", (0, 6, 1, 6), tail_in_every_bank(2)),
         ("tail_3", "ACCCACCCACCCC", (0, 5, 1, 7), tail_in_every_bank(3)),
         ("tail_4", "ACCCACCCACCCC", (0, 4, 1, 8), tail_in_every_bank(4)),
         ("thirteen_wide", "CCCCCCCCAAAAA", (0, 0, 0, 13), thirteen_wide)]


@pytest.mark.parametrize("name,row,comp,check_widths", CASES, ids=[c[0] for c in CASES])
def test_widths_that_follow_each_other_in_a_bank(m, pk, cheap, eng, name, row, comp, check_widths):
    cols = uniform_columns(comp, 1 if comp.count(0) == 3 else N_COLS, seed=6400 + len(name))
    cols = cols * (N_COLS if len(cols) == 1 else 1)
    for col in cols[:3]:
        check_widths(widths_of(row, col))
    for what, (e, tables) in (("stock", (eng, pk)), ("long_loops_cheap", cheap)):
        b, packed = device_planes(e, m, [row] + cols, (0, 1), (1, 1 + N_COLS))
        n_fin, n_low = check_planes(b, packed, model_values(tables, [row], cols), tables, f"{what} {name}")
        print(f"{what} {name}: {n_fin} of {N_COLS} pairs with a value, {n_low} below the packed instance's")
        assert n_fin > 0


@pytest.mark.parametrize("k", [3, 4, 5, 13])
def test_two_compositions_in_one_wave(eng, m, pk, cheap, k):
    """Mixed squares: the lanes of a wave differ in composition, so a row's width is the widest lane's and the narrower
    lanes' words inside it are empty; at k = 3, 4, 5 the rotation runs where fewer than three rows above a cell exist."""
    pool = mixed_pool(k, 150 if k == 13 else 64, seed=6500 + k)
    n = len(pool)
    assert n <= 200
    for name, (e, tables) in (("stock", (eng, pk)), ("long_loops_cheap", cheap)):
        b, packed = device_planes(e, m, pool, (0, n), (0, n))
        n_fin, n_low = check_planes(b, packed, model_values(tables, pool, pool), tables, f"{name} k={k}")
        print(f"{name} k={k}: {n_fin} of {n * n} pairs with a value, {n_low} below the packed instance's")
        assert n_fin >= 100
        if k <= tables["window"]["F"] + 1:
            np.testing.assert_array_equal(b, packed)
