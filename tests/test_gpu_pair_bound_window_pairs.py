"""The windowed bound first stage scans two cells of a row in one pass (csrc/thal_pairs_row.hip run_pair_window,
the generated scan row_bound_ring_pair_pinned.inc): the diagnostic plane msspe_cross_dimer_bound_window_dev against
tests/pair_bound_window_model.py, == on float64, on the stock tables and on the bundle whose long loops are cheap.

What the pairing can get wrong is decided by the widths of a table's rows (a row of width w is w // 2 two-cell scans
and, for odd w, one single scan behind them) and by where a pair's two slots fall, so one row oligo runs against 65
columns of one base composition -- a full and a partial wave -- chosen for the widths; the widths each case is named
for are asserted from row_starts.  Two compositions in one wave put lanes narrower than the widest into a pair: cell B
alone, or A and B, are off there (asserted from the widths as well); mixed pools do the same at random."""
import numpy as np
import pytest

from pair_bound_model import bounded_in_uniform_wave, mixed_pool
from test_gpu_pair_bound_window import (check_planes, cheap, device_planes, eng, m, model_values, pk, row_starts,  # noqa: F401
                                        uniform_columns)

pytestmark = pytest.mark.gpu

NS = 52
N_COLS = 65

#          name          row oligo        columns' (A, C, G, T)
WIDTHS = [("all_one", "AAAAAAAAAAAAA", (4, 4, 4, 1)),          # no pair anywhere
          ("all_two", "AAAAAAAAAAAAA", (4, 4, 3, 2)),          # pairs only
          ("all_three", "AAAAAAAAAAAAA", (4, 3, 3, 3)),        # a pair and an odd cell in every row
          ("four_five", "ACACACACACGTA", (2, 2, 4, 5)),        # 5, 4, 5, 4, ...: two pairs / two pairs and an odd cell
          ("full_even", "AAAAAAAACCTTA", (2, 2, 4, 5)),        # 52 stored cells, last stored row 2 wide: a pair ends at slot 51
          ("full_odd", "AAAAAAAACCTGA", (1, 3, 4, 5)),         # 52 stored cells, last stored row 3 wide: the odd cell is slot 51
          ("homopolymer", "ACGTTGCAAGTCA", (0, 0, 0, 13)),     # only the A rows hold cells (13 wide), the others are empty
          ("homopolymer_g", "ACTAGCATTACGA", (0, 0, 13, 0))]


def stored_widths(row, col):
    starts, total = row_starts(row, col)
    return [b - a for a, b in zip(starts, starts[1:] + [total])], total


@pytest.mark.parametrize("name,row,comp", WIDTHS, ids=[w[0] for w in WIDTHS])
def test_row_widths(m, pk, cheap, eng, name, row, comp):
    homo = comp.count(0) == 3
    cols = uniform_columns(comp, 1 if homo else N_COLS, seed=6400)
    cols = cols * (N_COLS if homo else 1)
    widths, total = stored_widths(row, cols[0])
    assert len(widths) == 12 and total <= NS
    if name in ("all_one", "all_two", "all_three"):
        assert set(widths) == {{"all_one": 1, "all_two": 2, "all_three": 3}[name]}
    if name == "four_five":
        assert widths[:10] == [5, 4] * 5 and set(widths) >= {4, 5}
    if name == "full_even":
        assert total == NS and widths[-1] == 2
    if name == "full_odd":
        assert total == NS and widths[-1] == 3 and 1 in widths
    if homo:
        assert set(widths) == {0, 13} and 0 < total <= NS
    ok = np.array([[bounded_in_uniform_wave(row, y) for y in cols]])
    assert ok.all()
    for what, (e, tables) in (("stock", (eng, pk)), ("long_loops_cheap", cheap)):
        b, packed = device_planes(e, m, [row] + cols, (0, 1), (1, 1 + N_COLS))
        np.testing.assert_array_equal(b != -np.inf, ok, err_msg=f"{name}: the pairs handed on unbounded are not the sizing rule's")
        n_fin, _ = check_planes(b, packed, model_values(tables, [row], cols), tables, f"{what} {name}")
        assert n_fin > 0


def test_two_compositions_in_one_wave(m, pk, cheap, eng):
    """Lanes narrower than their wave's widest inside a pair.  33 columns of one composition and 32 of another: whatever
    order the screen puts its columns in, the first wave's 64 lanes hold both.  The two have the same number of stored
    cells, so the sizing rule sheds neither party, and the padded table fits.  In the A rows one party has four cells
    and the other one, in the C rows the other way round: in the pair of cells 0 and 1 the narrow lanes have B alone
    off, in the pair of cells 2 and 3 they have A and B off."""
    row = "AAAAAACCCCCCA"
    t_rich, g_rich = uniform_columns((4, 4, 1, 4), 33, seed=6600), uniform_columns((4, 4, 4, 1), 32, seed=6601)
    cols = [c for pair in zip(t_rich, g_rich) for c in pair] + t_rich[32:]
    assert len(cols) == N_COLS and max(len(t_rich), len(g_rich)) < 64      # any 64 of the 65 hold both compositions
    (wt, tt), (wg, tg) = stored_widths(row, t_rich[0]), stored_widths(row, g_rich[0])
    assert tt == tg and sum(max(a, b) for a, b in zip(wt, wg)) <= NS        # nobody is shed, and the wave's table fits
    for i, x in enumerate(row[:-1]):
        w, n = (wt[i], wg[i]) if x == "A" else (wg[i], wt[i])
        assert (w, n) == (4, 1)      # cells (0, 1): the narrow lanes have A, not B; cells (2, 3): they have neither
    for what, (e, tables) in (("stock", (eng, pk)), ("long_loops_cheap", cheap)):
        b, packed = device_planes(e, m, [row] + cols, (0, 1), (1, 1 + N_COLS))
        n_fin, _ = check_planes(b, packed, model_values(tables, [row], cols), tables, f"{what} two compositions")
        assert n_fin == N_COLS       # every lane stayed in the wave (none handed on unbounded)


@pytest.mark.parametrize("k", range(2, 14))
def test_mixed_pools(eng, m, pk, cheap, k):
    """207 mixed 13-mers and 79 oligos at every shorter length.  No composition of the 13-mer pool has 64 members, so
    every full wave holds several, whatever the column order: lanes of differing widths in its rows."""
    pool = mixed_pool(k, 200 if k == 13 else 72, seed=6500 + k)
    n = len(pool)
    if k == 13:
        comps = [tuple(p.count(x) for x in "ACGT") for p in pool]
        assert n > 3 * 64 and max(comps.count(c) for c in set(comps)) < 64
    for name, (e, tables) in (("stock", (eng, pk)), ("long_loops_cheap", cheap)):
        b, packed = device_planes(e, m, pool, (0, n), (0, n))
        n_fin, _ = check_planes(b, packed, model_values(tables, pool, pool), tables, f"{name} k={k}")
        assert n_fin >= 100
