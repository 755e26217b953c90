"""The launch plan of the pair screens (csrc/screen_plan.hpp, read through msspe_host_screen_plan: no GPU) against the
Python model of tests/screen_plan_model.py, launch for launch; the invariants that keep a hand-over list from being
overrun, checked on the plan itself; and plans pinned to what the screens ran before the plan was a value of its own
(the module docstring of test_gpu_odd_pool_geometry.py, tests/golden/headline_65536.json).

The row-group invariant, as it holds of that arithmetic: a launch band that is not the block's last has whole groups
of 24 rows, or the even split gave it at most 24 rows -- the split is above half the largest whole-group launch, so
this needs a launch limit below 48 rows (26 rows of 100 columns under a list of 2,600: bands of 13 and 13)."""
import json

import numpy as np
import pytest

from screen_plan_model import CHUNK_PAIRS, FIRST_STAGES, ROW_GROUP, screen_plan_model

RECTANGULAR = [s for s in FIRST_STAGES if s != "bound_mirror"]
ROW0, ROW1, COL0, COL1, PAIRS, ENTRIES, FLUSH = range(7)


@pytest.fixture(scope="module")
def plan_of():
    from msspe_amd import capi
    return capi.host_screen_plan


def blocks():
    """(row0, row1, col0, ncols, list_cap) of the rectangular and the dense rule: seeded."""
    rng = np.random.default_rng(20240)
    out = []
    for _ in range(1000):       # lists as set_option can size them
        rows, cols = (int(x) for x in rng.integers(1, 5001, 2))
        out.append((0, rows, 0, cols, int(rng.integers(1 << 20, (1 << 22) + 1))))
    for _ in range(150):        # blocks that start inside the pool
        r0, c0 = (int(x) for x in rng.integers(1, 70000, 2))
        rows, cols = (int(x) for x in rng.integers(1, 5001, 2))
        out.append((r0, r0 + rows, c0, cols, int(rng.integers(1 << 20, (1 << 22) + 1))))
    for _ in range(400):        # capacities no option reaches: the budget at its tightest
        rows, cols = (int(x) for x in rng.integers(1, 301, 2))
        r0, c0 = (int(x) for x in rng.integers(0, 50, 2))
        out.append((r0, r0 + rows, c0, cols, int(rng.integers(2, 5001))))
    for cap in (2, 3, 24, 25, 47, 48, 49, 2600, 1 << 20):
        out += [(0, 1, 0, 1, cap), (5, 6, 9, 300, cap), (7, 307, 3, 1, cap), (0, 27, 0, 100, cap)]
    out += [(0, 3, 0, 3_000_000, 1 << 20), (11, 13, 5, (1 << 21) + 1, 1 << 21)]   # a row longer than a list: column chunks
    return out


def squares():
    """(n, list_cap) of the mirrored rule: n <= min(2^29, list_cap / 2)."""
    rng = np.random.default_rng(20241)
    out = [(int(rng.integers(1, 5001)), int(rng.integers(1 << 20, (1 << 22) + 1))) for _ in range(1000)]
    for _ in range(400):
        cap = int(rng.integers(2, 5001))
        out.append((int(rng.integers(1, min(300, cap // 2) + 1)), cap))
    out += [(1, 2), (1, 3), (2, 4), (24, 48), (25, 50), (300, 600), (1, 1 << 20), (1 << 19, 1 << 20)]
    return out


def check_budget(plan, list_cap):
    """Between two flushes the launches cannot append more than a list holds; no launch is over 2^29 pairs."""
    assert len(plan) and not plan[0, FLUSH]
    assert (plan[:, PAIRS] > 0).all() and (plan[:, PAIRS] <= CHUNK_PAIRS).all()
    run = 0
    for entries, flush in plan[:, [ENTRIES, FLUSH]]:
        run = entries if flush else run + entries
        assert run <= list_cap


def check_rectangular(plan, stage, row0, row1, col0, ncols, list_cap):
    """The launches tile the block exactly once, band by band, in whole row groups."""
    base = col0 if stage in ("dense", "wave") else 0
    bands = np.flatnonzero(plan[:, COL0] == base)
    assert bands[0] == 0 and plan[0, ROW0] == row0 and plan[-1, ROW1] == row1 and plan[-1, COL1] == base + ncols
    for i, at in enumerate(bands):
        end = bands[i + 1] if i + 1 < len(bands) else len(plan)
        band = plan[at:end]
        assert (band[:, ROW0] == band[0, ROW0]).all() and (band[:, ROW1] == band[0, ROW1]).all()
        assert (band[1:, COL0] == band[:-1, COL1]).all() and band[-1, COL1] == base + ncols      # columns: contiguous
        if end < len(plan):
            assert plan[end, ROW0] == band[0, ROW1]                                               # rows: contiguous
    rows, cols = plan[:, ROW1] - plan[:, ROW0], plan[:, COL1] - plan[:, COL0]
    assert (rows > 0).all() and (cols > 0).all() and (plan[:, PAIRS] == rows * cols).all()
    assert (plan[:, ENTRIES] == (0 if stage == "dense" else plan[:, PAIRS])).all()
    max_rows = max(1, min(CHUNK_PAIRS, list_cap) // ncols)
    inner = rows[plan[:, ROW1] < row1]
    assert ((inner % ROW_GROUP == 0) | ((inner <= ROW_GROUP) & (max_rows < 2 * ROW_GROUP))).all()


def check_mirrored(plan, n, list_cap):
    assert plan[0, ROW0] == 0 and plan[-1, ROW1] == n and (plan[1:, ROW0] == plan[:-1, ROW1]).all()
    assert (plan[:, COL0] == 0).all() and (plan[:, COL1] == n).all()
    p0, p1 = plan[:, ROW0], plan[:, ROW1]
    assert (plan[:, PAIRS] == (p1 - p0) * n - (p1 * (p1 - 1) - p0 * (p0 - 1)) // 2).all()      # sum of n - p
    assert plan[:, PAIRS].sum() == n * (n + 1) // 2
    assert (plan[:, PAIRS] <= min(CHUNK_PAIRS, list_cap // 2)).all()
    assert (plan[:, ENTRIES] == 2 * plan[:, PAIRS]).all()


def test_rectangular_and_dense_plans_equal_the_model(plan_of):
    for row0, row1, col0, ncols, cap in blocks():
        for stage in RECTANGULAR:
            plan = plan_of(stage, row0, row1, col0, ncols, cap)
            np.testing.assert_array_equal(plan, screen_plan_model(stage, row0, row1, col0, ncols, cap),
                                          err_msg=f"{stage} rows [{row0}, {row1}) cols {col0} + {ncols} cap {cap}")
            check_rectangular(plan, stage, row0, row1, col0, ncols, cap)
            check_budget(plan, cap)


def test_mirrored_plans_equal_the_model(plan_of):
    for n, cap in squares():
        for at in (0, 77):
            plan = plan_of("bound_mirror", at, at + n, at, n, cap)
            np.testing.assert_array_equal(plan, screen_plan_model("bound_mirror", at, at + n, at, n, cap),
                                          err_msg=f"n {n} cap {cap}")
            check_mirrored(plan, n, cap)
            check_budget(plan, cap)


def test_what_the_planner_refuses(plan_of):
    import msspe_amd
    for args in (("row", 0, 0, 0, 5, 1 << 20), ("row", 0, 5, 0, 0, 1 << 20), ("row", 0, 5, 0, 5, 0), ("row", -1, 5, 0, 5, 1 << 20),
                 ("bound_mirror", 0, 5, 1, 5, 1 << 20), ("bound_mirror", 0, 5, 0, 6, 1 << 20), ("bound_mirror", 0, 5, 0, 5, 9)):
        with pytest.raises(msspe_amd.MsspeError):
            plan_of(*args)


def rows_and_flushes(plan):
    return (plan[:, ROW1] - plan[:, ROW0]).tolist(), plan[:, FLUSH].tolist()


def test_pinned_plans(plan_of, golden_dir):
    # 1,500 oligos under a list of 2^20 (test_gpu_pair_mirror.py test_several_launches_and_flushes)
    assert rows_and_flushes(plan_of("bound", 0, 1500, 0, 1500, 1 << 20)) == ([504, 504, 492], [0, 1, 1])
    plan = plan_of("bound_mirror", 0, 1500, 0, 1500, 1 << 20)
    assert plan[:, [ROW0, ROW1, FLUSH]].tolist() == [[0, 288, 0], [288, 672, 1], [672, 1500, 1]]
    # the headline screen: nine launches in five flush groups, the fixture's boundaries
    plan = plan_of("row", 0, 65536, 0, 65536, 1 << 30)
    assert rows_and_flushes(plan) == ([7296] * 8 + [7168], [0, 0, 1, 0, 1, 0, 1, 0, 1])
    fixture = json.loads((golden_dir / "headline_65536.json").read_text())
    assert plan[1:, ROW0].tolist() == fixture["launch_boundaries"] == list(range(7296, 65536, 7296))
    plan = plan_of("bound_mirror", 0, 65536, 0, 65536, 1 << 30)
    assert plan[:, [ROW0, ROW1]].tolist() == [[0, 6936], [6936, 14808], [14808, 24144], [24144, 36312], [36312, 65536]]
    assert plan[:, FLUSH].tolist() == [0, 1, 1, 1, 1]
    # rows of test_gpu_odd_pool_geometry.py's table (list_cap_log2 = 29), and a small square
    assert rows_and_flushes(plan_of("row", 0, 65503, 0, 65503, 1 << 29))[0] == [7296] * 8 + [7135]
    assert rows_and_flushes(plan_of("row", 0, 35839, 0, 35839, 1 << 29))[0] == [11952] * 2 + [11935]
    assert rows_and_flushes(plan_of("row", 0, 1040, 0, 1040, 1 << 20)) == ([528, 512], [0, 1])
    # a block inside the pool: the wave and dense kernels' columns are the pool's, the others' sorted positions
    for stage in RECTANGULAR:
        plan = plan_of(stage, 100, 200, 40, 60, 1 << 20)
        assert plan.tolist() == [[100, 200, 40 if stage in ("dense", "wave") else 0, (100 if stage in ("dense", "wave") else 60),
                                  6000, 0 if stage == "dense" else 6000, 0]]
