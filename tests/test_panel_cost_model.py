"""The model of the thinning and selection by gain per cost (tests/panel_cost_model.py): with equal costs it equals the
weighted and unweighted models on the grid cases and on 200 random matrices; built cases where the costs change the kept
set, where a primer below min_gain must neither win nor stop the loop, the two tie levels, and the case only an exact
comparison decides; and the host layer's sequential twins (thin_panel_cost / select_panel_cost through their hooks)
against it -- every comparison on integers, exactly.  No GPU needed."""
import ctypes as C
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import panel_cost_model as cm
import panel_select_model as sm
import panel_thin_model as tm
import panel_weighted_model as wm
from test_panel_select_model import random_graph
from test_panel_thin_model import GRID, grid_case, random_bitmap
from test_panel_weighted_model import draw_weights

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
THIN = ("keep", "order", "gains", "covered", "covered_all", "covered_kept", "rounds")


@pytest.fixture(scope="module")
def host():
    import msspe_amd
    msspe_amd.load_library()
    return C.CDLL(str(LIB))


@pytest.fixture(scope="module")
def grid_incidence():
    out = {}
    for k, M, _ in GRID:
        g, fwd, rev = grid_case(k, M)
        out[k, M] = tm.incidence(g, 400, 170, 50, k, fwd, rev, M, 3)
    return out


def loses_nothing(res, weighted=False):
    """Guarantee 2: the thinning at min_gain 1 keeps every segment the whole set covers; with weights every unit of
    weight (a segment of weight 0 earns no pick, so it may go)."""
    assert res["weight_kept"] == res["weight_all"]
    assert weighted or res["covered_kept"] == res["covered_all"]


def equal_costs_equal_the_siblings(I, B, w, T, min_gain, forced, drop=False, c=1):
    n = I.shape[0]
    costs = [c] * n
    plain = dict(zip(THIN, tm.greedy(I, min_gain, forced)))
    got = cm.greedy_cost(I, costs, None, min_gain, forced)
    for key in THIN:
        np.testing.assert_array_equal(got[key], plain[key], key)
    assert (got["weight_all"], got["weight_kept"]) == (plain["covered_all"], plain["covered_kept"])
    assert got["cost_all"] == c * n and got["cost_kept"] == c * int(got["keep"].sum())
    if min_gain == 1:
        loses_nothing(got)
    want = wm.greedy_weighted(I, w, min_gain, forced)
    got = cm.greedy_cost(I, costs, w, min_gain, forced)
    for key, v in want.items():
        np.testing.assert_array_equal(got[key], v, key)
    if min_gain == 1:
        loses_nothing(got, True)
    want = sm.select(I, B, T, min_gain, forced, drop)
    got = cm.select_cost(I, B, costs, None, T, min_gain, forced, drop)
    for key, v in want.items():
        np.testing.assert_array_equal(got[key], v, key)
    want = wm.select_weighted(I, B, w, T, min_gain, forced, drop)
    got = cm.select_cost(I, B, costs, w, T, min_gain, forced, drop)
    for key, v in want.items():
        np.testing.assert_array_equal(got[key], v, key)
    assert got["cost_kept"] == c * int(got["keep"].sum())
    sm.check_independent(got, B, forced, drop)


@pytest.mark.parametrize("k,M,picks", GRID)
def test_equal_costs_on_the_grid_cases(grid_incidence, k, M, picks):
    I = grid_incidence[k, M]
    n = I.shape[0]
    rng = np.random.default_rng(k + M)
    w = draw_weights(rng, I.shape[1])
    for density, T, min_gain, c in ((0, 1, 1, 1), (0.05, 3, 2, 7), (1, 1, 1, 7), (0.05, 1, 1, 1)):
        equal_costs_equal_the_siblings(I, random_graph(n, density), w, T, min_gain, None, c=c)
    equal_costs_equal_the_siblings(I, random_graph(n, 0.05), w, 2, 1, rng.random(n) < 0.05, drop=True, c=7)
    assert len(cm.greedy_cost(I, [7] * n)["order"]) == picks


def test_equal_costs_on_200_random_matrices():
    for seed in range(200):
        rng = np.random.default_rng(seed)
        n, n_seg = int(rng.integers(1, 60)), int(rng.integers(1, 300))
        I = random_bitmap(rng, n, n_seg)
        forced = rng.random(n) < 0.1 if seed % 3 == 0 else None
        equal_costs_equal_the_siblings(I, random_graph(n, float(rng.choice([0, 0.05, 0.3])), seed=seed),
                                       draw_weights(rng, n_seg), int(rng.choice([1, 2, 64])), int(rng.choice([1, 2])),
                                       forced, bool(seed % 2), c=(1, 7)[seed % 2])


# ---- the built cases (shared with the GPU tests) ------------------------------------------------------------------
def case_cheap_primers():
    """One primer covers 6 segments at cost 7, three cover 2 each at cost 2."""
    I = np.zeros((4, 6), dtype=bool)
    I[0] = True
    I[1, 0:2] = I[2, 2:4] = I[3, 4:6] = True
    return I, [7, 2, 2, 2]


def case_below_min_gain():
    """p0 has the best ratio (1 / 1) but a gain below min_gain 2; p1 (4 / 8) and p2 (2 / 5) qualify."""
    I = np.zeros((3, 7), dtype=bool)
    I[0, 0] = True
    I[1, 1:5] = True
    I[2, 5:7] = True
    return I, [1, 8, 5], 2


def test_the_costs_change_the_kept_set():
    I, costs = case_cheap_primers()
    assert tm.greedy(I)[1].tolist() == [0]              # the plain rule keeps the one
    res = cm.greedy_cost(I, costs)
    assert res["order"].tolist() == [1, 2, 3] and res["gains"].tolist() == [2, 2, 2]
    assert (res["cost_kept"], res["cost_all"]) == (6, 13) and res["rounds"] == 4
    loses_nothing(res)
    sel = cm.select_cost(I, np.zeros((4, 4), dtype=bool), costs)
    assert sel["order"].tolist() == [1, 2, 3] and sel["cost_kept"] == 6


def test_a_gain_below_min_gain_is_no_candidate():
    I, costs, min_gain = case_below_min_gain()
    res = cm.greedy_cost(I, costs, None, min_gain)
    assert res["order"].tolist() == [1, 2] and res["gains"].tolist() == [4, 2]   # never p0, and the loop went on
    assert res["rounds"] == 3 and res["keep"].tolist() == [0, 1, 1]
    assert cm.greedy_cost(I, costs, None, 1)["order"].tolist() == [0, 1, 2]
    sel = cm.select_cost(I, np.zeros((3, 3), dtype=bool), costs, None, 1, min_gain)
    assert sel["order"].tolist() == [1, 2]


def test_ties():
    I = np.zeros((2, 6), dtype=bool)
    I[0, :2] = True                                     # 2 / 1
    I[1, 2:] = True                                     # 4 / 2: equal products, the greater gain wins
    assert cm.greedy_cost(I, [1, 2])["order"].tolist() == [1, 0]
    I = np.zeros((3, 6), dtype=bool)
    I[0, :2] = I[1, 2:4] = I[2, 4:] = True              # all equal: the lowest index
    assert cm.greedy_cost(I, [3, 3, 3])["order"].tolist() == [0, 1, 2]
    assert cm.select_cost(I, np.zeros((3, 3), dtype=bool), [3, 3, 3])["order"].tolist() == [0, 1, 2]


def test_only_the_exact_comparison_decides():
    I, w, costs = cm.EXACT_I, cm.EXACT_W, cm.EXACT_COSTS
    g0, g1 = w[0] + w[1], w[1]
    assert g0 * costs[1] == 18446744056529682435 and g1 * costs[0] == 18446744056529682436
    assert Fraction(g1, costs[1]) > Fraction(g0, costs[0])
    assert np.float64(g0) / np.float64(costs[0]) == np.float64(g1) / np.float64(costs[1])
    assert np.float32(g0) / np.float32(costs[0]) == np.float32(g1) / np.float32(costs[1])
    res = cm.greedy_cost(I, costs, w)
    assert res["order"].tolist() == [1, 0] and res["gains"].tolist() == [2 ** 32 - 2, 1]
    assert res["weight_kept"] == res["weight_all"] == 2 ** 32 - 1
    assert res["cost_kept"] == res["cost_all"] == 2 ** 33 - 5
    # a comparison by division ties, the tie goes to the greater gain, and p0 alone covers everything
    assert wm.greedy_weighted(I, w)["order"].tolist() == [0]


# ---- the host twins -----------------------------------------------------------------------------------------------
def host_thin(host, I, costs, w=None, min_gain=1, forced=None):
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    rows = tm.pack_rows(I)
    weights = None if w is None else np.ascontiguousarray(w, dtype=np.uint32)
    cost = np.ascontiguousarray(costs, dtype=np.uint32)
    order = np.full(max(n, 1), -1, dtype=np.int32)
    gains = np.zeros(max(n, 1), dtype=np.uint32)
    keep = np.full(max(n, 1), 9, dtype=np.uint8)
    sums = np.zeros(6, dtype=np.uint64)
    f = None if forced is None else np.ascontiguousarray(np.asarray(forced) != 0, dtype=np.uint8)
    host.odm_thin_panel_cost.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_longlong] + [C.c_void_p] * 5
    k = host.odm_thin_panel_cost(rows.ctypes.data, n, rows.shape[1], None if weights is None else weights.ctypes.data,
                                 n_seg, cost.ctypes.data, min_gain, f.ctypes.data if f is not None else None,
                                 order.ctypes.data, gains.ctypes.data, keep.ctypes.data, sums.ctypes.data)
    return {"order": order[:k], "gains": gains[:k], "keep": keep[:n], "covered_all": int(sums[0]),
            "covered_kept": int(sums[1]), "weight_all": int(sums[2]), "weight_kept": int(sums[3]),
            "cost_all": int(sums[4]), "cost_kept": int(sums[5])}


def host_select(host, I, B, costs, w=None, T=1, min_gain=1, forced=None, drop=False):
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    rows, bits = tm.pack_rows(I), sm.pack_bitmap(B)
    weights = None if w is None else np.ascontiguousarray(w, dtype=np.uint32)
    cost = np.ascontiguousarray(costs, dtype=np.uint32)
    order = np.full(max(n, 1), -1, dtype=np.int32)
    gains = np.zeros(max(n, 1), dtype=np.uint32)
    keep = np.full(max(n, 1), 9, dtype=np.uint8)
    tube = np.full(max(n, 1), -7, dtype=np.int32)
    barred = np.full(max(n, 1), 9, dtype=np.uint8)
    sums = np.zeros(8, dtype=np.uint64)
    f = None if forced is None else np.ascontiguousarray(np.asarray(forced) != 0, dtype=np.uint8)
    host.odm_select_panel_cost.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_int, C.c_longlong, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    k = host.odm_select_panel_cost(rows.ctypes.data, n, rows.shape[1], bits.ctypes.data,
                                   None if weights is None else weights.ctypes.data, n_seg, cost.ctypes.data, T,
                                   min_gain, f.ctypes.data if f is not None else None, 1 if drop else 0,
                                   order.ctypes.data, gains.ctypes.data, keep.ctypes.data, tube.ctypes.data,
                                   barred.ctypes.data, sums.ctypes.data)
    return {"order": order[:k], "gains": gains[:k], "keep": keep[:n], "tube": tube[:n], "barred": barred[:n],
            "covered_all": int(sums[0]), "covered_kept": int(sums[1]), "tubes_used": int(sums[2]),
            "rounds": int(sums[3]), "weight_all": int(sums[4]), "weight_kept": int(sums[5]),
            "cost_all": int(sums[6]), "cost_kept": int(sums[7])}


def draw_costs(rng, n):
    """1, small, a few large."""
    c = rng.choice([1, 1, 2, 3, 5, 9], size=n).astype(np.int64)
    big = rng.random(n) < 0.05
    c[big] = rng.integers(1000, 2 ** 32 - 1, size=int(big.sum()))
    return c


def same(got, want):
    for key, v in got.items():
        ref = np.where(want[key] == sm.TUBE_NONE, -1, want[key].astype(np.int32)) if key == "tube" else want[key]
        np.testing.assert_array_equal(v, ref, key)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("n_seg", [1, 53, 54, 160])
def test_the_host_twins_equal_the_model(host, n, n_seg):
    rng = np.random.default_rng(1000 * n + n_seg)
    I = random_bitmap(rng, n, n_seg)
    costs = draw_costs(rng, n)
    for w in (None, draw_weights(rng, n_seg)):
        for min_gain, forced in ((1, None), (2, rng.random(n) < 0.1), (500, None)):
            want = cm.greedy_cost(I, costs, w, min_gain, forced)
            same(host_thin(host, I, costs, w, min_gain, forced), want)
            if min_gain == 1:
                loses_nothing(want, w is not None)
            for T, drop in ((1, False), (2, True), (8, False)):
                B = random_graph(n, 0.05, seed=n + n_seg + T)
                want = cm.select_cost(I, B, costs, w, T, min_gain, forced, drop)
                same(host_select(host, I, B, costs, w, T, min_gain, forced, drop), want)
                sm.check_independent(want, B, forced, drop)
    ones = [1] * n                                      # the twins at cost 1 are the weighted hooks' answers
    w = draw_weights(rng, n_seg)
    want = wm.greedy_weighted(I, w)
    got = host_thin(host, I, ones, w)
    for key in ("order", "gains", "keep", "weight_all", "weight_kept"):
        np.testing.assert_array_equal(got[key], want[key], key)


def test_the_built_cases_on_the_host(host):
    I, costs = case_cheap_primers()
    assert host_thin(host, I, costs)["order"].tolist() == [1, 2, 3]
    I, costs, min_gain = case_below_min_gain()
    got = host_select(host, I, np.zeros((3, 3), dtype=bool), costs, None, 1, min_gain)
    assert got["order"].tolist() == [1, 2] and got["rounds"] == 3
    got = host_thin(host, cm.EXACT_I, cm.EXACT_COSTS, cm.EXACT_W)
    assert got["order"].tolist() == [1, 0] and got["gains"].tolist() == [2 ** 32 - 2, 1]
    assert got["cost_kept"] == 2 ** 33 - 5 and got["weight_kept"] == 2 ** 32 - 1
    got = host_select(host, cm.EXACT_I, np.zeros((2, 2), dtype=bool), cm.EXACT_COSTS, cm.EXACT_W)
    assert got["order"].tolist() == [1, 0]


def test_the_cost_line():
    assert cm.cost_line(6, 13, 3, 4) == "  Cost:     6/13 by the kept 3 of 4\n"
    block = tm.render_block(2, 3, 1, 4, 60, 5, 65, 7, 77, 77, 130)
    assert cm.with_cost_line(block, cm.cost_line(6, 13, 3, 4)).splitlines()[-2:] == [
        "  Segments: covered 77/130 by all 125, 77/130 by the kept 9", "  Cost:     6/13 by the kept 3 of 4"]
    both = cm.with_cost_line(block, cm.cost_line(6, 13, 3, 4), wm.weight_line(1, 1, 2, 125, 9))
    assert [l[:9] for l in both.splitlines()[-3:]] == ["  Segment", "  Weight:", "  Cost:  "]
