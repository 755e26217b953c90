"""The numpy model of the weighted thinning and selection (tests/panel_weighted_model.py): with w = 1 it equals the
unweighted models on the grid cases and on 200 random matrices; built cases where the weights change the first pick and
which segment a conflict costs; zero weights; min_gain in weight units; and the host layer's sequential twins
(thin_panel_weighted / select_panel_weighted through their hooks) against it on random matrices -- every comparison on
integers, exactly.  No GPU needed."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import panel_select_model as sm
import panel_thin_model as tm
import panel_weighted_model as wm
from test_panel_select_model import random_graph
from test_panel_thin_model import GRID, grid_case, random_bitmap

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


def ones_equal_the_unweighted_models(I, B, T, min_gain, forced, drop=False):
    ones = np.ones(I.shape[1], dtype=np.int64)
    plain = dict(zip(THIN, tm.greedy(I, min_gain, forced)))
    got = wm.greedy_weighted(I, ones, min_gain, forced)
    for key in THIN:
        np.testing.assert_array_equal(got[key], plain[key], key)
    assert (got["weight_all"], got["weight_kept"]) == (plain["covered_all"], plain["covered_kept"])
    plain = sm.select(I, B, T, min_gain, forced, drop)
    got = wm.select_weighted(I, B, ones, T, min_gain, forced, drop)
    for key, v in plain.items():
        np.testing.assert_array_equal(got[key], v, key)
    assert (got["weight_all"], got["weight_kept"]) == (plain["covered_all"], plain["covered_kept"])


@pytest.mark.parametrize("k,M,picks", GRID)
def test_ones_on_the_grid_cases(grid_incidence, k, M, picks):
    I = grid_incidence[k, M]
    n = I.shape[0]
    rng = np.random.default_rng(k + M)
    for density in (0, 0.05, 1):
        for T in (1, 3):
            for min_gain in (1, 2):
                ones_equal_the_unweighted_models(I, random_graph(n, density), T, min_gain, None)
    ones_equal_the_unweighted_models(I, random_graph(n, 0.05), 2, 1, rng.random(n) < 0.05, drop=True)
    assert len(wm.greedy_weighted(I, np.ones(I.shape[1]))["order"]) == picks


def test_ones_on_200_random_matrices():
    for seed in range(200):
        rng = np.random.default_rng(seed)
        n, n_seg = int(rng.integers(1, 60)), int(rng.integers(1, 300))
        I = random_bitmap(rng, n, n_seg)
        forced = rng.random(n) < 0.1 if seed % 3 == 0 else None
        ones_equal_the_unweighted_models(I, random_graph(n, float(rng.choice([0, 0.05, 0.3])), seed=seed),
                                         int(rng.choice([1, 2, 64])), int(rng.choice([1, 2])), forced, bool(seed % 2))


def test_the_weights_change_the_first_pick():
    I = np.zeros((2, 12), dtype=bool)
    I[0, :9] = True                                     # nine common segments
    I[1, 9:] = True                                     # three rare ones
    assert tm.greedy(I)[1].tolist() == [0, 1]
    w = np.ones(12, dtype=np.int64)
    w[9:] = 4
    res = wm.greedy_weighted(I, w)
    assert res["order"].tolist() == [1, 0] and res["gains"].tolist() == [12, 9]
    assert res["weight_kept"] == res["weight_all"] == 21 and res["covered_kept"] == 12
    w[9:] = 3                                           # a tie in weight: the lowest index
    assert wm.greedy_weighted(I, w)["order"].tolist() == [0, 1]


def test_the_weights_change_which_segment_a_conflict_costs():
    I = np.zeros((3, 10), dtype=bool)
    I[0, :6] = I[1, 4:9] = I[2, 9:] = True
    B = np.zeros((3, 3), dtype=bool)
    B[0, 1] = True
    plain = sm.select(I, B)
    assert plain["order"].tolist() == [0, 2] and plain["barred"].tolist() == [0, 1, 0]   # segments 6..8 are lost
    w = np.ones(10, dtype=np.int64)
    w[6:9] = 5
    res = wm.select_weighted(I, B, w)
    assert res["order"].tolist() == [1, 2] and res["barred"].tolist() == [1, 0, 0]       # now 0..3 are
    assert res["gains"].tolist() == [17, 1] and (res["weight_kept"], res["weight_all"]) == (18, 22)
    assert res["covered"].tolist() == [False] * 4 + [True] * 6
    sm.check_independent(res, B)
    two = wm.select_weighted(I, B, w, T=2)              # a second tube: nothing is lost
    assert two["order"].tolist() == [1, 0, 2] and two["tube"].tolist() == [1, 0, 0]
    assert two["weight_kept"] == two["weight_all"]


def test_zero_weights():
    I = np.zeros((3, 8), dtype=bool)
    I[0, :5] = I[1, 3:7] = I[2, 7:] = True
    w = np.array([0, 0, 0, 0, 0, 2, 2, 0])
    res = wm.greedy_weighted(I, w)
    assert res["order"].tolist() == [1] and res["gains"].tolist() == [4]      # 0 and 2 cover weight 0 only
    assert res["covered"].tolist() == [False] * 3 + [True] * 4 + [False]      # 3 and 4 are marked although they weigh 0
    assert (res["covered_all"], res["covered_kept"], res["weight_all"], res["weight_kept"]) == (8, 4, 4, 4)
    none = wm.greedy_weighted(I, np.zeros(8))
    assert none["order"].size == 0 and none["rounds"] == 1 and none["weight_all"] == 0
    sel = wm.select_weighted(I, np.zeros((3, 3), dtype=bool), w, 2)
    assert sel["order"].tolist() == [1] and not sel["barred"].any()


def test_min_gain_is_in_weight_units():
    I = np.zeros((3, 9), dtype=bool)
    I[0, :6] = I[1, 6:8] = I[2, 8:] = True
    w = np.array([1, 1, 1, 1, 1, 1, 10, 10, 3])
    assert wm.greedy_weighted(I, w, 1)["order"].tolist() == [1, 0, 2]
    res = wm.greedy_weighted(I, w, 4)                   # six segments of weight 1 pass, one of weight 3 does not
    assert res["order"].tolist() == [1, 0] and res["gains"].tolist() == [20, 6]
    assert (res["weight_kept"], res["weight_all"]) == (26, 29)
    assert wm.greedy_weighted(I, w, 7)["order"].tolist() == [1]
    assert wm.greedy_weighted(I, w, 21)["order"].size == 0
    assert tm.greedy(I, 4)[1].tolist() == [0]           # the unweighted rule counts heads


def test_the_total_is_bounded():
    I = np.ones((1, 2), dtype=bool)
    res = wm.greedy_weighted(I, [2 ** 31 - 1, 2 ** 31])
    assert res["gains"].tolist() == [2 ** 32 - 1]
    with pytest.raises(AssertionError):
        wm.greedy_weighted(I, [2 ** 31, 2 ** 31])


# ---- the host twins -----------------------------------------------------------------------------------------------
def host_thin(host, I, w, min_gain=1, forced=None):
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    rows = tm.pack_rows(I)
    weights = np.ascontiguousarray(w, dtype=np.uint32)
    order = np.full(max(n, 1), -1, dtype=np.int32)
    gains = np.zeros(max(n, 1), dtype=np.uint32)
    keep = np.full(max(n, 1), 9, dtype=np.uint8)
    sums = np.zeros(4, dtype=np.uint64)
    f = None if forced is None else np.ascontiguousarray(np.asarray(forced) != 0, dtype=np.uint8)
    host.odm_thin_panel_weighted.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_longlong] + [C.c_void_p] * 5
    k = host.odm_thin_panel_weighted(rows.ctypes.data, n, rows.shape[1], weights.ctypes.data, n_seg, min_gain,
                                     f.ctypes.data if f is not None else None, order.ctypes.data, gains.ctypes.data,
                                     keep.ctypes.data, sums.ctypes.data)
    return {"order": order[:k], "gains": gains[:k], "keep": keep[:n], "covered_all": int(sums[0]),
            "covered_kept": int(sums[1]), "weight_all": int(sums[2]), "weight_kept": int(sums[3])}


def host_select(host, I, B, w, T=1, min_gain=1, forced=None, drop=False):
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    rows, bits = tm.pack_rows(I), sm.pack_bitmap(B)
    weights = np.ascontiguousarray(w, dtype=np.uint32)
    order = np.full(max(n, 1), -1, dtype=np.int32)
    gains = np.zeros(max(n, 1), dtype=np.uint32)
    keep = np.full(max(n, 1), 9, dtype=np.uint8)
    tube = np.full(max(n, 1), -7, dtype=np.int32)
    barred = np.full(max(n, 1), 9, dtype=np.uint8)
    sums = np.zeros(6, dtype=np.uint64)
    f = None if forced is None else np.ascontiguousarray(np.asarray(forced) != 0, dtype=np.uint8)
    host.odm_select_panel_weighted.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                               C.c_longlong, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    k = host.odm_select_panel_weighted(rows.ctypes.data, n, rows.shape[1], bits.ctypes.data, weights.ctypes.data, n_seg,
                                       T, min_gain, f.ctypes.data if f is not None else None, 1 if drop else 0,
                                       order.ctypes.data, gains.ctypes.data, keep.ctypes.data, tube.ctypes.data,
                                       barred.ctypes.data, sums.ctypes.data)
    return {"order": order[:k], "gains": gains[:k], "keep": keep[:n], "tube": tube[:n], "barred": barred[:n],
            "covered_all": int(sums[0]), "covered_kept": int(sums[1]), "tubes_used": int(sums[2]),
            "rounds": int(sums[3]), "weight_all": int(sums[4]), "weight_kept": int(sums[5])}


def draw_weights(rng, n_seg):
    w = rng.choice([0, 1, 1, 2, 3, 7], size=n_seg).astype(np.int64)
    big = rng.random(n_seg) < 0.05
    w[big] = rng.integers(1000, 20_000_000, size=int(big.sum()))
    return w


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("n_seg", [1, 53, 54, 160])
def test_the_host_twins_equal_the_models(host, n, n_seg):
    rng = np.random.default_rng(1000 * n + n_seg)
    I = random_bitmap(rng, n, n_seg)
    w = draw_weights(rng, n_seg)
    B = random_graph(n, 0.05, seed=n + n_seg)
    for min_gain, forced in ((1, None), (3, rng.random(n) < 0.1)):
        want = wm.greedy_weighted(I, w, min_gain, forced)
        got = host_thin(host, I, w, min_gain, forced)
        for key, v in got.items():
            np.testing.assert_array_equal(v, want[key], key)
        for T, drop in ((1, False), (2, True), (64, False)):
            want = wm.select_weighted(I, B, w, T, min_gain, forced, drop)
            got = host_select(host, I, B, w, T, min_gain, forced, drop)
            for key, v in got.items():
                ref = np.where(want[key] == sm.TUBE_NONE, -1, want[key].astype(np.int32)) if key == "tube" else want[key]
                np.testing.assert_array_equal(v, ref, key)
            sm.check_independent(want, B, forced, drop)
    ones = np.ones(n_seg, dtype=np.int64)               # the twins at weight 1 are the unweighted hooks' answers
    plain = tm.greedy(I)
    got = host_thin(host, I, ones)
    np.testing.assert_array_equal(got["order"], plain[1])
    np.testing.assert_array_equal(got["gains"], plain[2])
    assert (got["weight_all"], got["weight_kept"]) == (plain[4], plain[5])


def test_a_gain_above_2_to_the_31_on_the_host(host):
    I = np.ones((1, 3), dtype=bool)
    got = host_thin(host, I, [2 ** 31 - 1, 2 ** 31 - 1, 1])
    assert got["gains"].tolist() == [2 ** 32 - 1] and got["weight_kept"] == 2 ** 32 - 1


def test_the_weight_line():
    assert wm.weight_line(21, 18, 40, 125, 9) == "  Weight:   covered 21/40 by all 125, 18/40 by the kept 9\n"
    block = tm.render_block(2, 3, 1, 4, 60, 5, 65, 7, 77, 77, 130)
    assert wm.with_weight_line(block, wm.weight_line(1, 1, 2, 125, 9)).splitlines()[-2:] == [
        "  Segments: covered 77/130 by all 125, 77/130 by the kept 9",
        "  Weight:   covered 1/2 by all 125, 1/2 by the kept 9"]
