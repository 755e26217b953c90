"""The numpy model of the selection by coverage (tests/panel_select_model.py) against the host layer's sequential rule
(select_panel through odm_select_panel): the grid inputs under random graphs, the hand-built graph shapes at the mask
and bitmap word boundaries over random incidence bitmaps, one-direction edges, forced sets whose neighbours must be
barred, min_gain above 1, the two identities (zero graph, complete graph), the independence guarantee and the CLI's
block -- every comparison on integers, exactly.  No GPU needed."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import cover_round_model as crm
import panel_select_model as sm
import panel_thin_model as tm
from test_panel_thin_model import GRID, grid_case, random_bitmap

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"


@pytest.fixture(scope="module")
def host():
    import msspe_amd
    msspe_amd.load_library()
    return C.CDLL(str(LIB))


@pytest.fixture(scope="module")
def grid_incidence():
    """The four grid cases' incidence matrices, computed once."""
    out = {}
    for k, M, _ in GRID:
        g, fwd, rev = grid_case(k, M)
        out[k, M] = tm.incidence(g, 400, 170, 50, k, fwd, rev, M, 3)
    return out


def host_select(host, I, B, T=1, min_gain=1, forced=None, drop=False):
    I = np.asarray(I, dtype=bool)
    n = I.shape[0]
    rows, bits = tm.pack_rows(I), sm.pack_bitmap(B)
    order = np.full(max(n, 1), -1, dtype=np.int32)
    gains = np.full(max(n, 1), -1, dtype=np.int32)
    keep = np.full(max(n, 1), 9, dtype=np.uint8)
    tube = np.full(max(n, 1), -7, dtype=np.int32)
    barred = np.full(max(n, 1), 9, dtype=np.uint8)
    counts = np.zeros(4, dtype=np.int64)
    f = None if forced is None else np.ascontiguousarray(np.asarray(forced) != 0, dtype=np.uint8)
    host.odm_select_panel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                      C.c_int] + [C.c_void_p] * 6
    k = host.odm_select_panel(rows.ctypes.data, n, rows.shape[1], bits.ctypes.data, T, min_gain,
                              f.ctypes.data if f is not None else None, 1 if drop else 0, order.ctypes.data,
                              gains.ctypes.data, keep.ctypes.data, tube.ctypes.data, barred.ctypes.data,
                              counts.ctypes.data)
    return {"order": order[:k], "gains": gains[:k], "keep": keep[:n], "tube": tube[:n], "barred": barred[:n],
            "covered_all": int(counts[0]), "covered_kept": int(counts[1]), "tubes_used": int(counts[2]),
            "rounds": int(counts[3])}


def same(host, I, B, T=1, min_gain=1, forced=None, drop=False):
    want = sm.select(I, B, T, min_gain, forced, drop)
    got = host_select(host, I, B, T, min_gain, forced, drop)
    for key in ("order", "gains", "keep", "barred"):
        np.testing.assert_array_equal(got[key], want[key], key)
    np.testing.assert_array_equal(np.where(got["tube"] < 0, sm.TUBE_NONE, got["tube"]), want["tube"])
    for key in ("covered_all", "covered_kept", "tubes_used", "rounds"):
        assert got[key] == want[key], key
    assert want["rounds"] == len(want["order"]) + 1 and want["covered_kept"] == int(want["covered"].sum())
    kept = want["keep"] != 0
    np.testing.assert_array_equal(np.asarray(I, dtype=bool)[kept].any(axis=0) if kept.any() else
                                  np.zeros(np.asarray(I).shape[1], dtype=bool), want["covered"])
    sm.check_independent(want, B, forced, drop)
    return want


def random_graph(n, density, seed=5, self_loops=True):
    B = np.random.default_rng(seed).random((n, n)) < density
    if not self_loops:
        B[np.arange(n), np.arange(n)] = False
    return B


@pytest.mark.parametrize("k,M,picks", GRID)
@pytest.mark.parametrize("density", [0, 0.02, 0.1, 0.3, 1])
def test_grid_cases_under_random_graphs(host, grid_incidence, k, M, picks, density):
    I = grid_incidence[k, M]
    n = I.shape[0]
    for self_loops in (True, False):
        B = random_graph(n, density, self_loops=self_loops)
        for T in (1, 2, 3, 64):
            for drop in (False, True):
                res = same(host, I, B, T, drop=drop)
                if density == 0:
                    assert len(res["order"]) == picks and res["tubes_used"] == 1
    if (k, M, density) == (13, 2, 0.1):   # the issue's figure: 6 picks cover 55 of 77 at T = 1
        res = sm.select(I, random_graph(n, 0.1), 1)
        assert (len(res["order"]), res["covered_kept"], res["covered_all"]) == (6, 55, 77)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("shape", crm.HAND_BUILT)
def test_hand_built_graphs_over_random_bitmaps(host, shape, n):
    rng = np.random.default_rng(n * 31 + len(shape))
    I = random_bitmap(rng, n, int(rng.integers(1, 400)))
    B = crm.hand_built(shape, n)
    for T in (1, 2, 64):
        same(host, I, B, T)
        same(host, I, B, T, drop=True)
    forced = rng.random(n) < 0.1
    same(host, I, B, 2, 1, forced)
    same(host, I, B, 1, 2, forced, drop=True)


def test_one_direction_edges(host):
    I = np.zeros((3, 10), dtype=bool)
    I[0, :6] = I[1, 2:9] = I[2, 9:] = True
    for B in (np.array([[0, 1, 0], [0, 0, 0], [0, 0, 0]], bool), np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0]], bool)):
        res = same(host, I, B)                     # 0 -> 1 or 1 -> 0 alone: the pair is an edge either way
        assert res["order"].tolist() == [1, 2] and res["barred"].tolist() == [1, 0, 0]
        assert res["covered_kept"] == 8 and res["covered_all"] == 10
        res = same(host, I, B, 2)                  # a second tube takes the neighbour
        assert res["order"].tolist() == [1, 0, 2] and res["tube"].tolist() == [1, 0, 0] and res["tubes_used"] == 2


def test_forced_primers_bar_their_neighbours(host):
    I = np.zeros((5, 12), dtype=bool)
    I[0, :2] = I[1, :9] = I[2, 4:11] = I[3, 11:] = I[4, :1] = True
    B = np.zeros((5, 5), dtype=bool)
    B[1, 0] = True                                 # the best primer conflicts with the forced one
    B[4, 4] = True                                 # a self loop: never live
    forced = [1, 0, 0, 0, 0]
    for T in (1, 3, 64):                           # the panel is in every tube: more tubes do not free primer 1
        res = same(host, I, B, T, 1, forced)
        assert res["order"].tolist() == [2, 3] and res["keep"].tolist() == [1, 0, 1, 1, 0]
        assert res["barred"].tolist() == [0, 1, 0, 0, 1] and res["tube"].tolist() == [255, 255, 0, 0, 255]
        assert (res["covered_kept"], res["covered_all"]) == (10, 12)
    res = same(host, I, B, 1, 1, forced, drop=True)   # without the self loop primer 4 is live, and covers nothing new
    assert res["barred"].tolist() == [0, 1, 0, 0, 0]
    every = np.ones(5, dtype=np.uint8)
    res = same(host, I, B, 2, 1, every)
    assert res["order"].size == 0 and res["tubes_used"] == 0 and not res["barred"].any()


@pytest.mark.parametrize("min_gain", [2, 5])
def test_min_gain(host, grid_incidence, min_gain):
    I = grid_incidence[13, 2]
    n = I.shape[0]
    for density in (0, 0.02, 0.1):
        B = random_graph(n, density, seed=7, self_loops=False)
        res = same(host, I, B, 2, min_gain)
        assert (res["gains"] >= min_gain).all()
        forced = np.random.default_rng(min_gain).random(n) < 0.06
        same(host, I, B, 2, min_gain, forced)


@pytest.mark.parametrize("seed", range(8))
def test_zero_graph_is_the_plain_thinning(host, seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 200))
    I = random_bitmap(rng, n, int(rng.integers(1, 2000)))
    forced = rng.random(n) < 0.1 if seed % 2 else None
    for T in (1, 5, 64):
        for G in (1, 2):
            keep, order, gains, covered, c_all, c_kept, rounds = tm.greedy(I, G, forced)
            res = same(host, I, np.zeros((n, n), dtype=bool), T, G, forced)
            np.testing.assert_array_equal(res["order"], order)
            np.testing.assert_array_equal(res["gains"], gains)
            np.testing.assert_array_equal(res["keep"], keep)
            np.testing.assert_array_equal(res["covered"], covered)
            assert (res["covered_all"], res["covered_kept"], res["rounds"]) == (c_all, c_kept, rounds)
            assert (res["tube"][order.astype(np.int64)] == 0).all() and not res["barred"].any()


@pytest.mark.parametrize("seed", range(8))
def test_complete_graph_keeps_the_first_picks(host, seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(2, 150))
    I = random_bitmap(rng, n, int(rng.integers(1, 1500)))
    B = ~np.eye(n, dtype=bool)
    _, order, gains, *_ = tm.greedy(I)
    for T in (1, 2, 3, 64):
        res = same(host, I, B, T)
        m = min(T, len(order))
        np.testing.assert_array_equal(res["order"], order[:m])
        np.testing.assert_array_equal(res["gains"], gains[:m])
        assert res["tube"][order[:m].astype(np.int64)].tolist() == list(range(m)) and res["tubes_used"] == m
        if m == T:                                   # every tube holds a neighbour of everyone else
            assert res["barred"].sum() == n - m


def test_empty_shapes(host):
    same(host, np.zeros((3, 0), dtype=bool), np.ones((3, 3), dtype=bool))
    same(host, np.zeros((1, 1), dtype=bool), np.zeros((1, 1), dtype=bool))
    res = same(host, np.ones((1, 1), dtype=bool), np.ones((1, 1), dtype=bool))
    assert res["order"].size == 0 and res["barred"].tolist() == [1]
    res = same(host, np.ones((1, 1), dtype=bool), np.ones((1, 1), dtype=bool), drop=True)
    assert res["order"].tolist() == [0]


def test_bitmap_packing_round_trip():
    for n in (1, 63, 64, 65, 129):
        B = random_graph(n, 0.3, seed=n)
        w = sm.pack_bitmap(B)
        assert w.shape == (n, (n + 63) // 64)
        np.testing.assert_array_equal(sm.unpack_bitmap(w, n), B)


def test_render_block():
    assert sm.render_block(0, 0.0, 2, 3, 1, 1, 4, 60, 5, 65, 7, 11, 77, 70, 130) == (
        "\nPanel selection by coverage (up to 2 mismatches, last 3 bases exact, gain >= 1, tubes <= 1):\n"
        "  Rule:     each round keeps the primer with the most new segments and bars its conflict neighbours from its "
        "tube\n"
        "  Primers:  kept 9 of 125 (forward 4 of 60, reverse 5 of 65), 7 forced\n"
        "  Barred:   11 by conflicts\n"
        "  Segments: covered 77/130 by all 125, 70/130 by the kept 9\n")
    assert sm.render_block("end1", 30, 2, 3, 2, 4, 4, 60, 5, 65, 0, 3, 50, 41, 130, [5, 3, 1]) == (
        "\nPanel selection by coverage (thal END1, t >= 30.00 C; matches within 2 mismatches, last 3 bases exact, "
        "gain >= 2, tubes <= 4):\n"
        "  Rule:     each round keeps the primer with the most new segments and bars its conflict neighbours from its "
        "tube\n"
        "  Primers:  kept 9 of 125 (forward 4 of 60, reverse 5 of 65), 0 forced\n"
        "  Barred:   3 by conflicts\n"
        "  Segments: held 50/130 by all 125, 41/130 by the kept 9\n"
        "  Tube 1: 5 primers\n  Tube 2: 3 primers\n  Tube 3: 1 primers\n")
