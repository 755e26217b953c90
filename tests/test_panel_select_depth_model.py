"""The numpy model of the selection to a coverage depth (tests/panel_select_depth_model.py) against the host layer's
sequential rule (select_panel_depth through odm_select_panel_depth): random incidences under random and planted
graphs, equal gains, forced sets with neighbours, self loops and drop, T in {1, 2, 4, 64}, R in {1, 2, 3, 7, 255},
min_gain in {1, 2, 5}; the guarantees of the header (R = 1 is the selection, prefix, independence, the zero-bitmap
depth bound, counts[1] monotone, the gains identity); hand-built rows, one where the unlayered rule loses a segment;
and the figures pinned for the 13-mer grid case -- every comparison on integers, exactly.  No GPU needed."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import panel_select_depth_model as dm
import panel_select_model as sm
import panel_thin_model as tm
from test_panel_select_model import host_select
from test_panel_thin_model import grid_case

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
KEYS = ("order", "gains", "layer", "keep", "barred", "depth_all", "depth_kept", "counts")


@pytest.fixture(scope="module")
def host():
    import msspe_amd
    msspe_amd.load_library()
    return C.CDLL(str(LIB))


@pytest.fixture(scope="module")
def grid13():
    g, fwd, rev = grid_case(13, 2)
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    assert I.shape == (130, 130) and int(I.any(axis=0).sum()) == 77 and int(I.sum(axis=0).max()) == 3
    I.setflags(write=False)
    return I


def host_select_depth(host, I, B, R, T=1, min_gain=1, forced=None, drop=False):
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    rows, bits = tm.pack_rows(I), sm.pack_bitmap(B)
    order, gains, layer = (np.full(max(n, 1), -1, dtype=np.int32) for _ in range(3))
    keep = np.full(max(n, 1), 9, dtype=np.uint8)
    tube = np.full(max(n, 1), -7, dtype=np.int32)
    barred = np.full(max(n, 1), 9, dtype=np.uint8)
    d_all, d_kept = np.full(max(n_seg, 1), 9, dtype=np.uint8), np.full(max(n_seg, 1), 9, dtype=np.uint8)
    counts = np.zeros(7, dtype=np.int64)
    f = None if forced is None else np.ascontiguousarray(np.asarray(forced) != 0, dtype=np.uint8)
    host.odm_select_panel_depth.argtypes = ([C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                             C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 9)
    k = host.odm_select_panel_depth(rows.ctypes.data, n, rows.shape[1], n_seg, bits.ctypes.data, R, T, min_gain,
                                    f.ctypes.data if f is not None else None, 1 if drop else 0, order.ctypes.data,
                                    gains.ctypes.data, layer.ctypes.data, keep.ctypes.data, tube.ctypes.data,
                                    barred.ctypes.data, d_all.ctypes.data, d_kept.ctypes.data, counts.ctypes.data)
    return {"order": order[:k], "gains": gains[:k], "layer": layer[:k], "keep": keep[:n], "tube": tube[:n],
            "barred": barred[:n], "depth_all": d_all[:n_seg], "depth_kept": d_kept[:n_seg], "counts": counts[:4],
            "tubes_used": int(counts[4]), "rounds": int(counts[5]), "layers": int(counts[6])}


def same(host, I, B, R, T=1, min_gain=1, forced=None, drop=False):
    """Model == host twin, and what holds of every run: the rounds, the true counts, the gains identity, the
    independence guarantee."""
    I = np.asarray(I, dtype=bool)
    want = dm.select_depth(I, B, R, T, min_gain, forced, drop)
    got = host_select_depth(host, I, B, R, T, min_gain, forced, drop)
    for key in KEYS:
        np.testing.assert_array_equal(got[key], want[key], key)
    np.testing.assert_array_equal(np.where(got["tube"] < 0, sm.TUBE_NONE, got["tube"]), want["tube"])
    for key in ("tubes_used", "rounds", "layers"):
        assert got[key] == want[key], key
    D = int(I.sum(axis=0).max()) if I.size else 0
    assert want["layers"] == min(R, max(1, D)) and want["rounds"] == len(want["order"]) + want["layers"]
    assert (np.diff(want["layer"].astype(int)) >= 0).all()
    kept = want["keep"] != 0
    np.testing.assert_array_equal(want["depth_kept"], np.minimum(I[kept].sum(axis=0), 255))
    np.testing.assert_array_equal(want["depth_all"], np.minimum(I.sum(axis=0), 255))
    for r, total in enumerate(want["layer_sums"], start=1):     # every hit a segment takes while open counts once
        assert int(want["gains"][want["layer"] == r].sum()) == total, r
    sm.check_independent(want, B, forced, drop)
    return want


def random_case(rng, n, n_seg, density, fill=0.1):
    I = rng.random((n, n_seg)) < fill
    B = rng.random((n, n)) < density
    return I, B


@pytest.mark.parametrize("seed", range(6))
def test_random_incidences_and_graphs(host, seed):
    rng = np.random.default_rng(100 + seed)
    n, n_seg = int(rng.integers(1, 301)), int(rng.integers(1, 4001))
    if seed == 0:
        n, n_seg = 300, 4000
    if seed == 1:
        n, n_seg = 1, 1
    n_seg = min(n_seg, 600) if seed >= 4 else n_seg               # dense rows: many equal gains
    I, B = random_case(rng, n, n_seg, (0.0, 0.01, 0.05, 0.3, 0.05, 0.02)[seed], 0.5 if seed >= 4 else 0.01)
    forced = rng.random(n) < 0.05 if seed % 2 else None
    for T, R, G in ((1, 1, 1), (2, 2, 1), (4, 3, 2), (64, 7, 1), (1, 255, 5), (2, 7, 2)):
        same(host, I, B, R, T, G, forced, drop=bool(seed & 2))


def test_equal_gains_go_to_the_lowest_index(host):
    I = np.zeros((6, 8), dtype=bool)
    I[[0, 1, 2], :4] = True
    I[[3, 4, 5], 4:] = True
    B = np.zeros((6, 6), dtype=bool)
    want = same(host, I, B, 3, 1)
    assert want["order"].tolist() == [0, 3, 1, 4, 2, 5] and want["layer"].tolist() == [1, 1, 2, 2, 3, 3]
    assert want["gains"].tolist() == [4] * 6 and want["rounds"] == 9 and (want["depth_kept"] == 3).all()
    B[0, 1] = True                                               # 1 is barred by the first pick: 2 takes its place
    want = same(host, I, B, 3, 1)
    assert want["order"].tolist() == [0, 3, 2, 4, 5] and want["barred"].tolist() == [0, 1, 0, 0, 0, 0]
    want = same(host, I, B, 3, 2)                                # with a second tube 1 is kept there
    assert want["order"].tolist() == [0, 3, 1, 4, 2, 5] and want["tube"].tolist() == [0, 1, 0, 0, 0, 0]


def test_the_unlayered_rule_loses_a_segment_and_the_layers_do_not(host):
    """Primers 0 and 1 match segments 0..3; primer 2 is the only one on segment 4 and conflicts with 1.  One loop at
    R = 2 picks 0, then 1 for its four second-primer gains, and 1 bars 2: segment 4 is lost.  The layers finish
    breadth first: 0, then 2 (the last uncovered segment), and only then is 1 found barred."""
    I = np.zeros((3, 5), dtype=bool)
    I[0, :4] = I[1, :4] = True
    I[2, 4] = True
    B = np.zeros((3, 3), dtype=bool)
    B[1, 2] = True
    flat = dm.unlayered(I, B, 2)
    assert flat["order"].tolist() == [0, 1] and flat["counts"].tolist() == [5, 4, 4, 4]
    want = same(host, I, B, 2)
    assert want["order"].tolist() == [0, 2] and want["layer"].tolist() == [1, 1]
    assert want["counts"].tolist() == [5, 5, 4, 0] and want["barred"].tolist() == [0, 1, 0] and want["rounds"] == 4
    want = same(host, I, B, 2, T=2)                              # a second tube gives the depth as well
    assert want["order"].tolist() == [0, 2, 1] and want["tube"].tolist() == [0, 1, 0]
    assert want["counts"].tolist() == [5, 5, 4, 4]


def test_a_pick_counts_on_closed_segments_too(host):
    """Layer 2 picks primers 2 and 3 for segments 2 and 1; both also match segment 0, which closed at 2 of 2: its
    count is the true 4, so layer 3 needs nothing more on it and primer 4, which matches nothing else, is not
    picked.  A rule that counted open segments only would see 2 there and pick it."""
    I = np.array([[1, 1, 0], [1, 0, 1], [1, 0, 1], [1, 1, 0], [1, 0, 0]], dtype=bool)
    want = same(host, I, np.zeros((5, 5), dtype=bool), 3)
    assert want["depth_all"].tolist() == [5, 2, 2]
    assert want["order"].tolist() == [0, 1, 2, 3] and want["layer"].tolist() == [1, 1, 2, 2]
    assert want["gains"].tolist() == [2, 1, 1, 1] and want["depth_kept"].tolist() == [4, 2, 2]
    assert want["layers"] == 3 and want["rounds"] == 7


def test_forced_rows_count_first_and_bar_their_neighbours(host, grid13):
    rng = np.random.default_rng(4)
    B = rng.random((130, 130)) < 0.02
    B[np.arange(130), np.arange(130)] = False
    forced = np.zeros(130, dtype=np.uint8)
    forced[[5, 77, 100]] = 1
    B[5, 19] = B[25, 77] = True                                  # the two best picks neighbour the panel
    for T in (1, 4):
        want = same(host, grid13, B, 3, T, forced=forced)
        assert want["barred"][19] == 1 and want["barred"][25] == 1
        assert (want["tube"][forced != 0] == sm.TUBE_NONE).all() and (want["keep"][forced != 0] == 1).all()
    want = same(host, grid13, B, 2, 2, forced=np.ones(130, dtype=np.uint8))
    assert want["order"].size == 0 and want["rounds"] == 2 and want["counts"].tolist() == [77, 77, 45, 45]


def test_self_loops_and_drop(host, grid13):
    B = np.zeros((130, 130), dtype=bool)
    B[19, 19] = B[25, 25] = True
    want = same(host, grid13, B, 2, 2)
    assert want["barred"][[19, 25]].tolist() == [1, 1] and want["keep"][[19, 25]].tolist() == [0, 0]
    want = same(host, grid13, B, 2, 2, drop=True)
    assert want["order"][:2].tolist() == [19, 25] and not want["barred"].any()


@pytest.mark.parametrize("T", [1, 2, 4, 64])
def test_depth_one_is_the_selection(host, grid13, T):
    for density, G, drop in ((0.0, 1, False), (0.02, 1, False), (0.1, 2, True), (0.1, 5, False)):
        B = np.random.default_rng(5).random((130, 130)) < density
        forced = np.random.default_rng(T).random(130) < 0.04
        for f in (None, forced):
            want = same(host, grid13, B, 1, T, G, f, drop)
            flat, twin = sm.select(grid13, B, T, G, f, drop), host_select(host, grid13, B, T, G, f, drop)
            for ref in (flat, twin):
                for key in ("order", "gains", "keep", "barred"):
                    np.testing.assert_array_equal(want[key], ref[key], key)
                assert (want["tubes_used"], want["rounds"]) == (ref["tubes_used"], ref["rounds"])
                assert want["counts"][:2].tolist() == [ref["covered_all"], ref["covered_kept"]]
            np.testing.assert_array_equal(want["tube"], flat["tube"])
            assert (want["layer"] == 1).all() and want["layers"] == 1


@pytest.mark.parametrize("G", [1, 2, 5])
def test_prefix_and_breadth_never_falls(host, grid13, G):
    for density, T in ((0.1, 1), (0.1, 2), (0.02, 4), (0.0, 64)):
        B = np.random.default_rng(5).random((130, 130)) < density
        runs = [same(host, grid13, B, R, T, G) for R in (1, 2, 3, 7, 255)]
        for a, b in zip(runs, runs[1:]):
            k = len(a["order"])
            assert len(b["order"]) >= k
            for key in ("order", "gains", "layer"):
                np.testing.assert_array_equal(b[key][:k], a[key], key)
            np.testing.assert_array_equal(b["tube"][a["order"].astype(np.int64)], a["tube"][a["order"].astype(np.int64)])
            assert b["counts"][1] >= a["counts"][1]
            if G == 1:
                assert b["counts"][1] == a["counts"][1]
        assert runs[3]["layers"] == runs[4]["layers"] == 3       # D = 3: depth 7 and 255 run the same three layers
        np.testing.assert_array_equal(runs[3]["order"], runs[4]["order"])


@pytest.mark.parametrize("R", [1, 2, 3, 7, 255])
def test_zero_bitmap_reaches_the_depth(host, grid13, R):
    rng = np.random.default_rng(R)
    for I in (grid13, rng.random((40, 300)) < 0.2):
        n = I.shape[0]
        for T in (1, 4):
            want = same(host, I, np.zeros((n, n), dtype=bool), R, T)
            assert (want["depth_kept"] >= np.minimum(R, want["depth_all"])).all()
            assert want["counts"][3] == want["counts"][2] and not want["barred"].any() and want["tubes_used"] <= 1


def test_saturation_at_255(host):
    I = np.ones((300, 3), dtype=bool)
    I[:, 2] = np.arange(300) < 7
    want = same(host, I, np.zeros((300, 300), dtype=bool), 255)
    assert want["depth_all"].tolist() == [255, 255, 7] and want["depth_kept"].tolist() == [255, 255, 7]
    assert want["layers"] == 255 and len(want["order"]) == 255 and want["rounds"] == 510


PINS = [  # density, T, R, picks, counts, barred, rounds
    (0.1, 1, 1, 6, [77, 55, 77, 55], 100, 7),
    (0.1, 1, 2, 6, [77, 55, 45, 0], 100, 8),
    (0.1, 2, 2, 9, [77, 66, 45, 18], 57, 11),
    (0.1, 4, 2, 15, [77, 77, 45, 43], 15, 17),
    (0.1, 4, 3, 15, [77, 77, 8, 0], 15, 18),
    (0.02, 1, 2, 11, [77, 68, 45, 26], 50, 13),
    (0.02, 2, 2, 16, [77, 77, 45, 45], 14, 18),
    (0.02, 2, 3, 16, [77, 77, 8, 8], 14, 19),
]


@pytest.mark.parametrize("density,T,R,picks,counts,barred,rounds", PINS)
def test_pinned_figures_of_the_grid_case(host, grid13, density, T, R, picks, counts, barred, rounds):
    B = np.random.default_rng(5).random((130, 130)) < density
    want = same(host, grid13, B, R, T)
    assert (len(want["order"]), want["counts"].tolist(), int(want["barred"].sum()), want["rounds"]) == (
        picks, counts, barred, rounds)


def test_why_layered_47_against_55(grid13):
    """The example of DESIGN.md 4.16: one loop with the depth thinning's rule and barring covers 47 segments at R = 2
    where the selection, and so the layered rule, covers 55."""
    B = np.random.default_rng(5).random((130, 130)) < 0.1
    assert dm.unlayered(grid13, B, 2)["counts"].tolist()[:2] == [77, 47]
    assert dm.select_depth(grid13, B, 2)["counts"].tolist()[:2] == [77, 55]
    assert dm.unlayered(grid13, B, 1)["counts"].tolist()[:2] == [77, 55]


def test_complete_graph(host, grid13):
    want = same(host, grid13, ~np.eye(130, dtype=bool), 3, 3)
    assert want["order"].tolist() == [19, 25, 105] and want["tube"][[19, 25, 105]].tolist() == [0, 1, 2]
    assert want["layer"].tolist() == [1, 1, 1] and want["rounds"] == 6


def test_empty_inputs(host):
    for shape in ((0, 5), (4, 0), (0, 0)):
        want = same(host, np.zeros(shape, dtype=bool), np.zeros((shape[0], shape[0]), dtype=bool), 3, 2)
        assert want["order"].size == 0 and want["layers"] == 1 and want["rounds"] == 1
        assert want["counts"].tolist() == [0, 0, 0, 0]


def test_render_depth_block():
    text = dm.render_depth_block(0, 0.0, 2, 3, 1, 4, 2, 10, 40, 8, 38, 0, 12, [77, 70, 45, 30], 80, [9, 5, 3, 1])
    base = sm.render_block(0, 0.0, 2, 3, 1, 4, 10, 40, 8, 38, 0, 12, 77, 70, 80, [9, 5, 3, 1])
    lines, ref = text.split("\n"), base.split("\n")
    assert lines[1] == ref[1].replace("tubes <= 4):", "tubes <= 4, depth 2):")
    assert lines[6] == "  Depth:    at least 2 primers on 45/80 segments by all 78, on 30/80 by the kept 18"
    assert lines[:1] + lines[2:6] + lines[7:] == ref[:1] + ref[2:]
