"""The numpy model of the panel thinning (tests/panel_thin_model.py) against the host layer's sequential rule
(thin_panel through odm_thin_panel): the project's grid inputs, random bitmaps with planted duplicates and equal gains,
forced sets, min_gain above 1 and hand-built rows -- every comparison on integers, exactly.  No GPU needed."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import coverage_mm_model as cm
import panel_thin_model as tm
from test_coverage_mm_model import draw_primers, rc

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
GRID = [(13, 0, 6), (13, 1, 8), (13, 2, 10), (24, 2, 5)]   # k, M, picks a greedy set cover needs (E = 3)


def grid_case(k, M):
    """The inputs of test_gpu_coverage_mismatch.py::test_grid_equals_the_model."""
    import msspe_amd
    g = msspe_amd.synth.aligned_genomes(10, 2600, seed=40 + k)
    rng = np.random.default_rng(100 * k + M)
    fwd = draw_primers(rng, g, 60, k)
    rev = [rc(w) for w in draw_primers(rng, g, 60, k)]
    return g, fwd, rev


@pytest.fixture(scope="module")
def host():
    import msspe_amd
    msspe_amd.load_library()
    return C.CDLL(str(LIB))


def host_thin(host, I, min_gain=1, forced=None):
    I = np.asarray(I, dtype=bool)
    n = I.shape[0]
    rows = tm.pack_rows(I)
    order = np.full(max(n, 1), -1, dtype=np.int32)
    gains = np.full(max(n, 1), -1, dtype=np.int32)
    keep = np.full(max(n, 1), 9, dtype=np.uint8)
    cov = np.zeros(2, dtype=np.int64)
    f = None if forced is None else np.ascontiguousarray(np.asarray(forced) != 0, dtype=np.uint8)
    host.odm_thin_panel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
    k = host.odm_thin_panel(rows.ctypes.data, n, rows.shape[1], min_gain, f.ctypes.data if f is not None else None,
                            order.ctypes.data, gains.ctypes.data, keep.ctypes.data, cov.ctypes.data)
    return keep[:n], order[:k], gains[:k], int(cov[0]), int(cov[1])


def same(host, I, min_gain=1, forced=None):
    keep, order, gains, covered, c_all, c_kept, rounds = tm.greedy(I, min_gain, forced)
    h_keep, h_order, h_gains, h_all, h_kept = host_thin(host, I, min_gain, forced)
    np.testing.assert_array_equal(h_order, order)
    np.testing.assert_array_equal(h_gains, gains)
    np.testing.assert_array_equal(h_keep, keep)
    assert (h_all, h_kept) == (c_all, c_kept)
    assert rounds == len(order) + 1 and c_kept == int(covered.sum())
    if min_gain == 1:
        assert c_all == c_kept
    return keep, order, gains, c_all, c_kept


@pytest.mark.parametrize("k,M,picks", GRID)
def test_grid_cases(host, k, M, picks):
    g, fwd, rev = grid_case(k, M)
    I = tm.incidence(g, 400, 170, 50, k, fwd, rev, M, 3)
    best, counts = cm.best_and_counts(g, 400, 170, 50, k, fwd, rev, M, 3)
    np.testing.assert_array_equal(I.sum(axis=1), counts)
    np.testing.assert_array_equal(I.any(axis=0), best != 255)
    keep, order, gains, c_all, c_kept = same(host, I)
    assert len(order) == picks
    assert c_all == int((best != 255).sum())
    np.testing.assert_array_equal(I[keep != 0].any(axis=0), best != 255)   # the guarantee at min_gain 1
    for G in (2, 5):
        same(host, I, G)
    rng = np.random.default_rng(k + M)
    same(host, I, 1, rng.random(I.shape[0]) < 0.05)


def random_bitmap(rng, n, n_seg):
    I = rng.random((n, n_seg)) < rng.choice([0.002, 0.02, 0.2])
    for _ in range(max(1, n // 10)):                 # planted duplicates
        a, b = rng.integers(n, size=2)
        I[a] = I[b]
    for _ in range(max(1, n // 10)):                 # planted equal gains: a row's bits moved to other segments
        a, b = rng.integers(n, size=2)
        I[a] = rng.permutation(I[b])
    return I


@pytest.mark.parametrize("seed", range(12))
def test_random_bitmaps(host, seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 301)) if seed else 300
    n_seg = int(rng.integers(1, 4001)) if seed else 4000
    I = random_bitmap(rng, n, n_seg)
    same(host, I)
    same(host, I, 2)
    same(host, I, 5)
    forced = rng.random(n) < 0.1
    same(host, I, 1, forced)
    same(host, I, 2, forced)
    _, order, gains, _, _ = same(host, I)
    assert (np.diff(gains.astype(np.int64)) <= 0).all()        # greedy gains never rise
    ties = [i for i in range(len(order) - 1) if gains[i] == gains[i + 1]]
    assert seed or ties                                        # the dense case does hold equal gains


def test_hand_built_rows(host):
    z = np.zeros((4, 70), dtype=bool)
    keep, order, gains, c_all, c_kept = same(host, z)
    assert order.size == 0 and keep.tolist() == [0, 0, 0, 0] and (c_all, c_kept) == (0, 0)
    one = z.copy()
    one[2] = True
    one[0, :10] = True
    keep, order, gains, _, _ = same(host, one)
    assert order.tolist() == [2] and gains.tolist() == [70] and keep.tolist() == [0, 0, 1, 0]
    twins = z.copy()
    twins[1, 5:40] = twins[3, 5:40] = True
    keep, order, gains, _, _ = same(host, twins)
    assert order.tolist() == [1] and gains.tolist() == [35] and keep.tolist() == [0, 1, 0, 0]
    forced = one.copy()
    keep, order, gains, c_all, c_kept = same(host, forced, 1, [0, 0, 1, 0])
    assert order.size == 0 and keep.tolist() == [0, 0, 1, 0] and (c_all, c_kept) == (70, 70)
    keep, order, gains, c_all, c_kept = same(host, one, 71)
    assert order.size == 0 and keep.tolist() == [0, 0, 0, 0] and (c_all, c_kept) == (70, 0)
    # equal gains across the list: the lowest index first, then what is left
    tie = z.copy()
    tie[3, 0:6] = tie[1, 3:9] = True
    keep, order, gains, _, _ = same(host, tie)
    assert order.tolist() == [1, 3] and gains.tolist() == [6, 3]
    same(host, np.zeros((3, 0), dtype=bool))
    same(host, np.zeros((1, 1), dtype=bool))
    same(host, np.ones((1, 1), dtype=bool))


def test_render_block():
    assert tm.render_block(2, 3, 1, 4, 60, 5, 65, 7, 77, 77, 130) == (
        "\nPanel thinning (up to 2 mismatches, last 3 bases exact, gain >= 1):\n"
        "  Primers:  kept 9 of 125 (forward 4 of 60, reverse 5 of 65), 7 forced\n"
        "  Segments: covered 77/130 by all 125, 77/130 by the kept 9\n")
