"""The numpy model of the thinning to a depth (tests/panel_thin_depth_model.py) against the host layer's sequential rule
(thin_panel_depth through odm_thin_panel_depth, thin_shadows through odm_thin_shadows): random bitmaps with planted
duplicates, equal gains and forced sets, forced duplicates, R in {1, 2, 3, 7, 255}, min_gain in {1, 2, 5}; at R = 1
equality with panel_thin_model.greedy and odm_thin_panel; the guarantee, both count identities and the gain sum; the
project's grid inputs with their picks and depths.  Every comparison on integers, exactly.  No GPU needed."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import panel_thin_depth_model as dm
import panel_thin_model as tm
from test_panel_thin_model import GRID, grid_case, host_thin, random_bitmap

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
# (k, M) -> (picks at R = 2, segments at depth >= 2, picks at R = 3, segments at depth >= 3), E = 3
DEPTH_GRID = {(13, 0): (6, 6, 6, 0), (13, 1): (12, 39, 14, 15), (13, 2): (16, 45, 16, 8), (24, 2): (7, 10, 7, 0)}


@pytest.fixture(scope="module")
def host():
    import msspe_amd
    msspe_amd.load_library()
    return C.CDLL(str(LIB))


def host_depth(host, I, depth, min_gain=1, forced=None, shadow=None):
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    rows = tm.pack_rows(I)
    order = np.full(max(n, 1), -1, dtype=np.int32)
    gains = np.full(max(n, 1), -1, dtype=np.int32)
    keep = np.full(max(n, 1), 9, dtype=np.uint8)
    d_all = np.full(max(n_seg, 1), 7, dtype=np.uint8)
    d_kept = np.full(max(n_seg, 1), 7, dtype=np.uint8)
    counts = np.zeros(5, dtype=np.int64)
    f = None if forced is None else np.ascontiguousarray(np.asarray(forced) != 0, dtype=np.uint8)
    s = None if shadow is None else np.ascontiguousarray(np.asarray(shadow) != 0, dtype=np.uint8)
    vp = C.c_void_p
    host.odm_thin_panel_depth.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                          vp]
    k = host.odm_thin_panel_depth(rows.ctypes.data, n, rows.shape[1], n_seg, depth, min_gain,
                                  f.ctypes.data if f is not None else None, s.ctypes.data if s is not None else None,
                                  order.ctypes.data, gains.ctypes.data, keep.ctypes.data, d_all.ctypes.data,
                                  d_kept.ctypes.data, counts.ctypes.data)
    return keep[:n], order[:k], gains[:k], d_all[:n_seg], d_kept[:n_seg], counts[:4], int(counts[4])


def same(host, I, depth, min_gain=1, forced=None, shadow=None):
    """Model == host twin, and the properties that hold for every input."""
    want = dm.greedy_depth(I, depth, min_gain, forced, shadow)
    keep, order, gains, d_all, d_kept, counts, rounds, cnt0, cnt = want
    got = host_depth(host, I, depth, min_gain, forced, shadow)
    np.testing.assert_array_equal(got[1], order)
    np.testing.assert_array_equal(got[2], gains)
    np.testing.assert_array_equal(got[0], keep)
    np.testing.assert_array_equal(got[3], d_all)
    np.testing.assert_array_equal(got[4], d_kept)
    np.testing.assert_array_equal(got[5], counts)
    assert got[6] == rounds == len(order) + 1
    assert int(gains.sum()) == int((cnt - cnt0).sum())           # a gain is the counters it bumps
    if shadow is not None and np.asarray(shadow).any():
        sh = np.asarray(shadow) != 0
        f = np.zeros(len(sh), dtype=bool) if forced is None else np.asarray(forced) != 0
        np.testing.assert_array_equal(keep[sh], f[sh].astype(np.uint8))   # a shadow's keep is its forced flag
        assert not set(order.tolist()) & set(np.flatnonzero(sh).tolist())
    if min_gain == 1:                                            # the guarantee and both count identities
        assert (d_kept.astype(int) >= np.minimum(depth, d_all.astype(int))).all()
        assert counts[1] == counts[0] and counts[3] == counts[2]
    if depth == 1 and (shadow is None or not np.asarray(shadow).any()):
        k1, o1, g1, cov1, c_all, c_kept, r1 = tm.greedy(I, min_gain, forced)
        np.testing.assert_array_equal(order, o1)
        np.testing.assert_array_equal(gains, g1)
        np.testing.assert_array_equal(keep, k1)
        assert rounds == r1 and (counts[0], counts[1]) == (c_all, c_kept)
        h = host_thin(host, I, min_gain, forced)
        np.testing.assert_array_equal(h[1], order)
        np.testing.assert_array_equal(h[0], keep)
    return want


def words_of(I):
    """One word per distinct row, so that equal rows are the planted duplicates (a word's row is a function of it)."""
    seen = {}
    return [seen.setdefault(r.tobytes(), len(seen)) for r in np.asarray(I, dtype=bool)]


def depth_one_equals_the_thinning(host, I, n_fwd, min_gain, forced):
    """At R = 1 the shadows change nothing: order, gains, keep and rounds are the plain thinning's on the same rows."""
    w = words_of(I)
    sh = dm.shadows(w[:n_fwd], w[n_fwd:], forced)
    keep, order, gains, d_all, d_kept, counts, rounds, _, _ = same(host, I, 1, min_gain, forced, sh)
    k1, o1, g1, cov1, c_all, c_kept, r1 = tm.greedy(I, min_gain, forced)
    np.testing.assert_array_equal(order, o1)
    np.testing.assert_array_equal(gains, g1)
    np.testing.assert_array_equal(keep, k1)
    assert rounds == r1 and (counts[0], counts[1]) == (c_all, c_kept)
    h = host_thin(host, I, min_gain, forced)
    np.testing.assert_array_equal(h[1], order)
    np.testing.assert_array_equal(h[2], gains)
    np.testing.assert_array_equal(h[0], keep)
    return sh


@pytest.mark.parametrize("seed", range(10))
def test_random_bitmaps(host, seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 301)) if seed else 300
    n_seg = int(rng.integers(1, 4001)) if seed else 4000
    I = random_bitmap(rng, n, n_seg)
    n_fwd = int(rng.integers(0, n + 1))
    forced = rng.random(n) < 0.1
    lo = hi = None
    if n >= 8:
        a, b, c, d = (int(x) for x in rng.choice(n, size=4, replace=False))
        lo, hi = sorted((a, b))
        I[hi] = I[lo]                       # a forced duplicate of a lower unforced index
        forced[lo], forced[hi] = False, True
        I[d] = I[c]                         # two forced duplicates
        forced[c] = forced[d] = True
    for f in (None, forced):
        for G in (1, 2, 5):
            sh = depth_one_equals_the_thinning(host, I, n_fwd, G, f)
            for R in (2, 3, 7, 255):
                same(host, I, R, G, f, sh)
                if R == 2 and G == 1:
                    same(host, I, R, G, f, None)
    if lo is not None and (lo < n_fwd) == (hi < n_fwd):   # one direction: the unforced lower index is a shadow
        w = words_of(I)
        assert dm.shadows(w[:n_fwd], w[n_fwd:], forced)[lo] == 1


def test_shadows_by_hand(host):
    fwd, rev = ["AC", "GG", "AC", "AC", "TT"], ["AC", "TT", "TT"]
    assert dm.shadows(fwd, rev).tolist() == [0, 0, 1, 1, 0, 0, 0, 1]
    assert dm.shadows(fwd, rev, [0, 0, 0, 1, 0, 0, 0, 0]).tolist() == [1, 0, 1, 0, 0, 0, 0, 1]   # forced 3 represents
    assert dm.shadows(fwd, rev, [0, 0, 1, 1, 0, 0, 1, 1]).tolist() == [1, 0, 0, 1, 0, 0, 0, 1]   # two forced: lowest
    assert dm.shadows([], []).tolist() == []
    host.odm_thin_shadows.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p]
    for forced in (None, [0, 0, 0, 1, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0, 1, 1], [1] * 8):
        out = np.full(8, 9, dtype=np.uint8)
        f = None if forced is None else np.array(forced, dtype=np.uint8)
        k = host.odm_thin_shadows("\n".join(fwd).encode(), "\n".join(rev).encode(),
                                  f.ctypes.data if f is not None else None, out.ctypes.data)
        want = dm.shadows(fwd, rev, forced)
        assert out.tolist() == want.tolist() and k == int(want.sum())


def test_hand_built_rows(host):
    z = np.zeros((5, 70), dtype=bool)
    keep, order, gains, d_all, d_kept, counts, rounds, _, _ = same(host, z, 2)
    assert order.size == 0 and counts.tolist() == [0, 0, 0, 0] and rounds == 1
    I = z.copy()
    I[0, :40] = I[1, 20:60] = I[2, 30:70] = True
    I[3] = I[0]                                                   # 3 repeats 0's word
    sh = np.array([0, 0, 0, 1, 0], dtype=np.uint8)
    keep, order, gains, d_all, d_kept, counts, _, _, _ = same(host, I, 2, shadow=sh)
    assert order.tolist() == [0, 1, 2] and gains.tolist() == [40, 40, 30] and keep.tolist() == [1, 1, 1, 0, 0]
    assert d_all[:20].tolist() == [1] * 20 and d_all[30:40].tolist() == [3] * 10
    # without the shadow flag the duplicate passes for a second primer: false redundancy, what the flags are for
    keep2, order2, _, d_all2, _, _, _, _, _ = same(host, I, 2)
    assert order2.tolist() == [0, 1, 2, 3] and keep2.tolist() == [1, 1, 1, 1, 0] and d_all2[:20].tolist() == [2] * 20
    # forced representatives count first: 0 forced leaves 1 and 2 to finish depth 2
    keep, order, gains, _, d_kept, _, _, cnt0, _ = same(host, I, 2, forced=[1, 0, 0, 0, 0], shadow=sh)
    assert order.tolist() == [1, 2] and gains.tolist() == [40, 30] and cnt0[:40].tolist() == [1] * 40
    # everything forced: nothing picked, a shadow's keep is its forced flag
    keep, order, _, d_all, d_kept, counts, _, _, _ = same(host, I, 3, forced=[1, 1, 1, 1, 1], shadow=sh)
    assert order.size == 0 and keep.tolist() == [1] * 5 and (d_all == d_kept).all()
    keep, order, _, _, _, _, _, _, _ = same(host, I, 3, forced=[0, 0, 0, 1, 0], shadow=[1, 0, 0, 0, 0])
    assert keep.tolist() == [0, 1, 1, 1, 0]
    # saturation: 300 rows on one segment
    ones = np.ones((300, 3), dtype=bool)
    keep, order, gains, d_all, d_kept, counts, rounds, _, _ = same(host, ones, 255)
    assert order.tolist() == list(range(255)) and d_all.tolist() == [255] * 3 and d_kept.tolist() == [255] * 3
    assert rounds == 256 and counts.tolist() == [3, 3, 3, 3]
    same(host, np.zeros((3, 0), dtype=bool), 2)
    same(host, np.ones((1, 1), dtype=bool), 2)


@pytest.mark.parametrize("k,M,picks", GRID)
def test_grid_cases(host, k, M, picks):
    g, fwd, rev = grid_case(k, M)
    I = tm.incidence(g, 400, 170, 50, k, fwd, rev, M, 3)
    sh = dm.shadows(fwd, rev)
    one = same(host, I, 1, shadow=sh)
    assert len(one[1]) == picks
    np.testing.assert_array_equal(one[1], tm.greedy(I)[1])
    p2, s2, p3, s3 = DEPTH_GRID[(k, M)]
    two = same(host, I, 2, shadow=sh)
    three = same(host, I, 3, shadow=sh)
    assert (len(two[1]), int(two[5][3])) == (p2, s2)
    assert (len(three[1]), int(three[5][3])) == (p3, s3)
    for G in (2, 5):
        same(host, I, 2, G, shadow=sh)
    rng = np.random.default_rng(k + M)
    forced = rng.random(I.shape[0]) < 0.05
    same(host, I, 2, 1, forced, dm.shadows(fwd, rev, forced))

