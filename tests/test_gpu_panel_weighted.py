"""msspe_panel_thin_weighted* and msspe_panel_select_weighted* on the device against the numpy model
(tests/panel_weighted_model.py): order, gains, keep, covered, both counts, both weights, tubes and barred, exactly.
All-ones weights against the unweighted calls, random weights at every group boundary, both word widths, more primers
than one block of the update, more than two batches of rounds, a pick that touches more groups than the update's grid,
a total of exactly 2^32 - 1, zero weights and the guarantee through the existing coverage call, forced primers and
min_gain in weight units, the selection's identities and graphs, the seed rule's modes 1 and 2, the call that screens
itself under a conflict rule, a second call of another size on the same context, and the argument errors."""
import ctypes as C

import numpy as np
import pytest

import coverage_thal_model as ctm
import panel_select_model as sm
import panel_thin_model as tm
import panel_thin_thal_model as ttm
import panel_weighted_model as wm
from test_coverage_mm_model import draw_primers, rc
from test_panel_thin_model import GRID, grid_case

pytestmark = pytest.mark.gpu
THIN_KEYS = ("order", "gains", "keep")
COUNTS = ("covered_all", "covered_kept", "weight_all", "weight_kept")


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def grid13():
    """(genomes, fwd, rev, incidence at M = 2, E = 3) of the k = 13 grid case, computed once and never written."""
    g, fwd, rev = grid_case(13, 2)
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    I.setflags(write=False)
    return g, fwd, rev, I


def draw_weights(rng, n_seg):
    """0, 1, small and a few large weights; the total stays far below 2^32."""
    w = rng.choice([0, 1, 1, 2, 3, 7], size=n_seg).astype(np.int64)
    big = rng.random(n_seg) < 0.05
    w[big] = rng.integers(1000, 2_000_000, size=int(big.sum()))
    return w


def primer_sets(rng, g, n, k):
    return draw_primers(rng, g, n, k), [rc(w) for w in draw_primers(rng, g, n, k)]


def distinct_sets(rng, g, n_f, n_r, k):
    words = list(dict.fromkeys(draw_primers(rng, g, 2 * (n_f + n_r), k)))
    fwd = words[:n_f]
    rev = [w for w in dict.fromkeys(rc(x) for x in words[n_f:]) if w not in set(fwd)][:n_r]
    assert len(fwd) == n_f and len(rev) == n_r and len(set(fwd + rev)) == n_f + n_r
    return fwd, rev


def thin_dict(got):
    keys = ("keep", "order", "gains", "covered", "covered_all", "covered_kept", "weight_all", "weight_kept")
    return dict(zip(keys, got))


def agree(got, want, what="", keys=THIN_KEYS):
    for key in keys:
        np.testing.assert_array_equal(got[key], want[key], f"{key} {what}")
    np.testing.assert_array_equal(got["covered"].reshape(-1), want["covered"].astype(np.uint8), f"covered {what}")
    for key in COUNTS:
        assert got[key] == want[key], f"{key} {what}"


def thin_check(eng, g, opt, fwd, rev, I, w, min_gain=1, forced=None, forms=("host",), M=2, E=3):
    want = wm.greedy_weighted(I, w, min_gain, forced)
    for form in forms:
        got = thin_dict(eng.panel_thin_weighted(g, opt, fwd, rev, M, E, w, min_gain, forced, form))
        agree(got, want, form)
        if I.size:
            assert eng.info("panel_thin_rounds") == want["rounds"], form
    if min_gain == 1:
        assert want["weight_kept"] == want["weight_all"]
    return want


def select_check(m, eng, g, opt, fwd, rev, I, B, w, T=1, min_gain=1, forced=None, drop=False, forms=("dev",),
                 rule=None):
    want = wm.select_weighted(I, B, w, T, min_gain, forced, drop)
    sm.check_independent(want, B, forced, drop)
    for form in forms:
        got = eng.panel_select_weighted(g, opt, fwd, rev, rule or m.seed_rule(2, 3), w, sm.pack_bitmap(B), T, min_gain,
                                        drop, forced, form)
        agree(got, want, form, THIN_KEYS + ("tube", "barred"))
        assert got["tubes_used"] == want["tubes_used"], form
        if I.size:
            assert eng.info("panel_select_rounds") == want["rounds"], form
    return want


# ---- the thinning -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,M,picks", GRID)
def test_all_ones_equal_the_unweighted_call_in_the_three_forms(m, eng, k, M, picks):
    g, fwd, rev = grid_case(k, M)
    opt = m.KmerOpt(400, 170, 50, k, 0, 0)
    ones = np.ones(130, dtype=np.uint32)
    for form in ("host", "dev", "packed"):
        plain = eng.panel_thin(g, opt, fwd, rev, M, 3, 1, None, form)
        rounds = eng.info("panel_thin_rounds")
        got = eng.panel_thin_weighted(g, opt, fwd, rev, M, 3, ones, 1, None, form)
        for a, b in zip(got[:6], plain):
            np.testing.assert_array_equal(a, b, form)
        assert got[6] == plain[4] and got[7] == plain[5] and len(got[1]) == picks
        assert eng.info("panel_thin_rounds") == rounds
    forced = np.random.default_rng(k + M).random(len(fwd) + len(rev)) < 0.06
    for G in (1, 2):
        plain = eng.panel_thin(g, opt, fwd, rev, M, 3, G, forced, "packed")
        got = eng.panel_thin_weighted(g, opt, fwd, rev, M, 3, ones, G, forced, "packed")
        for a, b in zip(got[:6], plain):
            np.testing.assert_array_equal(a, b)
        assert got[6:] == plain[4:]


@pytest.mark.parametrize("n_seq,L,n_seg", [(1, 400, 1), (4, 2440, 52), (53, 450, 53), (6, 1760, 54), (107, 500, 107),
                                           (10, 2950, 160)])
def test_random_weights_at_the_group_boundaries(m, eng, n_seq, L, n_seg):
    """53 segments per group: the padding bits of a group, and a last group that holds one segment (54, 107, 160)."""
    g = m.synth.aligned_genomes(n_seq, L, seed=n_seg)
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    assert n_seq * tm.n_partitions(L, 400, 170) == n_seg
    rng = np.random.default_rng(n_seg)
    fwd, rev = primer_sets(rng, g, 30, 13)
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    thin_check(eng, g, opt, fwd, rev, I, draw_weights(rng, n_seg), forms=("host", "packed"))
    assert eng.info("panel_thin_groups") == -(-n_seg // 53)


@pytest.mark.parametrize("k,W", [(13, 50), (17, 50), (31, 70), (13, 13)])
def test_word_widths_and_windows(m, eng, k, W):
    g = m.synth.aligned_genomes(6, 3000, seed=7)
    rng = np.random.default_rng(k + W)
    fwd, rev = primer_sets(rng, g, 25, k)
    opt = m.KmerOpt(max(W, 300), 150, W, k, 0, 0)
    I = tm.incidence(g, max(W, 300), 150, W, k, fwd, rev, 2, 1, 4)
    thin_check(eng, g, opt, fwd, rev, I, draw_weights(rng, I.shape[1]), forms=("host", "packed"), E=1)


def test_300_primers_more_than_one_block_of_the_update(m, eng):
    g = m.synth.aligned_genomes(12, 3000, seed=21)
    rng = np.random.default_rng(21)
    fwd, rev = (x[:150] for x in primer_sets(rng, g, 150, 13))
    assert (len(fwd) + len(rev)) == 300
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    w = draw_weights(rng, I.shape[1])
    thin_check(eng, g, opt, fwd, rev, I, w)
    thin_check(eng, g, opt, fwd, rev, I, w, 3, rng.random(300) < 0.03, forms=("packed",))


def test_more_than_two_batches_of_rounds(m, eng):
    rng = np.random.default_rng(5)
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(6, 2000))].copy()   # unrelated rows
    opt = m.KmerOpt(400, 200, 50, 13, 0, 0)
    fwd = [bytes(g[r, j * 200 + 5:j * 200 + 18]).decode() for r in range(6) for j in range(9)]   # one per segment
    I = tm.incidence(g, 400, 200, 50, 13, fwd, [], 0, 3)
    w = rng.integers(1, 1000, size=I.shape[1])
    want = thin_check(eng, g, opt, fwd, [], I, w, M=0)
    assert len(want["order"]) >= 40 and eng.info("panel_thin_rounds") == len(want["order"]) + 1 > 32
    assert (np.diff(want["gains"].astype(np.int64)) <= 0).all() and len(set(want["gains"].tolist())) > 20


def test_a_pick_that_touches_more_groups_than_the_update_grid(m, eng):
    """300 primers make the update's grid 2 x 1,024; 1,100 identical rows of 50 partitions are 55,000 segments in 1,038
    groups, and a primer that matches in one partition matches there in every row: its pick touches every group.  The
    incidence of identical rows is one row's, tiled."""
    one = m.synth.aligned_genomes(1, 8730, seed=31)
    g = np.repeat(one, 1100, axis=0)
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    P = tm.n_partitions(8730, 400, 170)
    assert P == 50
    rng = np.random.default_rng(31)
    fwd, rev = (x[:150] for x in primer_sets(rng, one, 150, 13))
    I = np.tile(tm.incidence(one, 400, 170, 50, 13, fwd, rev, 1, 3), (1, 1100))
    w = rng.choice([0, 1, 2, 5, 40000], size=I.shape[1], p=[0.2, 0.4, 0.2, 0.19, 0.01])
    want = thin_check(eng, g, opt, fwd, rev, I, w, M=1, forms=("packed",))
    assert eng.info("panel_thin_groups") == 1038 > 1024
    first = I[int(want["order"][0])]
    assert len({s // 53 for s in np.flatnonzero(first)}) > 1024


def test_a_total_of_exactly_2_to_the_32_minus_1(m, eng, grid13):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    every = np.flatnonzero(I.any(axis=0))
    w = np.ones(130, dtype=np.int64)
    a, b = int(every[0]), int(every[-1])
    w[a] = 2 ** 31 - 1
    w[b] = 2 ** 32 - 1 - w[a] - 128
    assert int(w.sum()) == 2 ** 32 - 1
    want = thin_check(eng, g, opt, fwd, rev, I, w, forms=("host", "packed"))
    assert int(want["gains"][0]) >= 2 ** 31 - 1 and want["weight_all"] > 2 ** 32 - 1 - 130
    both = np.flatnonzero(I[:, a] & I[:, b])            # one primer on both large segments, where there is one
    assert both.size == 0 or int(want["gains"][0]) >= 2 ** 32 - 1 - 128
    w[every[1]] += 1
    for form in ("host", "dev", "packed"):
        with pytest.raises(m.MsspeError) as e:
            eng.panel_thin_weighted(g, opt, fwd, rev, 2, 3, w, form=form)
        assert e.value.code == 1 and "4294967296" in str(e.value) and "4294967295" in str(e.value)
    with pytest.raises(m.MsspeError) as e:
        eng.panel_select_weighted(g, opt, fwd, rev, m.seed_rule(2, 3), w, None, form="packed")
    assert e.value.code == 1 and "4294967296" in str(e.value) and "4294967295" in str(e.value)


def test_zero_weights(m, eng, grid13):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    plain = tm.greedy(I)
    first = int(plain[1][0])
    w = np.random.default_rng(8).integers(1, 50, size=130)
    w[I[first]] = 0                                     # the unweighted first pick's segments all weigh 0
    top = int(wm.greedy_weighted(I, w)["order"][0])
    w[np.flatnonzero(I[top])[0]] = 0                    # and one segment of the weighted first pick, which stays a pick
    want = thin_check(eng, g, opt, fwd, rev, I, w, forms=("host", "packed"))
    assert top in want["order"].tolist()
    assert first not in want["order"].tolist() and (want["gains"] > 0).all()
    got = thin_dict(eng.panel_thin_weighted(g, opt, fwd, rev, 2, 3, w))
    keep = got["keep"]
    kf = [x for x, q in zip(fwd, keep[:len(fwd)]) if q]
    kr = [x for x, q in zip(rev, keep[len(fwd):]) if q]
    kept_cov = eng.segment_coverage_mm(g, opt, kf, kr, 2, 3).reshape(-1) != 255
    whole = eng.segment_coverage_mm(g, opt, fwd, rev, 2, 3).reshape(-1) != 255
    np.testing.assert_array_equal(got["covered"].reshape(-1) == 1, kept_cov)      # the kept set's real coverage
    assert got["weight_kept"] == int(w[kept_cov].sum()) == int(w[whole].sum()) == got["weight_all"]
    assert got["covered_kept"] == int(kept_cov.sum()) <= got["covered_all"] == int(whole.sum())
    assert (kept_cov & (w == 0)).any()                  # a zero segment is marked where a pick happens to cover it
    zero = thin_dict(eng.panel_thin_weighted(g, opt, fwd, rev, 2, 3, np.zeros(130, dtype=np.uint32)))
    assert zero["order"].size == 0 and zero["weight_all"] == 0 and zero["covered_all"] == plain[4]


@pytest.mark.parametrize("min_gain", [1, 2, 500])
def test_forced_primers_and_min_gain_in_weight_units(m, eng, grid13, min_gain):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    rng = np.random.default_rng(min_gain)
    w = draw_weights(rng, 130)
    want = thin_check(eng, g, opt, fwd, rev, I, w, min_gain)
    assert (want["gains"] >= min_gain).all()
    forced = rng.random(130) < 0.06
    thin_check(eng, g, opt, fwd, rev, I, w, min_gain, forced, forms=("host", "packed"))
    every = np.ones(130, dtype=np.uint8)
    want = thin_check(eng, g, opt, fwd, rev, I, w, min_gain, every)
    assert want["order"].size == 0 and want["weight_kept"] == want["weight_all"]
    some = np.zeros(130, dtype=np.uint8)
    some[wm.greedy_weighted(I, w)["order"][:3]] = 1     # the first picks forced: the rest goes on from there
    thin_check(eng, g, opt, fwd, rev, I, w, min_gain, some)


def test_a_second_call_of_another_size_on_the_same_context(m, eng):
    """The buffers grow and are kept; the weight plane is rewritten by every call."""
    cases = []
    for n_seq, L, seed in ((10, 2950, 1), (4, 2440, 2)):
        g = m.synth.aligned_genomes(n_seq, L, seed=seed)
        rng = np.random.default_rng(seed)
        fwd, rev = primer_sets(rng, g, 30 - 5 * seed, 13)
        I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
        cases.append((g, fwd, rev, I, draw_weights(rng, I.shape[1]), draw_weights(rng, I.shape[1])))
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    for i in (0, 1, 0, 1):
        g, fwd, rev, I, w1, w2 = cases[i]
        thin_check(eng, g, opt, fwd, rev, I, w1)
        thin_check(eng, g, opt, fwd, rev, I, w2, forms=("packed",))   # the same shape, other weights
        n = len(fwd) + len(rev)
        select_check(m, eng, g, opt, fwd, rev, I, np.zeros((n, n), dtype=bool), w1, 2, forms=("packed",))


# ---- the selection ------------------------------------------------------------------------------------------------
def planted(n, density, seed=5, self_loops=True):
    B = np.random.default_rng(seed).random((n, n)) < density
    if not self_loops:
        B[np.arange(n), np.arange(n)] = False
    return B


def test_selection_with_all_ones_equals_the_unweighted_call(m, eng, grid13):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    bits = sm.pack_bitmap(planted(130, 0.05))
    ones = np.ones(130, dtype=np.uint32)
    for form in ("dev", "packed"):
        for T in (1, 3):
            plain = eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), bits, T, form=form)
            rounds = eng.info("panel_select_rounds")
            got = eng.panel_select_weighted(g, opt, fwd, rev, m.seed_rule(2, 3), ones, bits, T, form=form)
            for key, v in plain.items():
                np.testing.assert_array_equal(got[key], v, key)
            assert (got["weight_all"], got["weight_kept"]) == (plain["covered_all"], plain["covered_kept"])
            assert eng.info("panel_select_rounds") == rounds


def test_a_zero_graph_is_the_weighted_thinning(m, eng, grid13):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    rng = np.random.default_rng(3)
    w = draw_weights(rng, 130)
    for forced in (None, rng.random(130) < 0.06):
        thin = thin_dict(eng.panel_thin_weighted(g, opt, fwd, rev, 2, 3, w, 1, forced, "packed"))
        for T in (1, 7, 64):
            got = eng.panel_select_weighted(g, opt, fwd, rev, m.seed_rule(2, 3), w, None, T, forced=forced,
                                            form="packed")
            for key in THIN_KEYS + ("covered",) + COUNTS:
                np.testing.assert_array_equal(got[key], thin[key], key)
            assert got["tubes_used"] == 1 and not got["barred"].any()


@pytest.mark.parametrize("T", [1, 3])
def test_a_complete_graph_keeps_the_first_picks_of_the_weighted_thinning(m, eng, grid13, T):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    w = draw_weights(np.random.default_rng(4), 130)
    want = select_check(m, eng, g, opt, fwd, rev, I, ~np.eye(130, dtype=bool), w, T, forms=("dev", "packed"))
    thin = wm.greedy_weighted(I, w)
    k = min(T, len(thin["order"]))
    np.testing.assert_array_equal(want["order"], thin["order"][:k])
    np.testing.assert_array_equal(want["gains"], thin["gains"][:k])


@pytest.mark.parametrize("T", [1, 2, 8])
def test_random_graphs(m, eng, grid13, T):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    rng = np.random.default_rng(T)
    w = draw_weights(rng, 130)
    for density in (0.03, 0.15):
        B = planted(130, density, seed=T)
        select_check(m, eng, g, opt, fwd, rev, I, B, w, T, forms=("dev", "packed"))
    select_check(m, eng, g, opt, fwd, rev, I, B, w, T, 3, rng.random(130) < 0.05, drop=True, forms=("packed",))


def test_the_weights_decide_which_segment_a_conflict_costs(m, eng):
    """Two primers in conflict, each alone on one segment: the heavier segment is kept, whichever it is."""
    rng = np.random.default_rng(77)
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(4, 1400))].copy()
    opt = m.KmerOpt(400, 200, 50, 13, 0, 0)
    P = tm.n_partitions(1400, 400, 200)
    a = bytes(g[0, 200 + 7:200 + 20]).decode()          # row 0, partition 1
    b = bytes(g[2, 600 + 9:600 + 22]).decode()          # row 2, partition 3
    I = tm.incidence(g, 400, 200, 50, 13, [a, b], [], 0, 3)
    sa, sb = 0 * P + 1, 2 * P + 3
    assert I.sum() == 2 and I[0, sa] and I[1, sb]
    B = np.array([[0, 1], [0, 0]], dtype=bool)
    for wa, wb, kept in ((1, 1, 0), (1, 9, 1), (9, 1, 0), (0, 1, 1)):
        w = np.ones(I.shape[1], dtype=np.int64)
        w[sa], w[sb] = wa, wb
        want = select_check(m, eng, g, opt, [a, b], [], I, B, w, rule=m.seed_rule(0, 3), forms=("dev", "packed"))
        assert want["order"].tolist() == [kept] and want["barred"].tolist() == [kept, 1 - kept]
        assert want["weight_kept"] == (wa, wb)[kept] and want["weight_all"] == wa + wb


@pytest.mark.parametrize("mode", ["any", "end1"])
def test_the_held_rule_against_the_model(m, eng, oracle, oracle_tables, mode):
    g = m.synth.aligned_genomes(10, 2600, seed=53)
    rng = np.random.default_rng(1302)
    fwd, rev = distinct_sets(rng, g, 30, 30, 13)
    chem = m.Chem.ntthal()
    res = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, 13, fwd, rev, 2, 3, mode, 30.0, oracle.ntthal_args())
    H = ttm.held_incidence(res)
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    assert 0 < H.sum() <= I.sum()
    w = draw_weights(rng, H.shape[1])
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    rule = m.seed_rule(2, 3, mode, chem, 30.0)
    for T in (1, 2):
        select_check(m, eng, g, opt, fwd, rev, H, planted(60, 0.05, seed=T), w, T, rule=rule, forms=("dev", "packed"))


def test_the_call_that_screens_itself_under_a_rule(m, eng, grid13):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem = m.Chem.ntthal()
    w = draw_weights(np.random.default_rng(12), 130)
    for dg, end_tm in ((-9000.0, None), (-9000.0, 20.0)):
        rule = m.ConflictRule.of(dg, end_tm)
        B = sm.unpack_bitmap(eng.conflict_graph(fwd + rev, chem, rule)["bitmap"], 130)
        assert 0 < B.sum() < 130 * 130
        for T in (1, 3):
            want = wm.select_weighted(I, B, w, T)
            got = eng.panel_select_weighted(g, opt, fwd, rev, m.seed_rule(2, 3), w, None, T, form="screen", chem=chem,
                                            threshold=dg, end_tm_threshold=end_tm)
            agree(got, want, f"{end_tm} {T}", THIN_KEYS + ("tube", "barred"))
            sm.check_independent(got, B)


def test_the_call_that_screens_itself_under_the_end_rule_alone(m, eng, grid13):
    """threshold None, end_tm_threshold set: the binding documents it, and built a c_float(None) before it looked at the
    rule (found when the third session campaign began to draw the three shapes of the rule)."""
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem = m.Chem.ntthal()
    w = draw_weights(np.random.default_rng(12), 130)
    B = sm.unpack_bitmap(eng.conflict_graph(fwd + rev, chem, m.ConflictRule.of(None, 20.0))["bitmap"], 130)
    assert 0 < B.sum() < 130 * 130
    want = wm.select_weighted(I, B, w, 3)
    got = eng.panel_select_weighted(g, opt, fwd, rev, m.seed_rule(2, 3), w, None, 3, form="screen", chem=chem,
                                    threshold=None, end_tm_threshold=20.0)
    agree(got, want, "END alone", THIN_KEYS + ("tube", "barred"))
    sm.check_independent(got, B)
    with pytest.raises(ValueError):                 # no rule at all has no unweighted form to fall to
        eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), None, 3, form="screen", chem=chem, threshold=None)


def test_argument_errors(m, eng, grid13):
    g, fwd, rev, I = grid13
    L = m.load_library()
    opt, mm, thin = m.KmerOpt(400, 170, 50, 13, 0, 0), m.MismatchOpt(2, 3), m.ThinOpt(1)
    f, r = m.pack_oligos(fwd), m.pack_oligos(rev)
    keep, tube = np.zeros(130, np.uint8), np.zeros(130, np.uint8)
    order, gains, picked = np.zeros(130, np.uint32), np.zeros(130, np.uint32), C.c_int(-1)
    w = np.ones(130, dtype=np.uint32)
    w_all = C.c_uint64(7)

    def thin_call(wp=w.ctypes.data, th=thin, k=keep.ctypes.data, mmo=mm, o=opt):
        return L.msspe_panel_thin_weighted(eng.ptr, g.ctypes.data, g.shape[0], g.shape[1], C.byref(o), C.byref(mmo),
                                           C.byref(th) if th is not None else None, f.ctypes.data, len(f), r.ctypes.data,
                                           len(r), None, wp, k, order.ctypes.data, gains.ctypes.data, C.byref(picked),
                                           None, None, None, C.byref(w_all), None)

    assert thin_call() == 0 and picked.value == 10 and w_all.value == 77
    assert thin_call(wp=None) == 1 and "weights" in L.msspe_last_error(eng.ptr).decode() and w_all.value == 0
    assert thin_call(th=None) == 1
    assert thin_call(th=m.ThinOpt(0)) == 1
    assert thin_call(k=None) == 1
    assert thin_call(mmo=m.MismatchOpt(14, 3)) == 1
    assert thin_call(o=m.KmerOpt(400, 170, 50, 32, 0, 0)) == 2
    assert thin_call(o=m.KmerOpt(400, 0, 50, 13, 0, 0)) == 1        # stride < 1: before the weights are summed
    head = (None, 2, 600, C.byref(opt), C.byref(mm), C.byref(thin), f.ctypes.data, 1, r.ctypes.data, 1, None,
            w.ctypes.data, keep.ctypes.data, order.ctypes.data, gains.ctypes.data, C.byref(picked), None, None, None,
            None, None)
    for name in ("msspe_panel_thin_weighted", "msspe_panel_thin_weighted_dev", "msspe_panel_thin_weighted_packed_dev"):
        assert getattr(L, name)(eng.ptr, *head) == 1, name             # null sequences
        assert getattr(L, name)(None, *head) == 1, name
    for bad in ({"weights": None}, {"max_tubes": 0}, {"max_tubes": 65}, {"min_gain": 0}):
        kw = {"weights": w, "max_tubes": 1, "min_gain": 1, **bad}
        for form in ("dev", "packed", "screen"):
            if kw["weights"] is None:
                rule, sel, chem, cr = m.seed_rule(2, 3), m.SelectOpt(1, 1, 0), m.Chem.ntthal(), m.ConflictRule.of()
                d = C.c_void_p()
                eng._check(L.msspe_device_put(eng.ptr, g.ctypes.data, g.size, C.byref(d)))
                bits = C.c_void_p()
                zero = np.zeros((130, 3), dtype=np.uint64)
                eng._check(L.msspe_device_put(eng.ptr, zero.ctypes.data, zero.nbytes, C.byref(bits)))
                try:
                    tail = (None, keep.ctypes.data, order.ctypes.data, gains.ctypes.data, C.byref(picked),
                            tube.ctypes.data, None, None, None, None, None, None, None)
                    ins = (g.shape[0], g.shape[1], C.byref(opt), C.byref(rule), C.byref(sel), f.ctypes.data, len(f),
                           r.ctypes.data, len(r), None)
                    assert L.msspe_panel_select_weighted_dev(eng.ptr, d, *ins, bits, *tail) == 1
                    assert "weights" in L.msspe_last_error(eng.ptr).decode()
                    assert L.msspe_panel_select_weighted_rule(eng.ptr, g.ctypes.data, *ins, C.byref(chem), C.byref(cr),
                                                              *tail) == 1
                    assert "weights" in L.msspe_last_error(eng.ptr).decode()
                    assert L.msspe_panel_select_weighted_rule(eng.ptr, g.ctypes.data, *ins, C.byref(chem), None,
                                                              w.ctypes.data, *tail[1:]) == 1
                finally:
                    eng.device_free(int(d.value))
                    eng.device_free(int(bits.value))
                break
            with pytest.raises(m.MsspeError) as e:
                eng.panel_select_weighted(g, opt, fwd, rev, m.seed_rule(2, 3), kw["weights"], None, kw["max_tubes"],
                                          kw["min_gain"], form=form)
            assert e.value.code == 1
    with pytest.raises(ValueError):
        eng.panel_thin_weighted(g, opt, fwd, rev, 2, 3, np.ones(129))
    with pytest.raises(ValueError):
        eng.panel_thin_weighted(g, opt, fwd, rev, 2, 3, -np.ones(130))
