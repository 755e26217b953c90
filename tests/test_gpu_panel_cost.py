"""msspe_panel_thin_cost* and msspe_panel_select_cost* on the device against the model (tests/panel_cost_model.py):
order, gains, keep, covered, both counts, both weights, both costs, tubes, barred and rounds, exactly.  Equal costs
against the four siblings in every form, random costs and weights at every group boundary, pool sizes around the pick's
strides, planted ties of both levels inside one thread's stride, in two lanes and in two waves, the built cases and the
case only an exact comparison decides, 54 picks over four batches of rounds, no weights, forced primers and min_gain, the
selection's identities and graphs, the held rule, the call that screens itself, the guarantee through the existing
coverage call, calls of different sizes on one context, and the argument errors."""
import ctypes as C

import numpy as np
import pytest

import coverage_thal_model as ctm
import panel_cost_model as cm
import panel_select_model as sm
import panel_thin_model as tm
import panel_thin_thal_model as ttm
import panel_weighted_model as wm
from test_coverage_mm_model import draw_primers, rc
from test_panel_cost_model import case_below_min_gain, case_cheap_primers, draw_costs
from test_panel_thin_model import grid_case

pytestmark = pytest.mark.gpu
THIN_KEYS = ("order", "gains", "keep")
COUNTS = ("covered_all", "covered_kept", "weight_all", "weight_kept", "cost_all", "cost_kept")
K = 13


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
    w = rng.choice([0, 1, 1, 2, 3, 7], size=n_seg).astype(np.int64)
    big = rng.random(n_seg) < 0.05
    w[big] = rng.integers(1000, 2_000_000, size=int(big.sum()))
    return w


def primer_sets(rng, g, n_f, n_r, k=K):
    return draw_primers(rng, g, n_f, k), [rc(w) for w in draw_primers(rng, g, n_r, k)]


SEG = 100   # the planted alignments: a row is one segment of 100 bases, searched whole


def planted(I, seed=0):
    """An alignment and forward primers whose incidence at M = 0 is exactly I: a row of random bases per segment, a
    random word per primer written into every row it is to match in.  A chance match elsewhere (one in 4^13 per place)
    is met by drawing again."""
    I = np.asarray(I, dtype=bool)
    n, n_seg = I.shape
    for attempt in range(50):
        rng = np.random.default_rng(seed + 1000 * attempt)
        g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n_seg, SEG))].copy()
        used = np.zeros((n_seg, SEG // K), dtype=bool)
        words = []
        for p in range(n):
            rows = np.flatnonzero(I[p])
            slot = int(np.flatnonzero(~used[rows].any(axis=0))[0])      # free in every row of the primer
            used[rows, slot] = True
            w = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=K)]
            g[rows, slot * K:(slot + 1) * K] = w
            words.append(bytes(w).decode())
        if len(set(words)) == n and np.array_equal(tm.incidence(g, SEG, 170, SEG, K, words, [], 0, 3), I):
            return g, words
    raise AssertionError("no alignment with this incidence in 50 draws")


def planted_opt(m):
    return m.KmerOpt(SEG, 170, SEG, K, 0, 0)


def thin_dict(got):
    keys = ("keep", "order", "gains", "covered", "covered_all", "covered_kept", "weight_all", "weight_kept", "cost_all",
            "cost_kept")
    return dict(zip(keys, got))


def agree(got, want, what="", keys=THIN_KEYS):
    for key in keys:
        np.testing.assert_array_equal(got[key], want[key], f"{key} {what}")
    np.testing.assert_array_equal(got["covered"].reshape(-1), want["covered"].astype(np.uint8), f"covered {what}")
    for key in COUNTS:
        assert got[key] == want[key], f"{key} {what}"


def thin_check(eng, g, opt, fwd, rev, I, costs, w=None, min_gain=1, forced=None, forms=("host",), M=2, E=3):
    want = cm.greedy_cost(I, costs, w, min_gain, forced)
    for form in forms:
        got = thin_dict(eng.panel_thin_cost(g, opt, fwd, rev, M, E, costs, w, min_gain, forced, form))
        agree(got, want, form)
        if I.size:
            assert eng.info("panel_thin_rounds") == want["rounds"], form
    if min_gain == 1:                                   # guarantee 2
        assert want["weight_kept"] == want["weight_all"]
        assert w is not None or want["covered_kept"] == want["covered_all"]
    return want


def select_check(m, eng, g, opt, fwd, rev, I, B, costs, w=None, T=1, min_gain=1, forced=None, drop=False,
                 forms=("dev",), rule=None):
    want = cm.select_cost(I, B, costs, w, T, min_gain, forced, drop)
    sm.check_independent(want, B, forced, drop)         # guarantee 3
    for form in forms:
        got = eng.panel_select_cost(g, opt, fwd, rev, rule or m.seed_rule(2, 3), costs, w, sm.pack_bitmap(B), T,
                                    min_gain, drop, forced, form)
        agree(got, want, form, THIN_KEYS + ("tube", "barred"))
        assert got["tubes_used"] == want["tubes_used"], form
        if I.size:
            assert eng.info("panel_select_rounds") == want["rounds"], form
    return want


# ---- guarantee 1: equal costs against the four siblings ----------------------------------------------------------
@pytest.mark.parametrize("c", [1, 7])
def test_equal_costs_equal_the_thinning_siblings_in_the_three_forms(m, eng, grid13, c):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    costs = np.full(130, c, dtype=np.uint32)
    w = draw_weights(np.random.default_rng(c), 130)
    forced = np.random.default_rng(15).random(130) < 0.06
    for form in ("host", "dev", "packed"):
        for min_gain, f in ((1, None), (2, forced)):
            plain = eng.panel_thin(g, opt, fwd, rev, 2, 3, min_gain, f, form)
            rounds = eng.info("panel_thin_rounds")
            got = eng.panel_thin_cost(g, opt, fwd, rev, 2, 3, costs, None, min_gain, f, form)
            for a, b in zip(got[:6], plain):
                np.testing.assert_array_equal(a, b, form)
            assert got[6:8] == plain[4:6] and eng.info("panel_thin_rounds") == rounds
            assert got[8] == 130 * c and got[9] == c * int(got[0].sum())
            sib = eng.panel_thin_weighted(g, opt, fwd, rev, 2, 3, w, min_gain, f, form)
            rounds = eng.info("panel_thin_rounds")
            got = eng.panel_thin_cost(g, opt, fwd, rev, 2, 3, costs, w, min_gain, f, form)
            for a, b in zip(got[:8], sib):
                np.testing.assert_array_equal(a, b, form)
            assert eng.info("panel_thin_rounds") == rounds


@pytest.mark.parametrize("c", [1, 7])
def test_equal_costs_equal_the_selection_siblings_in_the_three_forms(m, eng, grid13, c):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    costs = np.full(130, c, dtype=np.uint32)
    w = draw_weights(np.random.default_rng(c), 130)
    bits = sm.pack_bitmap(np.random.default_rng(5).random((130, 130)) < 0.05)
    chem = m.Chem.ntthal()
    for form, graph in (("dev", {"bitmap": bits}), ("packed", {"bitmap": bits}),
                        ("screen", {"chem": chem, "threshold": -9000.0, "end_tm_threshold": 20.0})):
        for T in (1, 3):
            plain = eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), max_tubes=T, form=form, **graph)
            rounds = eng.info("panel_select_rounds")
            got = eng.panel_select_cost(g, opt, fwd, rev, m.seed_rule(2, 3), costs, None, max_tubes=T, form=form, **graph)
            for key, v in plain.items():
                np.testing.assert_array_equal(got[key], v, key)
            assert (got["weight_all"], got["weight_kept"]) == (plain["covered_all"], plain["covered_kept"])
            assert eng.info("panel_select_rounds") == rounds
            assert got["cost_all"] == 130 * c and got["cost_kept"] == c * int(got["keep"].sum())
            sib = eng.panel_select_weighted(g, opt, fwd, rev, m.seed_rule(2, 3), w, max_tubes=T, form=form, **graph)
            rounds = eng.info("panel_select_rounds")
            got = eng.panel_select_cost(g, opt, fwd, rev, m.seed_rule(2, 3), costs, w, max_tubes=T, form=form, **graph)
            for key, v in sib.items():
                np.testing.assert_array_equal(got[key], v, key)
            assert eng.info("panel_select_rounds") == rounds


# ---- the thinning -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_seq,L,n_seg", [(1, 400, 1), (4, 2440, 52), (53, 450, 53), (6, 1760, 54), (107, 500, 107),
                                           (10, 2950, 160)])
def test_random_costs_and_weights_at_the_group_boundaries(m, eng, n_seq, L, n_seg):
    g = m.synth.aligned_genomes(n_seq, L, seed=n_seg)
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    assert n_seq * tm.n_partitions(L, 400, 170) == n_seg
    rng = np.random.default_rng(n_seg)
    fwd, rev = primer_sets(rng, g, 30, 30)
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    costs = draw_costs(rng, len(fwd) + len(rev))
    thin_check(eng, g, opt, fwd, rev, I, costs, draw_weights(rng, n_seg), forms=("host", "packed"))
    thin_check(eng, g, opt, fwd, rev, I, costs, None, forms=("dev",))


@pytest.fixture(scope="module")
def pool300(m):
    """300 primers on 12 genomes and their incidence, computed once; the smaller pools are its prefixes."""
    g = m.synth.aligned_genomes(12, 3000, seed=21)
    rng = np.random.default_rng(21)
    words = list(dict.fromkeys(draw_primers(rng, g, 330, K)))[:300]        # distinct: the selection's graph needs that
    assert len(words) == 300 and not {rc(x) for x in words} & set(words)
    I = tm.incidence(g, 400, 170, 50, K, words, [], 2, 3)
    I.setflags(write=False)
    return g, words, I


@pytest.mark.parametrize("n", [63, 64, 65, 129, 255, 256, 257, 300])
def test_pool_sizes_around_the_strides_of_the_pick(m, eng, pool300, n):
    g, words, I = pool300
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    rng = np.random.default_rng(n)
    n_f = (n + 1) // 2                                  # an odd pool: the lists differ in length
    fwd, rev = words[:n_f], [rc(x) for x in words[n_f:n]]
    Ir = tm.incidence(g, 400, 170, 50, K, [], rev, 2, 3)
    In = np.vstack([I[:n_f], Ir])
    costs, w = draw_costs(rng, n), draw_weights(rng, In.shape[1])
    thin_check(eng, g, opt, fwd, rev, In, costs, w, forms=("packed",))
    B = np.random.default_rng(n + 1).random((n, n)) < 0.03
    select_check(m, eng, g, opt, fwd, rev, In, B, costs, w, 2, forms=("packed",))


@pytest.fixture(scope="module")
def diagonal520():
    """520 primers, each alone on its own segment: a gain is the segment's weight and stays what it is."""
    return planted(np.eye(520, dtype=bool), seed=520)


BIG = (16777219, 16777223, 16777227)   # c and 3 c are past 2^24: binary32 rounds c up and 3 c down, so 3 c / c < 3


def tie_plan():
    """(costs, weights) of the diagonal case: everyone at 1 / 1000 but two groups of contenders.  Group A has the ratio
    3 with different gains (equal products: the greater gain wins), group B the ratio 2 in equal pairs (all equal: the
    lowest index wins); each group has a pair inside one thread's stride (p, p + 256), in two lanes of one wave, and in
    two waves.  One contender of each pair of group A is (3 c, c) with c in BIG: a pick that divides in binary32 ranks
    it below its partner."""
    w = np.ones(520, dtype=np.int64)
    costs = np.full(520, 1000, dtype=np.int64)
    a = {5: (3, 1), 261: (3 * BIG[1], BIG[1]), 12: (9, 3), 40: (3 * BIG[2], BIG[2]), 100: (15, 5),
         230: (3 * BIG[0], BIG[0])}
    b = {7: (4, 2), 263: (4, 2), 14: (8, 4), 50: (8, 4), 70: (16, 8), 200: (16, 8)}
    for p, (gain, cost) in {**a, **b}.items():
        w[p], costs[p] = gain, cost
    for c in BIG:
        assert np.float32(3 * c) / np.float32(c) < np.float32(3)
    return costs, w


def test_planted_ties_in_a_stride_in_two_lanes_and_in_two_waves(m, eng, diagonal520):
    g, words = diagonal520
    I = np.eye(520, dtype=bool)
    costs, w = tie_plan()
    want = thin_check(eng, g, planted_opt(m), words, [], I, costs, w, forms=("packed",), M=0)
    assert want["order"][:12].tolist() == [40, 261, 230, 100, 12, 5, 70, 200, 14, 50, 7, 263]
    assert want["order"][12:].tolist() == [p for p in range(520) if costs[p] == 1000]
    B = np.zeros((520, 520), dtype=bool)
    B[230, 100] = B[70, 200] = True                     # a barred contender leaves the tie to the next one
    sel = select_check(m, eng, g, planted_opt(m), words, [], I, B, costs, w, forms=("packed",),
                       rule=m.seed_rule(0, 3))
    assert sel["order"][:10].tolist() == [40, 261, 230, 12, 5, 70, 14, 50, 7, 263]


def test_the_built_cases(m, eng):
    I, costs = case_cheap_primers()
    g, words = planted(I, seed=1)
    want = thin_check(eng, g, planted_opt(m), words, [], I, costs, forms=("dev",), M=0)
    assert want["order"].tolist() == [1, 2, 3] and (want["cost_kept"], want["cost_all"]) == (6, 13)
    assert eng.panel_thin(g, planted_opt(m), words, [], 0, 3, form="dev")[1].tolist() == [0]
    I, costs, min_gain = case_below_min_gain()
    g, words = planted(I, seed=2)
    want = thin_check(eng, g, planted_opt(m), words, [], I, costs, None, min_gain, forms=("dev",), M=0)
    assert want["order"].tolist() == [1, 2] and want["rounds"] == 3
    want = select_check(m, eng, g, planted_opt(m), words, [], I, np.zeros((3, 3), dtype=bool), costs, None, 1, min_gain,
                        rule=m.seed_rule(0, 3))
    assert want["order"].tolist() == [1, 2]
    I = np.zeros((3, 6), dtype=bool)
    I[0, :2] = I[1, 2:4] = I[2, 4:] = True
    g, words = planted(I, seed=3)
    assert thin_check(eng, g, planted_opt(m), words, [], I, [3, 3, 3], forms=("dev",), M=0)["order"].tolist() == [0, 1, 2]
    I = np.zeros((2, 6), dtype=bool)
    I[0, :2] = I[1, 2:] = True
    g, words = planted(I, seed=4)
    assert thin_check(eng, g, planted_opt(m), words, [], I, [1, 2], forms=("dev",), M=0)["order"].tolist() == [1, 0]


def test_only_the_exact_comparison_decides(m, eng):
    """The cross products differ by 1 in 2^64; the quotients are equal in binary64 and binary32.  The weights' total is
    2^32 - 1 exactly."""
    g, words = planted(cm.EXACT_I, seed=9)
    assert sum(cm.EXACT_W) == 2 ** 32 - 1
    for form in ("host", "dev", "packed"):
        want = thin_check(eng, g, planted_opt(m), words, [], cm.EXACT_I, cm.EXACT_COSTS, cm.EXACT_W, forms=(form,), M=0)
        assert want["order"].tolist() == [1, 0] and want["gains"].tolist() == [2 ** 32 - 2, 1]
    want = select_check(m, eng, g, planted_opt(m), words, [], cm.EXACT_I, np.zeros((2, 2), dtype=bool), cm.EXACT_COSTS,
                        cm.EXACT_W, forms=("dev", "packed"), rule=m.seed_rule(0, 3))
    assert want["order"].tolist() == [1, 0] and want["cost_kept"] == 2 ** 33 - 5


def test_54_picks_over_four_batches_of_rounds(m, eng):
    I = np.eye(54, dtype=bool)
    g, words = planted(I, seed=54)
    rng = np.random.default_rng(54)
    costs, w = draw_costs(rng, 54), rng.integers(1, 1000, size=54)
    want = thin_check(eng, g, planted_opt(m), words, [], I, costs, w, forms=("dev",), M=0)
    assert len(want["order"]) == 54 and eng.info("panel_thin_rounds") == 55 > 3 * 16
    want = select_check(m, eng, g, planted_opt(m), words, [], I, np.zeros((54, 54), dtype=bool), costs, w,
                        rule=m.seed_rule(0, 3))
    assert len(want["order"]) == 54 and want["rounds"] == 55


def test_without_weights(m, eng, grid13):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    costs = draw_costs(np.random.default_rng(2), 130)
    want = thin_check(eng, g, opt, fwd, rev, I, costs, None, forms=("host", "dev", "packed"))
    assert (want["weight_all"], want["weight_kept"]) == (want["covered_all"], want["covered_kept"])
    assert want["order"].tolist() != tm.greedy(I)[1].tolist()            # the costs do change the order here
    B = np.random.default_rng(3).random((130, 130)) < 0.05
    select_check(m, eng, g, opt, fwd, rev, I, B, costs, None, 2, forms=("dev", "packed"))


@pytest.mark.parametrize("min_gain", [1, 2, 500])
def test_forced_primers_and_min_gain(m, eng, grid13, min_gain):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    rng = np.random.default_rng(min_gain)
    costs, w = draw_costs(rng, 130), draw_weights(rng, 130)
    want = thin_check(eng, g, opt, fwd, rev, I, costs, w, min_gain)
    assert (want["gains"] >= min_gain).all()
    forced = rng.random(130) < 0.06
    want = thin_check(eng, g, opt, fwd, rev, I, costs, w, min_gain, forced, forms=("host", "packed"))
    assert want["cost_kept"] >= int(costs[forced].sum())                 # forced primers count in the kept cost
    thin_check(eng, g, opt, fwd, rev, I, costs, None, min_gain, forced, forms=("packed",))
    every = np.ones(130, dtype=np.uint8)
    want = thin_check(eng, g, opt, fwd, rev, I, costs, w, min_gain, every)
    assert want["order"].size == 0 and want["cost_kept"] == want["cost_all"]
    B = np.random.default_rng(9).random((130, 130)) < 0.05
    select_check(m, eng, g, opt, fwd, rev, I, B, costs, w, 2, min_gain, forced, forms=("packed",))


def test_the_thinning_loses_nothing(m, eng, grid13):
    """Guarantee 2 through the existing coverage call: the kept subset covers what the whole set covers."""
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    rng = np.random.default_rng(6)
    costs = draw_costs(rng, 130)
    whole = eng.segment_coverage_mm(g, opt, fwd, rev, 2, 3).reshape(-1) != 255
    for w in (None, rng.integers(1, 50, size=130)):
        got = thin_dict(eng.panel_thin_cost(g, opt, fwd, rev, 2, 3, costs, w))
        kf = [x for x, q in zip(fwd, got["keep"][:len(fwd)]) if q]
        kr = [x for x, q in zip(rev, got["keep"][len(fwd):]) if q]
        kept_cov = eng.segment_coverage_mm(g, opt, kf, kr, 2, 3).reshape(-1) != 255
        np.testing.assert_array_equal(kept_cov, whole)
        np.testing.assert_array_equal(got["covered"].reshape(-1) == 1, kept_cov)
        assert got["covered_kept"] == got["covered_all"] == int(whole.sum())
        assert got["weight_kept"] == got["weight_all"] == (int(whole.sum()) if w is None else int(w[whole].sum()))
        assert got["cost_kept"] == int(costs[got["keep"] == 1].sum()) < got["cost_all"] == int(costs.sum())


# ---- the selection ------------------------------------------------------------------------------------------------
def test_a_zero_graph_is_the_cost_thinning(m, eng, grid13):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    rng = np.random.default_rng(3)
    costs, w = draw_costs(rng, 130), draw_weights(rng, 130)
    for forced in (None, rng.random(130) < 0.06):
        thin = thin_dict(eng.panel_thin_cost(g, opt, fwd, rev, 2, 3, costs, w, 1, forced, "packed"))
        for T in (1, 64):
            got = eng.panel_select_cost(g, opt, fwd, rev, m.seed_rule(2, 3), costs, w, None, T, forced=forced,
                                        form="packed")
            for key in THIN_KEYS + ("covered",) + COUNTS:
                np.testing.assert_array_equal(got[key], thin[key], key)
            assert got["tubes_used"] == 1 and not got["barred"].any()


@pytest.mark.parametrize("T", [1, 3])
def test_a_complete_graph_keeps_the_first_picks_of_the_cost_thinning(m, eng, grid13, T):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    rng = np.random.default_rng(4)
    costs, w = draw_costs(rng, 130), draw_weights(rng, 130)
    want = select_check(m, eng, g, opt, fwd, rev, I, ~np.eye(130, dtype=bool), costs, w, T, forms=("dev", "packed"))
    thin = cm.greedy_cost(I, costs, w)
    k = min(T, len(thin["order"]))
    np.testing.assert_array_equal(want["order"], thin["order"][:k])


@pytest.mark.parametrize("T", [1, 2, 8])
def test_random_graphs(m, eng, grid13, T):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    rng = np.random.default_rng(T)
    costs, w = draw_costs(rng, 130), draw_weights(rng, 130)
    for density in (0.03, 0.15):
        B = np.random.default_rng(T + 10).random((130, 130)) < density
        select_check(m, eng, g, opt, fwd, rev, I, B, costs, w, T, forms=("dev", "packed"))
    select_check(m, eng, g, opt, fwd, rev, I, B, costs, w, T, 3, rng.random(130) < 0.05, drop=True, forms=("packed",))


def test_the_held_rule_against_the_model(m, eng, oracle, oracle_tables):
    g = m.synth.aligned_genomes(10, 2600, seed=53)
    rng = np.random.default_rng(1302)
    words = list(dict.fromkeys(draw_primers(rng, g, 120, K)))
    fwd = words[:30]
    rev = [x for x in dict.fromkeys(rc(y) for y in words[30:]) if x not in set(fwd)][:30]
    assert len(set(fwd + rev)) == 60
    chem = m.Chem.ntthal()
    res = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, 13, fwd, rev, 2, 3, "any", 30.0, oracle.ntthal_args())
    H = ttm.held_incidence(res)
    assert 0 < H.sum()
    costs, w = draw_costs(rng, 60), draw_weights(rng, H.shape[1])
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    B = np.random.default_rng(2).random((60, 60)) < 0.05
    select_check(m, eng, g, opt, fwd, rev, H, B, costs, w, 2, rule=m.seed_rule(2, 3, "any", chem, 30.0),
                 forms=("dev", "packed"))


def test_the_call_that_screens_itself_under_a_rule(m, eng, grid13):
    g, fwd, rev, I = grid13
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem = m.Chem.ntthal()
    rng = np.random.default_rng(12)
    costs, w = draw_costs(rng, 130), draw_weights(rng, 130)
    for dg, end_tm in ((-9000.0, None), (-9000.0, 20.0)):
        B = sm.unpack_bitmap(eng.conflict_graph(fwd + rev, chem, m.ConflictRule.of(dg, end_tm))["bitmap"], 130)
        assert 0 < B.sum() < 130 * 130
        for T, weights in ((1, w), (3, None)):
            want = cm.select_cost(I, B, costs, weights, T)
            got = eng.panel_select_cost(g, opt, fwd, rev, m.seed_rule(2, 3), costs, weights, None, T, form="screen",
                                        chem=chem, threshold=dg, end_tm_threshold=end_tm)
            agree(got, want, f"{end_tm} {T}", THIN_KEYS + ("tube", "barred"))
            sm.check_independent(got, B)
            assert eng.info("panel_select_rounds") == want["rounds"]


def test_calls_of_different_sizes_then_a_weighted_sibling_on_one_context(m, eng):
    """The cost slot grows and is kept; a sibling call after a cost call runs the sibling's pick."""
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    cases = []
    for n_seq, L, seed in ((10, 2950, 1), (4, 2440, 2)):
        g = m.synth.aligned_genomes(n_seq, L, seed=seed)
        rng = np.random.default_rng(seed)
        fwd, rev = primer_sets(rng, g, 30 - 5 * seed, 30 - 5 * seed)
        I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
        cases.append((g, fwd, rev, I, draw_costs(rng, len(fwd) + len(rev)), draw_weights(rng, I.shape[1])))
    for i in (1, 0, 1):
        g, fwd, rev, I, costs, w = cases[i]
        n = len(fwd) + len(rev)
        thin_check(eng, g, opt, fwd, rev, I, costs, w, forms=("packed",))
        select_check(m, eng, g, opt, fwd, rev, I, np.zeros((n, n), dtype=bool), costs, w, 2, forms=("packed",))
        want = wm.greedy_weighted(I, w)
        got = eng.panel_thin_weighted(g, opt, fwd, rev, 2, 3, w, form="packed")
        np.testing.assert_array_equal(got[1], want["order"])
        np.testing.assert_array_equal(got[2], want["gains"])
        sel = eng.panel_select_weighted(g, opt, fwd, rev, m.seed_rule(2, 3), w, None, 2, form="packed")
        np.testing.assert_array_equal(sel["order"], wm.select_weighted(I, np.zeros((n, n), dtype=bool), w, 2)["order"])


def test_argument_errors(m, eng, grid13):
    g, fwd, rev, I = grid13
    L = m.load_library()
    opt, mm, thin = m.KmerOpt(400, 170, 50, 13, 0, 0), m.MismatchOpt(2, 3), m.ThinOpt(1)
    f, r = m.pack_oligos(fwd), m.pack_oligos(rev)
    keep, tube = np.zeros(130, np.uint8), np.zeros(130, np.uint8)
    order, gains, picked = np.zeros(130, np.uint32), np.zeros(130, np.uint32), C.c_int(-1)
    costs = np.ones(130, dtype=np.uint32)
    c_all, c_kept, w_all = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)

    def thin_call(cp=costs.ctypes.data):
        return L.msspe_panel_thin_cost(eng.ptr, g.ctypes.data, g.shape[0], g.shape[1], C.byref(opt), C.byref(mm),
                                       C.byref(thin), f.ctypes.data, len(f), r.ctypes.data, len(r), None, None, cp,
                                       keep.ctypes.data, order.ctypes.data, gains.ctypes.data, C.byref(picked), None,
                                       None, None, C.byref(w_all), None, C.byref(c_all), C.byref(c_kept))

    assert thin_call() == 0 and picked.value == 10 and (w_all.value, c_all.value, c_kept.value) == (77, 130, 10)
    assert thin_call(cp=None) == 1 and "null costs" in L.msspe_last_error(eng.ptr).decode()
    assert (c_all.value, c_kept.value) == (0, 0)
    zero = costs.copy()
    zero[[41, 97]] = 0
    for form in ("host", "dev", "packed"):
        with pytest.raises(m.MsspeError) as e:
            eng.panel_thin_cost(g, opt, fwd, rev, 2, 3, zero, form=form)
        assert e.value.code == 1 and "primer 41 " in str(e.value) and "97" not in str(e.value)
    for form in ("dev", "packed", "screen"):
        with pytest.raises(m.MsspeError) as e:
            eng.panel_select_cost(g, opt, fwd, rev, m.seed_rule(2, 3), zero, form=form)
        assert e.value.code == 1 and "primer 41 " in str(e.value)
    rule, sel, chem, cr = m.seed_rule(2, 3), m.SelectOpt(1, 1, 0), m.Chem.ntthal(), m.ConflictRule.of()
    tail = (None, None, keep.ctypes.data, order.ctypes.data, gains.ctypes.data, C.byref(picked), tube.ctypes.data, None,
            None, None, None, None, None, None, None, None)
    ins = (g.shape[0], g.shape[1], C.byref(opt), C.byref(rule), C.byref(sel), f.ctypes.data, len(f), r.ctypes.data,
           len(r), None)
    assert L.msspe_panel_select_cost_rule(eng.ptr, g.ctypes.data, *ins, C.byref(chem), C.byref(cr), *tail) == 1
    assert "null costs" in L.msspe_last_error(eng.ptr).decode()
    w = np.ones(130, dtype=np.int64)
    w[0] = 2 ** 32 - 129                                # the total is 2^32
    assert int(w.sum()) == 2 ** 32
    for call in (lambda: eng.panel_thin_cost(g, opt, fwd, rev, 2, 3, costs, w),
                 lambda: eng.panel_select_cost(g, opt, fwd, rev, m.seed_rule(2, 3), costs, w, form="packed")):
        with pytest.raises(m.MsspeError) as e:
            call()
        assert e.value.code == 1 and "4294967296" in str(e.value) and "4294967295" in str(e.value)
    for bad in ({"max_tubes": 0}, {"max_tubes": 65}, {"min_gain": 0}):
        with pytest.raises(m.MsspeError) as e:
            eng.panel_select_cost(g, opt, fwd, rev, m.seed_rule(2, 3), costs, **bad)
        assert e.value.code == 1
    with pytest.raises(ValueError):
        eng.panel_thin_cost(g, opt, fwd, rev, 2, 3, np.ones(129))
    with pytest.raises(ValueError):
        eng.panel_thin_cost(g, opt, fwd, rev, 2, 3, -np.ones(130))
