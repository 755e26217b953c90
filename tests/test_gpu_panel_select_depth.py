"""msspe_panel_select_depth* on the device against the numpy model (tests/panel_select_depth_model.py): order, gains,
layers, keep, tube, barred, both depth planes, the four counts, the tubes in use, the rounds and the layers, exactly.
The grid inputs under planted graphs in the bitmap, _dev and _packed_dev forms at R = 2 and 3, R = 1 against
Engine.panel_select on the same context, the prefix property device against device, depth_kept through the existing
coverage call, the mask, bitmap and group boundaries, a self loop, a one-direction edge, forced primers with
neighbours, min_gain above 1, saturation over 255 layers and a layer that spans batches, the held incidence (END1),
the forms that screen the pool themselves, the empty inputs, the matrix cap, the depth's range, the context's shared
buffers, and the CLI's --select-depth."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import coverage_thal_model as ctm
import panel_select_depth_model as dm
import panel_select_model as sm
import panel_thin_model as tm
import panel_thin_thal_model as ttm
from test_gpu_panel_select import distinct_sets, planted, primer_sets, run_cli, small_case
from test_panel_thin_model import grid_case

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KEYS = ("order", "gains", "layer", "keep", "tube", "barred", "counts")
PLANES = ("depth_all", "depth_kept")


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
def grids():
    """(genomes, fwd, rev, incidence at M = 2, E = 3) of the two grid cases, computed once and never written."""
    out = {}
    for k in (13, 24):
        g, fwd, rev = grid_case(k, 2)
        I = tm.incidence(g, 400, 170, 50, k, fwd, rev, 2, 3)
        I.setflags(write=False)
        out[k] = (g, fwd, rev, I)
    return out


def agree(got, want, what=""):
    for key in KEYS:
        np.testing.assert_array_equal(got[key], want[key], f"{key} {what}")
    for key in PLANES:
        np.testing.assert_array_equal(got[key].reshape(-1), want[key], f"{key} {what}")
    assert got["tubes_used"] == want["tubes_used"], f"tubes_used {what}"


def check(m, eng, g, opt, fwd, rev, I, B, R, T=1, min_gain=1, forced=None, drop=False, forms=("bitmap",), M=2, E=3):
    """The device result of every form against the model over the incidence I; returns the model's result."""
    want = dm.select_depth(I, B, R, T, min_gain, forced, drop)
    sm.check_independent(want, B, forced, drop)
    bits = sm.pack_bitmap(B)
    for form in forms:
        got = eng.panel_select_depth(g, opt, fwd, rev, m.seed_rule(M, E), R, bits, T, min_gain, drop, forced, form)
        agree(got, want, form)
        if I.size:
            assert eng.info("panel_select_rounds") == want["rounds"], form
            assert eng.info("panel_select_depth_layers") == want["layers"], form
            assert eng.info("panel_select_tubes") == want["tubes_used"], form
            assert eng.info("panel_select_barred") == int(want["barred"].sum()), form
            assert eng.info("panel_select_depth_layer_us") >= 0
    return want


@pytest.mark.parametrize("k", [13, 24])
@pytest.mark.parametrize("density", [0.02, 0.1])
def test_grid_under_planted_graphs_in_the_three_forms(m, eng, grids, k, density):
    g, fwd, rev, I = grids[k]
    opt = m.KmerOpt(400, 170, 50, k, 0, 0)
    B = planted(130, density)
    for T in (1, 2, 4):
        for R in (2, 3):
            want = check(m, eng, g, opt, fwd, rev, I, B, R, T, forms=("bitmap", "dev", "packed"))
            if (k, density, T, R) == (13, 0.1, 2, 2):
                assert (len(want["order"]), want["counts"].tolist(), want["rounds"]) == (9, [77, 66, 45, 18], 11)
            if (k, density, T, R) == (13, 0.02, 2, 3):
                assert (len(want["order"]), want["counts"].tolist(), want["rounds"]) == (16, [77, 77, 8, 8], 19)
    check(m, eng, g, opt, fwd, rev, I, B, 2, 2, drop=True, forms=("packed",))


def test_depth_one_is_the_selection_on_the_same_context(m, eng, grids):
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    forced = np.random.default_rng(2).random(130) < 0.05
    for density, T, G, f in ((0.1, 1, 1, None), (0.02, 4, 1, forced), (0.1, 2, 2, forced), (0.0, 64, 1, None)):
        bits = sm.pack_bitmap(planted(130, density))
        flat = eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), bits, T, G, forced=f, form="packed")
        rounds, barred = eng.info("panel_select_rounds"), eng.info("panel_select_barred")
        one = eng.panel_select_depth(g, opt, fwd, rev, m.seed_rule(2, 3), 1, bits, T, G, forced=f, form="packed")
        for key in ("order", "gains", "keep", "tube", "barred"):
            np.testing.assert_array_equal(one[key], flat[key], key)
        assert one["tubes_used"] == flat["tubes_used"] and (one["layer"] == 1).all()
        assert one["counts"][:2].tolist() == [flat["covered_all"], flat["covered_kept"]]
        assert (eng.info("panel_select_rounds"), eng.info("panel_select_barred")) == (rounds, barred)
        assert eng.info("panel_select_depth_layers") == 1
        np.testing.assert_array_equal(one["depth_kept"] != 0, flat["covered"] != 0)


def test_prefix_device_against_device(m, eng, grids):
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    for density, T, G in ((0.1, 2, 1), (0.02, 1, 1), (0.1, 4, 2)):
        bits = sm.pack_bitmap(planted(130, density))
        runs = [eng.panel_select_depth(g, opt, fwd, rev, m.seed_rule(2, 3), R, bits, T, G, form="packed")
                for R in (1, 2, 3, 255)]
        for a, b in zip(runs, runs[1:]):
            k = len(a["order"])
            for key in ("order", "gains", "layer"):
                np.testing.assert_array_equal(b[key][:k], a[key], key)
            picks = a["order"].astype(np.int64)
            np.testing.assert_array_equal(b["tube"][picks], a["tube"][picks])
            assert b["counts"][1] >= a["counts"][1] and (G > 1 or b["counts"][1] == a["counts"][1])
        assert len(runs[1]["order"]) > len(runs[0]["order"])             # layer 2 adds something
        np.testing.assert_array_equal(runs[3]["order"], runs[2]["order"])  # D = 3


def test_depth_kept_is_what_the_kept_primers_match(m, eng, grids):
    """depth_kept against the existing coverage call, one kept primer at a time: the number of kept primers whose own
    segment_coverage_mm row is not 255."""
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    forced = np.zeros(130, dtype=np.uint8)
    forced[[3, 90]] = 1
    got = eng.panel_select_depth(g, opt, fwd, rev, m.seed_rule(2, 3), 2, sm.pack_bitmap(planted(130, 0.02)), 2,
                                 forced=forced)
    kept = np.flatnonzero(got["keep"])
    assert 2 < kept.size < 130
    total = np.zeros(got["depth_kept"].shape, dtype=np.int64)
    for p in kept:
        f, r = ([fwd[p]], []) if p < len(fwd) else ([], [rev[p - len(fwd)]])
        total += eng.segment_coverage_mm(g, opt, f, r, 2, 3) != 255
    np.testing.assert_array_equal(got["depth_kept"], total)
    assert got["counts"][1] == int((total >= 1).sum()) and got["counts"][3] == int((total >= 2).sum()) > 0


@pytest.mark.parametrize("n", [63, 64, 65, 129])
@pytest.mark.parametrize("n_seq,L,n_seg", [(4, 2440, 52), (53, 450, 53), (6, 1760, 54), (107, 500, 107)])
def test_word_and_group_boundaries(m, eng, n, n_seq, L, n_seg):
    """n primers at the mask and bitmap word boundaries over 52, 53, 54 and 107 segments (53 per group)."""
    g = m.synth.aligned_genomes(n_seq, L, seed=n_seg)
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    assert n_seq * tm.n_partitions(L, 400, 170) == n_seg
    rng = np.random.default_rng(n_seg * 1000 + n)
    fwd, rev = distinct_sets(rng, g, n // 2, n - n // 2, 13)
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    B = planted(n, 0.08, seed=n)
    check(m, eng, g, opt, fwd, rev, I, B, 2, 2, forms=("bitmap", "packed"))
    B[n - 1, 0] = B[0, n - 1] = True                 # the last bit of a row, the last row
    check(m, eng, g, opt, fwd, rev, I, B, 3, 64, forced=rng.random(n) < 0.05)


def test_a_self_loop_with_and_without_drop_self_pairs(m, eng):
    g, fwd, rev, opt = small_case(m)
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    best = int(tm.greedy(I)[1][0])
    B = np.zeros((40, 40), dtype=bool)
    B[best, best] = True
    want = check(m, eng, g, opt, fwd, rev, I, B, 2, 2, forms=("bitmap", "packed"))
    assert want["barred"][best] == 1 and want["keep"][best] == 0 and want["barred"].sum() == 1
    want = check(m, eng, g, opt, fwd, rev, I, B, 2, 2, drop=True, forms=("bitmap", "packed"))
    assert want["order"][0] == best and not want["barred"].any()


def test_a_one_direction_edge(m, eng):
    g, fwd, rev, opt = small_case(m)
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    a, b = (int(x) for x in tm.greedy(I)[1][:2])
    for src, dst in ((a, b), (b, a)):
        B = np.zeros((40, 40), dtype=bool)
        B[src, dst] = True
        want = check(m, eng, g, opt, fwd, rev, I, B, 2, 1, forms=("bitmap", "packed"))
        assert want["order"][0] == a and want["barred"][b] == 1 and want["keep"][b] == 0
        want = check(m, eng, g, opt, fwd, rev, I, B, 2, 2)
        assert want["tube"][a] == 0 and want["tube"][b] == 1


def test_forced_primers_with_neighbours(m, eng, grids):
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    order = tm.greedy(I)[1].astype(np.int64)
    forced = np.zeros(130, dtype=np.uint8)
    forced[[5, 77]] = 1
    B = planted(130, 0.02, seed=9, self_loops=False)
    B[5, order[0]] = B[order[1], 77] = True          # the two best picks are neighbours of the panel, either direction
    for T in (1, 4):
        want = check(m, eng, g, opt, fwd, rev, I, B, 3, T, forced=forced, forms=("bitmap", "dev", "packed"))
        assert want["barred"][order[0]] == 1 and want["barred"][order[1]] == 1
        assert (want["tube"][forced != 0] == 255).all() and (want["keep"][forced != 0] == 1).all()
    every = np.ones(130, dtype=np.uint8)
    want = check(m, eng, g, opt, fwd, rev, I, B, 2, 2, forced=every)
    assert want["order"].size == 0 and want["tubes_used"] == 0 and want["counts"].tolist() == [77, 77, 45, 45]


@pytest.mark.parametrize("min_gain", [2, 5])
def test_min_gain(m, eng, grids, min_gain):
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    B = planted(130, 0.05, seed=min_gain)
    want = check(m, eng, g, opt, fwd, rev, I, B, 3, 2, min_gain, forms=("bitmap", "packed"))
    assert want["order"].size and (want["gains"] >= min_gain).all() and want["layers"] == 3


def test_saturation_over_255_layers(m, eng):
    """300 distinct 5-mers at M = 5, E = 0 over a zero graph: every primer matches every window, so every count is
    300, both planes saturate, and each of the 255 layers is one pick and one stopping round."""
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(1).integers(0, 4, size=(2, 600))].copy()
    words = ["".join("ACGT"[(i >> (2 * j)) & 3] for j in range(5)) for i in range(300)]
    opt = m.KmerOpt(300, 150, 40, 5, 0, 0)
    n_seg = 2 * tm.n_partitions(600, 300, 150)
    I = np.ones((300, n_seg), dtype=bool)
    want = check(m, eng, g, opt, words[:150], words[150:], I, np.zeros((300, 300), dtype=bool), 255, M=5, E=0)
    assert want["order"].tolist() == list(range(255)) and want["layer"].tolist() == list(range(1, 256))
    assert (want["depth_all"] == 255).all() and (want["depth_kept"] == 255).all() and want["rounds"] == 510
    assert want["counts"].tolist() == [n_seg] * 4 and eng.info("panel_select_depth_layers") == 255


def test_layers_that_span_batches_of_rounds(m, eng):
    """One primer per segment and a second one on two in three: layer 1 and layer 2 each take more than 16 rounds."""
    rng = np.random.default_rng(5)
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(6, 2000))].copy()   # unrelated rows
    opt = m.KmerOpt(400, 200, 50, 13, 0, 0)
    fwd = [bytes(g[r, j * 200 + 5:j * 200 + 18]).decode() for r in range(6) for j in range(9)]
    fwd += [bytes(g[r, j * 200 + 25:j * 200 + 38]).decode() for r in range(6) for j in range(9) if j % 3]
    assert len(set(fwd)) == len(fwd)
    I = tm.incidence(g, 400, 200, 50, 13, fwd, [], 0, 3)
    want = check(m, eng, g, opt, fwd, [], I, planted(len(fwd), 0.02, seed=1, self_loops=False), 3, 2, M=0)
    per_layer = np.bincount(want["layer"], minlength=4)
    assert per_layer[1] > 32 and per_layer[2] > 16, per_layer


@pytest.mark.parametrize("thr", [30.0, -5.0])
def test_the_held_incidence_end1(m, eng, oracle, oracle_tables, thr):
    """Mode 2 at 30 C against the model over the held incidence (the CPU oracle scores every match); at a threshold
    <= 0 the matrix is the string rule's."""
    g = m.synth.aligned_genomes(10, 2600, seed=53)
    fwd, rev = distinct_sets(np.random.default_rng(1302), g, 60, 60, 13)
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem = m.Chem.ntthal()
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    if thr > 0:
        res = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, 13, fwd, rev, 2, 3, "end1", thr, oracle.ntthal_args())
        H = ttm.held_incidence(res)
        assert H.sum() < I.sum() and not (H & ~I).any()
    else:
        H = I
    B = planted(120, 0.03, seed=7)
    bits = sm.pack_bitmap(B)
    forced = np.zeros(120, dtype=np.uint8)
    forced[[4, 117]] = 1
    rule = m.seed_rule(2, 3, "end1", chem, thr)
    for R, T, f in ((2, 1, None), (3, 2, forced)):
        want = dm.select_depth(H, B, R, T, 1, f)
        for form in ("bitmap", "packed"):
            agree(eng.panel_select_depth(g, opt, fwd, rev, rule, R, bits, T, forced=f, form=form), want, form)
        assert eng.info("panel_select_rounds") == want["rounds"]


def test_the_forms_that_screen_themselves(m, eng, grids):
    """msspe_panel_select_depth and _rule against the bitmap form fed the screen's own bitmap (ntthal chemistry,
    -9,000 cal/mol; under the rule also END1 at 30 C)."""
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem, thr, n = m.Chem.ntthal(), -9000.0, 130
    pool = fwd + rev
    B = sm.unpack_bitmap(eng.cross_dimer(pool, chem, thr, want_dg=False)["bitmap"], n)
    assert 0 < int((B & ~np.eye(n, dtype=bool)).sum()) < n * (n - 1)
    U = sm.unpack_bitmap(eng.conflict_graph(pool, chem, m.ConflictRule.of(thr, 30.0))["bitmap"], n)
    assert not (B & ~U).any()
    for T, drop, R in ((1, False, 2), (3, False, 3), (2, True, 2)):
        for graph, end_tm in ((B, None), (U, 30.0)):
            ref = eng.panel_select_depth(g, opt, fwd, rev, m.seed_rule(2, 3), R, sm.pack_bitmap(graph), T,
                                         drop_self_pairs=drop)
            got = eng.panel_select_depth(g, opt, fwd, rev, m.seed_rule(2, 3), R, None, T, drop_self_pairs=drop,
                                         form="screen", chem=chem, threshold=thr, end_tm_threshold=end_tm)
            for key in KEYS + PLANES:
                np.testing.assert_array_equal(got[key], ref[key], key)
            assert got["tubes_used"] == ref["tubes_used"]
    agree(ref, dm.select_depth(I, U, 2, 2, 1, None, True), "the union, dropped self pairs")


def test_empty_inputs(m, eng):
    g = m.synth.aligned_genomes(5, 1500, seed=3)
    fwd, rev = distinct_sets(np.random.default_rng(3), g, 20, 20, 13)
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    for f, r in (([], []), (fwd, []), ([], rev)):
        n = len(f) + len(r)
        I = tm.incidence(g, 400, 170, 50, 13, f, r, 2, 3)
        check(m, eng, g, opt, f, r, I, planted(n, 0.1), 2, 2, forms=("bitmap", "dev", "packed"))
    n = len(fwd) + len(rev)
    forced = np.zeros(n, dtype=np.uint8)
    forced[[1, n - 1]] = 1
    got = eng.panel_select_depth(g, m.KmerOpt(2000, 170, 50, 13, 0, 0), fwd, rev, m.seed_rule(2, 3), 3, None, 2,
                                 forced=forced)                                         # seq_len < segment
    assert got["keep"].tolist() == forced.tolist() and got["order"].size == 0 and got["depth_kept"].shape == (5, 0)
    assert (got["tube"] == 255).all() and not got["barred"].any()
    assert got["counts"].tolist() == [0, 0, 0, 0] and got["tubes_used"] == 0
    gaps = np.full((4, 1500), ord("-"), dtype=np.uint8)
    want = check(m, eng, gaps, opt, fwd, rev, np.zeros((n, 4 * tm.n_partitions(1500, 400, 170)), dtype=bool),
                 planted(n, 0.1), 3, 1, forced=forced)
    assert want["order"].size == 0 and want["counts"].tolist() == [0, 0, 0, 0] and want["rounds"] == 1


def test_matrix_cap_and_the_depth_range(m, eng, grids):
    g = m.synth.aligned_genomes(40, 6000, seed=9)
    opt = m.KmerOpt(400, 60, 50, 13, 0, 0)
    fwd, rev = primer_sets(np.random.default_rng(9), g, 995, 13)       # 2,000 primers: 71 groups x 2,048 words
    default = eng.info("panel_thin_matrix_max_mb")
    eng.set_option("panel_thin_matrix_max_mb", 1)
    try:
        with pytest.raises(m.MsspeError) as e:
            eng.panel_select_depth(g, opt, fwd, rev, m.seed_rule(1, 3), 2, None, 2)
        assert e.value.code == 5 and "needs 2 MB" in str(e.value)
    finally:
        eng.set_option("panel_thin_matrix_max_mb", default)
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    for R in (0, 256, -1):
        for form in ("bitmap", "dev", "packed", "screen"):
            with pytest.raises(m.MsspeError) as e:
                eng.panel_select_depth(g, opt, fwd, rev, m.seed_rule(2, 3), R, None, 1, form=form)
            assert e.value.code == 1 and "depth" in str(e.value), (R, form)
    with pytest.raises(m.MsspeError) as e:                         # the form that screens under the rule
        eng.panel_select_depth(g, opt, fwd, rev, m.seed_rule(2, 3), 256, None, 1, form="screen", end_tm_threshold=30.0)
    assert e.value.code == 1 and "depth" in str(e.value)
    for T in (0, 65):
        with pytest.raises(m.MsspeError) as e:
            eng.panel_select_depth(g, opt, fwd, rev, m.seed_rule(2, 3), 2, None, T)
        assert e.value.code == 1 and "max_tubes" in str(e.value)
    with pytest.raises(m.MsspeError) as e:
        eng.panel_select_depth(g, opt, fwd + [fwd[3]], rev, m.seed_rule(2, 3), 2, None, 1)
    assert e.value.code == 1 and "duplicate" in str(e.value)
    with pytest.raises(m.MsspeError) as e:
        eng.panel_select_depth(g, opt, fwd, rev, m.seed_rule(2, 3), 2, None, 1, min_gain=0)
    assert e.value.code == 1
    for R in (1, 255):                                             # the ends of the range are taken
        assert len(eng.panel_select_depth(g, opt, fwd, rev, m.seed_rule(2, 3), R, None, 1)["order"]) >= 10
    L = m.load_library()
    keep, tube = np.zeros(130, np.uint8), np.zeros(130, np.uint8)
    order, gains, picked = np.zeros(130, np.uint32), np.zeros(130, np.uint32), C.c_int(-1)
    f, r, bits = m.pack_oligos(fwd), m.pack_oligos(rev), np.zeros((130, 3), dtype=np.uint64)
    rule, sel = m.seed_rule(2, 3), m.SelectDepthOpt(1, 1, 0, 2)

    def call(k=keep.ctypes.data, o=order.ctypes.data, ga=gains.ctypes.data, npk=C.byref(picked), t=tube.ctypes.data,
             b=bits.ctypes.data, ru=C.byref(rule), se=C.byref(sel)):
        return L.msspe_panel_select_depth_bitmap(eng.ptr, g.ctypes.data, g.shape[0], g.shape[1], C.byref(opt), ru, se,
                                                 f.ctypes.data, len(f), r.ctypes.data, len(r), None, b, k, o, ga, npk,
                                                 t, None, None, None, None, None, None)

    assert call() == 0 and picked.value > 10                       # every optional output may be NULL
    for bad in ({"k": None}, {"o": None}, {"ga": None}, {"npk": None}, {"t": None}, {"b": None}, {"ru": None},
                {"se": None}):
        assert call(**bad) == 1, bad


def test_shared_buffers_with_the_other_calls(m, eng, grids):
    """A larger depth call, a smaller one on the same context, then the selection and the depth thinning with their
    usual results."""
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    bits = sm.pack_bitmap(planted(130, 0.1))
    before = eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), bits, 2, form="packed")
    thin_before = eng.panel_thin_depth(g, opt, fwd, rev, 2, 3, 2, form="packed")
    check(m, eng, g, opt, fwd, rev, I, planted(130, 0.1), 3, 2, forms=("packed",))
    small = m.synth.aligned_genomes(3, 900, seed=2)
    f2, r2 = distinct_sets(np.random.default_rng(2), small, 9, 9, 13)
    I2 = tm.incidence(small, 400, 170, 50, 13, f2, r2, 2, 3)
    check(m, eng, small, opt, f2, r2, I2, planted(18, 0.1, seed=3), 2, 2, forms=("bitmap", "packed"))
    after = eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), bits, 2, form="packed")
    for key in ("order", "gains", "keep", "tube", "barred", "covered"):
        np.testing.assert_array_equal(after[key], before[key], key)
    assert (after["covered_all"], after["covered_kept"]) == (before["covered_all"], before["covered_kept"]) == (77, 66)
    for a, b in zip(thin_before, eng.panel_thin_depth(g, opt, fwd, rev, 2, 3, 2, form="packed")):
        np.testing.assert_array_equal(a, b)


# ---- the CLI ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_fasta(m, tmp_path_factory):
    """The inputs of test_gpu_panel_select.py's CLI tests."""
    g = np.concatenate([m.synth.aligned_genomes(20, 6000, seed=700 + j) for j in range(2)])
    fa = tmp_path_factory.mktemp("select_depth_cli") / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    return fa, g


def block_of(out):
    at = out.index("\nPanel selection by coverage")
    lines = out[at:].split("\n")
    end = 7
    while end < len(lines) and lines[end].startswith("  Tube "):
        end += 1
    return "".join(l + "\n" for l in lines[:end])


def cli_case(m, eng, fa, g, tmp_path, extra, T=1, R=2, panel=((), ()), rule_args=(), mode=0, tm_c=0.0):
    """The CLI with the flag against the device fed what the CLI fed it (and, in mode 0, against the model): the
    primers that reach the step are the kept ones and the rejected ones of reason select_*, in the order of the lists;
    the graph is the screen's."""
    rej = tmp_path / "rej.csv"
    out, rows = run_cli(fa, tmp_path / "b.csv", *extra, *rule_args, "--select-by-coverage", "true",
                        "--thin-mismatches", "2", "--select-depth", str(R), "--rejected-out", str(rej))
    dropped = [l.split(",") for l in rej.read_text().splitlines()[1:] if l]
    sel_drop = {r[2]: r[4] for r in dropped if r[4].startswith("select_")}
    _, every = run_cli(fa, tmp_path / "all.csv", *extra, "--keep-all", "true")
    kept_words = {r[2] for r in rows}
    fwd = [r[2] for r in every if r[0] == "F" and (r[2] in kept_words or r[2] in sel_drop)]
    rev = [r[2] for r in every if r[0] == "R" and (r[2] in kept_words or r[2] in sel_drop)]
    assert len(fwd) + len(rev) == len(rows) + len(sel_drop)
    all_f, all_r = fwd + list(panel[0]), rev + list(panel[1])
    pool = all_f + all_r
    n = len(pool)
    forced = np.array([0] * len(fwd) + [1] * len(panel[0]) + [0] * len(rev) + [1] * len(panel[1]), dtype=np.uint8)
    chem = m.Chem.ntthal()
    B = sm.unpack_bitmap(eng.cross_dimer(pool, chem, -9000.0, want_dg=False)["bitmap"], n)
    rule = m.seed_rule(2, 3, mode, chem if mode else None, tm_c)
    opt = m.KmerOpt(500, 250, 50, 13, 0, 0)
    dev = eng.panel_select_depth(g, opt, all_f, all_r, rule, R, sm.pack_bitmap(B), T, forced=forced)
    if not mode:
        I = tm.incidence(g, 500, 250, 50, 13, all_f, all_r, 2, 3)
        agree(dev, dm.select_depth(I, B, R, T, 1, forced), "cli inputs")
    flat = eng.panel_select(g, opt, all_f, all_r, rule, sm.pack_bitmap(B), T, forced=forced)
    assert int(dev["keep"].sum()) > int(flat["keep"].sum())         # the depth keeps primers the selection drops
    keep, tube, barred = dev["keep"], dev["tube"], dev["barred"]
    kf = [w for w, q in zip(fwd, keep[:len(fwd)]) if q]
    kr = [w for w, q in zip(rev, keep[len(all_f):len(all_f) + len(rev)]) if q]
    assert [r[2] for r in rows if r[0] == "F"] == kf and [r[2] for r in rows if r[0] == "R"] == kr
    assert 0 < len(kf) + len(kr) < len(fwd) + len(rev)
    new = forced == 0
    for w, q, b in zip(np.array(pool)[new], keep[new], barred[new]):
        assert (w in sel_drop) == (not q)
        if not q:
            assert sel_drop[w] == ("select_conflict" if b else "select_unneeded"), w
    per_tube = None
    if "--tubes" in extra:
        of = {w: int(t) for w, t in zip(pool, tube)}
        assert [int(r[7]) for r in rows] == [of[r[2]] + 1 for r in rows]          # the CSV's column counts from 1
        per_tube = [int((tube[new & (keep != 0)] == t).sum()) for t in range(dev["tubes_used"])]
    assert block_of(out) == dm.render_depth_block(mode, tm_c, 2, 3, 1, T, R, len(kf), len(fwd), len(kr), len(rev),
                                                  int(forced.sum()), int(barred[new].sum()), dev["counts"],
                                                  g.shape[0] * tm.n_partitions(g.shape[1], 500, 250), per_tube)
    return out, rows


def test_cli_depth_one_prints_todays_bytes(small_fasta, tmp_path):
    fa, g = small_fasta
    args = ("--select-by-coverage", "true", "--thin-mismatches", "2", "--tubes", "2")
    plain, _ = run_cli(fa, tmp_path / "0.csv", *args)
    one, _ = run_cli(fa, tmp_path / "1.csv", *args, "--select-depth", "1")
    assert one == plain and "Panel selection by coverage" in plain
    assert (tmp_path / "0.csv").read_bytes() == (tmp_path / "1.csv").read_bytes()
    assert "Depth:" not in one and ", depth" not in one


def test_cli_selects_to_a_depth_with_tubes(m, eng, small_fasta, tmp_path):
    fa, g = small_fasta
    cli_case(m, eng, fa, g, tmp_path, ("--tubes", "4"), T=4)


def test_cli_with_existing_primers(m, eng, small_fasta, tmp_path):
    fa, g = small_fasta
    _, first = run_cli(fa, tmp_path / "first.csv")
    panel_rows = [r for r in first if r[0] == "F"][:4] + [r for r in first if r[0] == "R"][:4]
    panel = tmp_path / "panel.csv"
    panel.write_text("direction,name,primers,gc,avg,std,tm\n" + "".join(",".join(r) + "\n" for r in panel_rows))
    pf = [r[2] for r in panel_rows if r[0] == "F"]
    pr = [r[2] for r in panel_rows if r[0] == "R"]
    out, rows = cli_case(m, eng, fa, g, tmp_path, ("--existing-primers", str(panel)), panel=(pf, pr))
    assert not {r[2] for r in rows} & set(pf + pr) and ", 8 forced\n" in out


def test_cli_with_the_held_rule(m, eng, small_fasta, tmp_path):
    fa, g = small_fasta
    cli_case(m, eng, fa, g, tmp_path, (), rule_args=("--thin-tm", "30", "--thin-thal", "end1"), mode=2, tm_c=30.0)
