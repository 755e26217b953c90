"""msspe_panel_select* on the device against the numpy model (tests/panel_select_model.py): order, gains, keep, tube,
barred, covered, both counts, the tubes in use and the rounds, exactly.  The grid inputs under planted graphs in the
host-bitmap, _dev and _packed_dev forms, the zero-graph identity against the thinning calls, the complete graph, the
mask, bitmap and group boundaries, a self loop, a one-direction edge, forced primers with neighbours, min_gain above 1,
more than two batches of rounds, the empty inputs, the matrix cap, the argument errors, the call that screens itself,
the guarantee through the existing coverage call, and the CLI's --select-by-coverage."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import panel_select_model as sm
import panel_thin_model as tm
from test_coverage_mm_model import draw_primers, rc
from test_panel_thin_model import grid_case

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"
GOLDEN = ROOT / "tests" / "golden" / "panel_select"
KEYS = ("order", "gains", "keep", "tube", "barred")
COUNTS = ("covered_all", "covered_kept", "tubes_used")


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


def planted(n, density, seed=5, self_loops=True):
    B = np.random.default_rng(seed).random((n, n)) < density
    if not self_loops:
        B[np.arange(n), np.arange(n)] = False
    return B


def primer_sets(rng, g, n, k):
    return draw_primers(rng, g, n, k), [rc(w) for w in draw_primers(rng, g, n, k)]


def distinct_sets(rng, g, n_f, n_r, k):
    """n_f forward and n_r reverse primers, no word twice: the graph's nodes are distinct."""
    words = list(dict.fromkeys(draw_primers(rng, g, 2 * (n_f + n_r), k)))
    fwd = words[:n_f]
    rev = [w for w in dict.fromkeys(rc(x) for x in words[n_f:]) if w not in set(fwd)][:n_r]
    assert len(fwd) == n_f and len(rev) == n_r and len(set(fwd + rev)) == n_f + n_r
    return fwd, rev


def agree(got, want, what=""):
    for key in KEYS:
        np.testing.assert_array_equal(got[key], want[key], f"{key} {what}")
    np.testing.assert_array_equal(got["covered"].reshape(-1), want["covered"].astype(np.uint8), f"covered {what}")
    for key in COUNTS:
        assert got[key] == want[key], f"{key} {what}"


def check(m, eng, g, opt, fwd, rev, I, B, T=1, min_gain=1, forced=None, drop=False, forms=("bitmap",), M=2, E=3):
    """The device result of every form against the model over the incidence I; returns the model's result."""
    want = sm.select(I, B, T, min_gain, forced, drop)
    sm.check_independent(want, B, forced, drop)
    bits = sm.pack_bitmap(B)
    for form in forms:
        got = eng.panel_select(g, opt, fwd, rev, m.seed_rule(M, E), bits, T, min_gain, drop, forced, form)
        agree(got, want, form)
        if I.size:
            assert eng.info("panel_select_rounds") == want["rounds"], form
            assert eng.info("panel_select_tubes") == want["tubes_used"], form
            assert eng.info("panel_select_barred") == int(want["barred"].sum()), form
    return want


@pytest.mark.parametrize("k", [13, 24])
@pytest.mark.parametrize("density", [0.02, 0.1])
def test_grid_under_planted_graphs_in_the_three_forms(m, eng, grids, k, density):
    g, fwd, rev, I = grids[k]
    assert len(set(fwd + rev)) == 130
    opt = m.KmerOpt(400, 170, 50, k, 0, 0)
    B = planted(130, density)
    for T in (1, 2, 4):
        want = check(m, eng, g, opt, fwd, rev, I, B, T, forms=("bitmap", "dev", "packed"))
        if (k, density, T) == (13, 0.1, 1):
            assert (len(want["order"]), want["covered_kept"], want["covered_all"]) == (6, 55, 77)
    check(m, eng, g, opt, fwd, rev, I, B, 2, drop=True, forms=("packed",))


def test_covered_is_what_the_kept_primers_cover(m, eng, grids):
    """The guarantee through the existing call: covered_out == (segment_coverage_mm(kept) != 255)."""
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    forced = np.random.default_rng(2).random(130) < 0.05
    got = eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), sm.pack_bitmap(planted(130, 0.05)), 2, forced=forced)
    keep = got["keep"]
    assert 0 < keep.sum() < 130
    kf = [w for w, q in zip(fwd, keep[:len(fwd)]) if q]
    kr = [w for w, q in zip(rev, keep[len(fwd):]) if q]
    np.testing.assert_array_equal(got["covered"] == 1, eng.segment_coverage_mm(g, opt, kf, kr, 2, 3) != 255)
    assert got["covered_kept"] == int(got["covered"].sum()) <= got["covered_all"]


def test_zero_graph_is_the_thinning(m, eng, grids):
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    forced = np.random.default_rng(3).random(130) < 0.06
    for f in (None, forced):
        keep, order, gains, covered, c_all, c_kept = eng.panel_thin(g, opt, fwd, rev, 2, 3, 1, f, "packed")
        rounds = eng.info("panel_thin_rounds")
        for T in (1, 7, 64):
            got = eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), None, T, forced=f, form="packed")
            np.testing.assert_array_equal(got["order"], order)
            np.testing.assert_array_equal(got["gains"], gains)
            np.testing.assert_array_equal(got["keep"], keep)
            np.testing.assert_array_equal(got["covered"], covered)
            assert (got["covered_all"], got["covered_kept"]) == (c_all, c_kept)
            assert eng.info("panel_select_rounds") == rounds and got["tubes_used"] == 1
            assert (got["tube"][order.astype(np.int64)] == 0).all() and not got["barred"].any()


def test_zero_graph_is_the_thal_thinning_in_mode_2(m, eng, grids):
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem = m.Chem.ntthal()
    keep, order, gains, covered, c_all, c_kept = eng.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, "end1", 30.0)
    assert 0 < order.size and c_all <= int(I.any(axis=0).sum())         # H is a subset of I
    for T in (1, 3):
        got = eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3, "end1", chem, 30.0), None, T, form="packed")
        np.testing.assert_array_equal(got["order"], order)
        np.testing.assert_array_equal(got["gains"], gains)
        np.testing.assert_array_equal(got["keep"], keep)
        np.testing.assert_array_equal(got["covered"], covered)
        assert (got["covered_all"], got["covered_kept"], got["tubes_used"]) == (c_all, c_kept, 1)
    # a threshold <= 0 gives mode 0's matrix
    want = eng.panel_thin(g, opt, fwd, rev, 2, 3)
    got = eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3, "any", chem, 0.0), None, 1)
    np.testing.assert_array_equal(got["order"], want[1])
    np.testing.assert_array_equal(got["gains"], want[2])


@pytest.mark.parametrize("T", [1, 3, 64])
def test_complete_graph(m, eng, grids, T):
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    want = check(m, eng, g, opt, fwd, rev, I, ~np.eye(130, dtype=bool), T, forms=("bitmap", "packed"))
    _, order, gains, *_ = tm.greedy(I)
    k = min(T, len(order))
    np.testing.assert_array_equal(want["order"], order[:k])
    assert want["tube"][order[:k].astype(np.int64)].tolist() == list(range(k)) and want["tubes_used"] == k


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
    check(m, eng, g, opt, fwd, rev, I, B, 2, forms=("bitmap", "packed"))
    B[n - 1, 0] = B[0, n - 1] = True                 # the last bit of a row, the last row
    check(m, eng, g, opt, fwd, rev, I, B, 64, forced=rng.random(n) < 0.05)


def small_case(m):
    g, fwd, rev = grid_case(13, 2)
    return g, fwd[:20], rev[:20], m.KmerOpt(400, 170, 50, 13, 0, 0)


def test_a_self_loop_with_and_without_drop_self_pairs(m, eng):
    g, fwd, rev, opt = small_case(m)
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    best = int(tm.greedy(I)[1][0])
    B = np.zeros((40, 40), dtype=bool)
    B[best, best] = True
    want = check(m, eng, g, opt, fwd, rev, I, B, 2, forms=("bitmap", "packed"))
    assert want["barred"][best] == 1 and want["keep"][best] == 0 and want["barred"].sum() == 1
    want = check(m, eng, g, opt, fwd, rev, I, B, 2, drop=True, forms=("bitmap", "packed"))
    assert want["order"][0] == best and not want["barred"].any()


def test_a_one_direction_edge(m, eng):
    g, fwd, rev, opt = small_case(m)
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    a, b = (int(x) for x in tm.greedy(I)[1][:2])
    for src, dst in ((a, b), (b, a)):
        B = np.zeros((40, 40), dtype=bool)
        B[src, dst] = True
        want = check(m, eng, g, opt, fwd, rev, I, B, 1, forms=("bitmap", "packed"))
        assert want["order"][0] == a and want["barred"][b] == 1 and want["keep"][b] == 0
        want = check(m, eng, g, opt, fwd, rev, I, B, 2)
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
        want = check(m, eng, g, opt, fwd, rev, I, B, T, forced=forced, forms=("bitmap", "dev", "packed"))
        assert want["barred"][order[0]] == 1 and want["barred"][order[1]] == 1
        assert (want["tube"][forced != 0] == 255).all() and (want["keep"][forced != 0] == 1).all()
    every = np.ones(130, dtype=np.uint8)
    want = check(m, eng, g, opt, fwd, rev, I, B, 2, forced=every)
    assert want["order"].size == 0 and want["tubes_used"] == 0


@pytest.mark.parametrize("min_gain", [2, 5])
def test_min_gain(m, eng, grids, min_gain):
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    B = planted(130, 0.05, seed=min_gain)
    want = check(m, eng, g, opt, fwd, rev, I, B, 2, min_gain, forms=("bitmap", "packed"))
    assert want["order"].size and (want["gains"] >= min_gain).all()


def test_more_than_two_batches_of_rounds(m, eng):
    rng = np.random.default_rng(5)
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(6, 2000))].copy()   # unrelated rows
    opt = m.KmerOpt(400, 200, 50, 13, 0, 0)
    fwd = [bytes(g[r, j * 200 + 5:j * 200 + 18]).decode() for r in range(6) for j in range(9)]   # one per segment
    assert len(set(fwd)) == len(fwd)
    I = tm.incidence(g, 400, 200, 50, 13, fwd, [], 0, 3)
    want = check(m, eng, g, opt, fwd, [], I, planted(len(fwd), 0.03, seed=1, self_loops=False), 2, M=0)
    assert len(want["order"]) > 32 and eng.info("panel_select_rounds") == len(want["order"]) + 1


def test_empty_inputs(m, eng):
    g = m.synth.aligned_genomes(5, 1500, seed=3)
    fwd, rev = distinct_sets(np.random.default_rng(3), g, 20, 20, 13)
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    for f, r in (([], []), (fwd, []), ([], rev)):
        n = len(f) + len(r)
        I = tm.incidence(g, 400, 170, 50, 13, f, r, 2, 3)
        check(m, eng, g, opt, f, r, I, planted(n, 0.1), 2, forms=("bitmap", "dev", "packed"))
    n = len(fwd) + len(rev)
    forced = np.zeros(n, dtype=np.uint8)
    forced[[1, n - 1]] = 1
    got = eng.panel_select(g, m.KmerOpt(2000, 170, 50, 13, 0, 0), fwd, rev, m.seed_rule(2, 3), None, 2,
                           forced=forced)                                               # seq_len < segment
    assert got["keep"].tolist() == forced.tolist() and got["order"].size == 0 and got["covered"].shape == (5, 0)
    assert (got["tube"] == 255).all() and not got["barred"].any()
    assert (got["covered_all"], got["covered_kept"], got["tubes_used"]) == (0, 0, 0)
    gaps = np.full((4, 1500), ord("-"), dtype=np.uint8)
    want = check(m, eng, gaps, opt, fwd, rev, np.zeros((n, 4 * tm.n_partitions(1500, 400, 170)), dtype=bool),
                 planted(n, 0.1), 1, forced=forced)
    assert want["order"].size == 0 and want["covered_all"] == 0


def test_matrix_cap_duplicates_and_tube_limits(m, eng, grids):
    g = m.synth.aligned_genomes(40, 6000, seed=9)
    opt = m.KmerOpt(400, 60, 50, 13, 0, 0)
    fwd, rev = primer_sets(np.random.default_rng(9), g, 995, 13)       # 2,000 primers: 71 groups x 2,048 words
    default = eng.info("panel_thin_matrix_max_mb")
    eng.set_option("panel_thin_matrix_max_mb", 1)
    try:
        with pytest.raises(m.MsspeError) as e:
            eng.panel_select(g, opt, fwd, rev, m.seed_rule(1, 3), None, 2)
        assert e.value.code == 5 and "needs 2 MB" in str(e.value) and "panel_thin_matrix_max_mb is 1" in str(e.value)
    finally:
        eng.set_option("panel_thin_matrix_max_mb", default)
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    for f, r in ((fwd + [fwd[3]], rev), (fwd, rev + [fwd[0]])):          # a word twice, within a list and across both
        with pytest.raises(m.MsspeError) as e:
            eng.panel_select(g, opt, f, r, m.seed_rule(2, 3), None, 1)
        assert e.value.code == 1 and "duplicate" in str(e.value)
    for T in (0, 65, -1):
        for form in ("bitmap", "dev", "packed", "screen"):
            with pytest.raises(m.MsspeError) as e:
                eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), None, T, form=form)
            assert e.value.code == 1 and "max_tubes" in str(e.value)
    with pytest.raises(m.MsspeError) as e:
        eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), None, 1, min_gain=0)
    assert e.value.code == 1
    with pytest.raises(m.MsspeError) as e:
        eng.panel_select(g, m.KmerOpt(400, 170, 50, 1, 0, 0), ["A"], ["C"], m.seed_rule(0, 0), None, 1)
    assert e.value.code == 2
    with pytest.raises(m.MsspeError) as e:
        eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3, 3), None, 1)
    assert e.value.code == 1
    with pytest.raises(m.MsspeError) as e:
        eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3, 1, None, 30.0), None, 1)
    assert e.value.code == 1
    L = m.load_library()
    keep, tube = np.zeros(130, np.uint8), np.zeros(130, np.uint8)
    order, gains, picked = np.zeros(130, np.uint32), np.zeros(130, np.uint32), C.c_int(-1)
    f, r, bits = m.pack_oligos(fwd), m.pack_oligos(rev), np.zeros((130, 3), dtype=np.uint64)
    rule, sel = m.seed_rule(2, 3), m.SelectOpt(1, 1, 0)

    def call(k=keep.ctypes.data, o=order.ctypes.data, ga=gains.ctypes.data, npk=C.byref(picked), t=tube.ctypes.data,
             b=bits.ctypes.data, ru=C.byref(rule), se=C.byref(sel)):
        return L.msspe_panel_select_bitmap(eng.ptr, g.ctypes.data, g.shape[0], g.shape[1], C.byref(opt), ru, se,
                                           f.ctypes.data, len(f), r.ctypes.data, len(r), None, b, k, o, ga, npk, t,
                                           None, None, None, None, None)

    assert call() == 0 and picked.value == 10
    for bad in ({"k": None}, {"o": None}, {"ga": None}, {"npk": None}, {"t": None}, {"b": None}, {"ru": None},
                {"se": None}):
        assert call(**bad) == 1, bad


def device_put(m, eng, a):
    dev = C.c_void_p()
    eng._check(eng.L.msspe_device_put(eng.ptr, a.ctypes.data, a.nbytes, C.byref(dev)))
    return int(dev.value)


def test_the_call_that_screens_itself(m, eng, grids):
    """msspe_panel_select against the _packed_dev form fed msspe_cross_dimer_dev's bitmap, at the ntthal chemistry and
    -9,000 cal/mol: there the CPU oracle (pyoracle.pool_pairs over the 130 grid primers of k = 13, forward then
    reverse) shows 154 directed off-diagonal edges and 8 self conflicts, so the threshold stays at its default."""
    g, fwd, rev, I = grids[13]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem, thr, n, W = m.Chem.ntthal(), -9000.0, 130, 3
    d_pool = device_put(m, eng, np.concatenate([m.pack_oligos(fwd), m.pack_oligos(rev)]))
    d_bits = device_put(m, eng, np.zeros((n, W), dtype=np.uint64))
    try:
        eng.cross_dimer_dev(d_pool, n, 13, chem, thr, (0, n), (0, n), d_bitmap=d_bits)
        B = sm.unpack_bitmap(eng.device_get(d_bits, n * W * 8).view(np.uint64), n)
        off = B & ~np.eye(n, dtype=bool)
        assert 0 < int(off.sum()) < n * (n - 1)
        for T, drop in ((1, False), (3, False), (2, True)):
            ref = eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), d_bits, T, drop_self_pairs=drop, form="packed")
            got = eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), None, T, drop_self_pairs=drop, form="screen",
                                   chem=chem, threshold=thr)
            for key in KEYS + COUNTS:
                np.testing.assert_array_equal(got[key], ref[key], key)
            np.testing.assert_array_equal(got["covered"], ref["covered"])
            agree(ref, sm.select(I, B, T, 1, None, drop), "planted from the screen")
            # the kept set, screened again, has no conflicting pair in one tube
            kept = np.flatnonzero(got["keep"])
            words = [(fwd + rev)[i] for i in kept]
            again = sm.unpack_bitmap(eng.cross_dimer(words, chem, thr, want_dg=False)["bitmap"], len(words))
            if drop:
                again &= ~np.eye(len(words), dtype=bool)
            same_tube = got["tube"][kept][:, None] == got["tube"][kept][None, :]
            assert len(words) > 1 and not ((again | again.T) & same_tube).any()
    finally:
        eng.device_free(d_pool)
        eng.device_free(d_bits)


# ---- the CLI ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_fasta(m, tmp_path_factory):
    g = np.concatenate([m.synth.aligned_genomes(20, 6000, seed=700 + j) for j in range(2)])
    fa = tmp_path_factory.mktemp("select_cli") / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    return fa, g


def run_cli(fa, csv, *extra):
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rows = [l.split(",") for l in Path(csv).read_text().splitlines()[1:] if l]
    return r.stdout, rows


def block_of(out):
    at = out.index("\nPanel selection by coverage")
    lines = out[at:].split("\n")
    end = 6
    while end < len(lines) and lines[end].startswith("  Tube "):
        end += 1
    return "".join(l + "\n" for l in lines[:end])


def cli_case(m, eng, fa, g, tmp_path, extra, T=1, panel=((), ()), rule_args=(), mode=0, tm_c=0.0):
    """The CLI with the flag against the model fed what the CLI fed the device: the primers that reach the step are
    the kept ones and the rejected ones of reason select_*, in the order of the lists; the graph is the screen's."""
    rej = tmp_path / "rej.csv"
    out, rows = run_cli(fa, tmp_path / "b.csv", *extra, *rule_args, "--select-by-coverage", "true",
                        "--thin-mismatches", "2", "--rejected-out", str(rej))
    dropped = [l.split(",") for l in rej.read_text().splitlines()[1:] if l]
    assert {r[4] for r in dropped} <= {"stage_b", "select_conflict", "select_unneeded"}
    sel_drop = {r[2]: r[4] for r in dropped if r[4].startswith("select_")}
    # the offered lists in stage B's order: a plain run with --keep-all true lists every candidate in that order
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
    dev = eng.panel_select(g, m.KmerOpt(500, 250, 50, 13, 0, 0), all_f, all_r, rule, sm.pack_bitmap(B), T,
                           forced=forced)
    if not mode:
        I = tm.incidence(g, 500, 250, 50, 13, all_f, all_r, 2, 3)
        agree(dev, sm.select(I, B, T, 1, forced), "cli inputs")
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
        assert "Tube assignment" not in out
    assert block_of(out) == sm.render_block(mode, tm_c, 2, 3, 1, T, len(kf), len(fwd), len(kr), len(rev),
                                            int(forced.sum()), int(barred[new].sum()), dev["covered_all"],
                                            dev["covered_kept"], g.shape[0] * tm.n_partitions(g.shape[1], 500, 250),
                                            per_tube)
    assert out.index("Coverage report") < out.index("Panel selection by coverage")
    return out, rows


def test_cli_selects_by_coverage(m, eng, small_fasta, tmp_path):
    fa, g = small_fasta
    cli_case(m, eng, fa, g, tmp_path, ())


def test_cli_with_tubes(m, eng, small_fasta, tmp_path):
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


def test_cli_without_the_flag_is_unchanged(small_fasta, tmp_path):
    """Byte for byte the text and the CSV recorded from the parent commit on the same input."""
    fa, g = small_fasta
    out, _ = run_cli(fa, tmp_path / "plain.csv")
    assert out == (GOLDEN / "plain.stdout.txt").read_text()
    assert (tmp_path / "plain.csv").read_text() == (GOLDEN / "plain.csv").read_text()
    out, _ = run_cli(fa, tmp_path / "tubes.csv", "--tubes", "4", "--select-by-coverage", "false")
    assert out == (GOLDEN / "tubes4.stdout.txt").read_text()
    assert (tmp_path / "tubes.csv").read_text() == (GOLDEN / "tubes4.csv").read_text()
