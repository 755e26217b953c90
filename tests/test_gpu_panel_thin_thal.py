"""msspe_panel_thin_thal* on the device against its model (tests/panel_thin_thal_model.py: the scored matches of
coverage_thal_model with the CPU oracle's thal, the greedy loop of panel_thin_model): keep, order, gains, covered and
both counts, exactly.  The grid in both chemistries, modes and thresholds with forced sets and min_gain 2, the three
entry points, the guarantee through the device's own segment_coverage_thal, thin_thal_unique 0 against 1, slabs split
by groups and by primers, every scoring route, the group edges, W = k, invalid columns, the capacity statuses, argument
errors and empties, refused tables, the context's shared state, and the CLI's --thin-tm."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import coverage_thal_model as ctm
import panel_thin_model as tm
import panel_thin_thal_model as ttm
import param_variants as pv
from test_coverage_mm_model import draw_primers, rc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


def chems(m, oracle):
    return {"ntthal": (m.Chem.ntthal(), oracle.ntthal_args()), "primer3": (m.Chem.primer3(), oracle.p3_args())}


def primer_sets(rng, g, n, k, **kw):
    return draw_primers(rng, g, n, k, **kw), [rc(w) for w in draw_primers(rng, g, n, k, **kw)]


def equal(got, want, what=""):
    """An Engine.panel_thin_thal tuple against panel_thin_model.greedy's."""
    keep, order, gains, covered, c_all, c_kept = want[:6]
    np.testing.assert_array_equal(got[1], order, what)
    np.testing.assert_array_equal(got[2], gains, what)
    np.testing.assert_array_equal(got[0], keep, what)
    np.testing.assert_array_equal(got[3].reshape(-1), np.asarray(covered).astype(np.uint8).reshape(-1), what)
    assert (got[4], got[5]) == (c_all, c_kept), what


def flat(x):
    vals = x.values() if isinstance(x, dict) else x
    return [np.asarray(v).tobytes() for v in vals if isinstance(v, (np.ndarray, int))]


@pytest.fixture(scope="module")
def grid_input(m):
    """test_gpu_coverage_thal.py::grid_input: 65 + 65 primers, 130 matches in 77 of the 130 segments."""
    g = m.synth.aligned_genomes(10, 2600, seed=53)
    rng = np.random.default_rng(1302)
    fwd, rev = primer_sets(rng, g, 60, 13)
    return g, fwd, rev


@pytest.fixture(scope="module")
def grid_models(m, oracle, oracle_tables, grid_input):
    """The scored matches of the grid, per chemistry and mode, computed once and shared."""
    g, fwd, rev = grid_input
    out = {}
    for name, (_, args) in chems(m, oracle).items():
        for mode in ("any", "end1"):
            out[name, mode] = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, 13, fwd, rev, 2, 3, mode, 30.0, args)
    return out


@pytest.mark.parametrize("chem_name", ["ntthal", "primer3"])
@pytest.mark.parametrize("mode", ["any", "end1"])
def test_grid_equals_the_model(m, eng, oracle, grid_input, grid_models, chem_name, mode):
    g, fwd, rev = grid_input
    chem = chems(m, oracle)[chem_name][0]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    n = len(fwd) + len(rev)
    for thr in (30.0, 40.0):
        res = ctm.rethreshold(grid_models[chem_name, mode], thr)
        H = ttm.held_incidence(res)
        want = tm.greedy(H)
        equal(eng.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, mode, thr), want)
        assert eng.info("panel_thin_rounds") == want[6] and eng.info("panel_thin_groups") == -(-130 // 53)
        assert eng.info("panel_thin_thal_matches") == 130 and eng.info("panel_thin_thal_slabs") == 1
        assert want[4] == {("ntthal", 30.0): 69, ("ntthal", 40.0): 44, ("primer3", 30.0): 62,
                           ("primer3", 40.0): 40}[chem_name, thr]
        assert len(want[1]) == {("ntthal", 30.0): 10, ("ntthal", 40.0): 7, ("primer3", 30.0): 8,
                                ("primer3", 40.0): 6}[chem_name, thr]
        assert want[1].tolist() != tm.greedy(tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3))[1].tolist()[:len(want[1])]
        # forced sets: the first picks forced, and a primer whose row of H is empty forced
        some = np.zeros(n, dtype=np.uint8)
        some[want[1][:3]] = 1
        empty_row = int(np.flatnonzero(H.sum(axis=1) == 0)[0])
        some[empty_row] = 1
        got = eng.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, mode, thr, forced=some)
        equal(got, tm.greedy(H, 1, some), "forced")
        assert got[0][empty_row] == 1 and empty_row not in got[1].tolist()
        rng = np.random.default_rng(int(thr))
        rand = rng.random(n) < 0.06
        equal(eng.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, mode, thr, forced=rand), tm.greedy(H, 1, rand))
        every = np.ones(n, dtype=np.uint8)
        got = eng.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, mode, thr, forced=every)
        equal(got, tm.greedy(H, 1, every))
        assert got[1].size == 0 and got[4] == got[5]
        for G in (2, 5):
            equal(eng.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, mode, thr, min_gain=G), tm.greedy(H, G), f"G={G}")
            equal(eng.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, mode, thr, min_gain=G, forced=some),
                  tm.greedy(H, G, some), f"G={G} forced")
    # a threshold <= 0: H is the string rule's incidence, and the answer msspe_panel_thin's
    for thr in (0.0, -5.0):
        equal(eng.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, mode, thr), eng.panel_thin(g, opt, fwd, rev, 2, 3))


def test_entry_points_agree(m, eng, oracle, grid_input, grid_models):
    g, fwd, rev = grid_input
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem = m.Chem.ntthal()
    want = tm.greedy(ttm.held_incidence(grid_models["ntthal", "end1"]))
    for form in ("host", "dev", "packed"):
        equal(eng.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, "end1", 30.0, form=form), want, form)
    for form, put in (("packed", eng.put_rows_packed),):
        h = put(g)
        try:   # a resident alignment, as the CLI calls it
            equal(eng.panel_thin_thal((h, g.shape[0], g.shape[1]), opt, fwd, rev, 2, 3, chem, "end1", 30.0, form=form),
                  want, "resident " + form)
        finally:
            eng.device_free(h)
    for k in (24,):   # 64-bit primer words through the three forms, against each other
        g2 = m.synth.aligned_genomes(20, 5000, seed=3)
        f2, r2 = primer_sets(np.random.default_rng(5), g2, 80, k)
        o2 = m.KmerOpt(500, 250, 50, k, 0, 0)
        host = eng.panel_thin_thal(g2, o2, f2, r2, 2, 3, chem, "end1", 30.0)
        assert host[1].size > 3
        for form in ("dev", "packed"):
            assert flat(eng.panel_thin_thal(g2, o2, f2, r2, 2, 3, chem, "end1", 30.0, form=form)) == flat(host)


@pytest.mark.parametrize("chem_name,mode,thr", [("ntthal", "any", 30.0), ("ntthal", "end1", 40.0),
                                                ("primer3", "any", 40.0)])
def test_the_guarantee_through_the_devices_own_coverage(m, eng, oracle, grid_input, chem_name, mode, thr):
    g, fwd, rev = grid_input
    chem = chems(m, oracle)[chem_name][0]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    keep, order, gains, covered, c_all, c_kept = eng.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, mode, thr)
    whole = eng.segment_coverage_thal(g, opt, fwd, rev, 2, 3, chem, mode, thr)
    kf = [w for w, q in zip(fwd, keep[:len(fwd)]) if q]
    kr = [w for w, q in zip(rev, keep[len(fwd):]) if q]
    assert 0 < len(kf) + len(kr) < len(fwd) + len(rev)
    kept = eng.segment_coverage_thal(g, opt, kf, kr, 2, 3, chem, mode, thr)
    np.testing.assert_array_equal(kept["held"] == 2, whole["held"] == 2)
    np.testing.assert_array_equal(covered == 1, whole["held"] == 2)
    assert c_all == c_kept == int((whole["held"] == 2).sum()) == int(gains.sum())
    assert (whole["held"] == 1).any()        # segments with unstable matches only are not part of the promise


def test_unique_pairs_and_every_match_give_the_same_answer(m, eng, oracle, grid_input, grid_models):
    g, fwd, rev = grid_input
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    res = grid_models["ntthal", "any"]
    assert res["count"] == 130 and ttm.distinct_pairs(res) == 36
    assert eng.info("thin_thal_unique") in (0, 1)
    every = m.Engine(0)
    once = m.Engine(0)
    try:
        every.set_option("thin_thal_unique", 0)
        once.set_option("thin_thal_unique", 1)
        for chem_name, (chem, _) in chems(m, oracle).items():
            for mode in ("any", "end1"):
                for thr in (30.0, 40.0):
                    a = every.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, mode, thr)
                    b = once.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, mode, thr)
                    assert flat(a) == flat(b), (chem_name, mode, thr)
                    equal(b, tm.greedy(ttm.held_incidence(ctm.rethreshold(grid_models[chem_name, mode], thr))))
                    assert every.info("panel_thin_thal_matches") == once.info("panel_thin_thal_matches") == 130
                    assert every.info("panel_thin_thal_unique_pairs") == 130
                    assert once.info("panel_thin_thal_unique_pairs") == 36 < once.info("panel_thin_thal_matches")
        for bad in (2, -1, "x"):
            with pytest.raises(m.MsspeError):
                once.set_option("thin_thal_unique", bad)
    finally:
        every.close()
        once.close()


@pytest.fixture(scope="module")
def dense_case(m, oracle, oracle_tables):
    """test_gpu_coverage_thal.py::test_work_list_at_its_minimum's input: 43,216 matches, ten work lists of 2^12."""
    g = m.synth.aligned_genomes(24, 4000, seed=9)
    rng = np.random.default_rng(8)
    fwd, rev = primer_sets(rng, g, 30, 8)
    res = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, 8, fwd, rev, 3, 0, "any", 5.0, oracle.p3_args())
    return g, fwd, rev, res


@pytest.mark.parametrize("unique", [0, 1])
def test_slabs_accumulate_into_one_matrix(m, eng, dense_case, unique):
    g, fwd, rev, res = dense_case
    assert res["count"] == 43216
    H = ttm.held_incidence(res)
    assert 0 < H.sum() < (ttm.held_incidence(ctm.rethreshold(res, 0.0))).sum()
    want = tm.greedy(H)
    opt = m.KmerOpt(400, 170, 50, 8, 0, 0)
    chem = m.Chem.primer3()
    small = m.Engine(0)
    try:
        small.set_option("site_list_cap_log2", 12)
        small.set_option("thin_thal_unique", unique)
        equal(small.panel_thin_thal(g, opt, fwd, rev, 3, 0, chem, "any", 5.0), want)
        assert small.info("panel_thin_thal_redone") > 0 and small.info("panel_thin_thal_slabs") > 10
        assert small.info("panel_thin_thal_matches") == 43216
        pairs = small.info("panel_thin_thal_unique_pairs")   # per slab: the same pair in two slabs counts twice
        assert pairs == 43216 if not unique else ttm.distinct_pairs(res) <= pairs < 43216
        some = np.zeros(len(fwd) + len(rev), dtype=np.uint8)
        some[want[1][:2]] = 1
        equal(small.panel_thin_thal(g, opt, fwd, rev, 3, 0, chem, "any", 5.0, min_gain=2, forced=some, form="packed"),
              tm.greedy(H, 2, some))
    finally:
        small.close()
    eng.set_option("thin_thal_unique", unique)
    try:   # the default list holds it in one slab
        equal(eng.panel_thin_thal(g, opt, fwd, rev, 3, 0, chem, "any", 5.0), want)
        assert eng.info("panel_thin_thal_redone") == 0 and eng.info("panel_thin_thal_slabs") == 1
        if unique:
            assert eng.info("panel_thin_thal_unique_pairs") == ttm.distinct_pairs(res)
    finally:
        eng.set_option("thin_thal_unique", 1)


@pytest.mark.parametrize("unique", [0, 1])
def test_a_slab_split_by_primers(m, oracle, oracle_tables, unique):
    """One segment group, every position a match (M = k) and each word listed ten times: 10,320 matches of one group
    against a 2^12 list, which can only be split by primers; the duplicates' rows are equal, so every tie is there."""
    k = 10
    rng = np.random.default_rng(17)
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(1, 740))].copy()
    opt = m.KmerOpt(400, 170, 50, k, 0, 0)
    assert tm.n_partitions(740, 400, 170) == 3
    word = lambda col: bytes(g[0, col:col + k]).decode()
    f0 = [word(j * 170 + 4 + 9 * j) for j in range(3)] + ["".join("ACGT"[x] for x in rng.integers(0, 4, k))]
    r0 = [rc(word(j * 170 + 350 + 3 + 7 * j)) for j in range(3)] + ["".join("ACGT"[x] for x in rng.integers(0, 4, k))]
    fwd, rev = f0 * 10, r0 * 10     # each window's own word, its exact site in one segment, and a stranger
    base = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, k, fwd, rev, k, 0, "any", 0.0, oracle.p3_args(), cache={})
    assert base["count"] == 3 * 41 * 80
    tmax = np.maximum(base["matches"]["t"], 0.0)
    thr = float(np.sort(tmax)[-60]) / 2           # between the strongest duplexes and the bulk of mismatched ones
    res = ctm.rethreshold(base, thr)
    H = ttm.held_incidence(res)
    assert H.any() and not H.all() and len(tm.greedy(H)[1]) >= 2
    small = m.Engine(0)
    try:
        small.set_option("site_list_cap_log2", 12)
        small.set_option("thin_thal_unique", unique)
        equal(small.panel_thin_thal(g, opt, fwd, rev, k, 0, m.Chem.primer3(), "any", thr), tm.greedy(H))
        assert small.info("panel_thin_groups") == 1 and small.info("panel_thin_thal_redone") > 0
        assert small.info("panel_thin_thal_slabs") >= 3 and small.info("panel_thin_thal_matches") == base["count"]
    finally:
        small.close()


def split_threshold(t):
    tmax = np.maximum(t, 0.0)
    thr = float(np.median(tmax))
    return thr if thr > 0.0 else float(np.median(tmax[tmax > 0.0]))


@pytest.mark.parametrize("k", [8, 13, 16, 17, 31])
def test_lengths_on_every_route(m, eng, oracle, oracle_tables, k):
    g = m.synth.aligned_genomes(10, 2600)
    fwd, rev = primer_sets(np.random.default_rng(k), g, 40, k)
    opt = m.KmerOpt(400, 170, 50, k, 0, 0)
    base = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, k, fwd, rev, 2, 3, "end1", 0.0, oracle.ntthal_args())
    thr = split_threshold(base["matches"]["t"])
    res = ctm.rethreshold(base, thr)
    assert res["matches"]["stable"].any() and not res["matches"]["stable"].all()
    equal(eng.panel_thin_thal(g, opt, fwd, rev, 2, 3, m.Chem.ntthal(), "end1", thr), tm.greedy(ttm.held_incidence(res)))
    if k == 13:
        want = tm.greedy(ttm.held_incidence(res))
        for key, value in (("force_generic", 1), ("wave_kernel", 0)):
            e = m.Engine(0)
            try:
                e.set_option(key, value)
                for unique in (0, 1):
                    e.set_option("thin_thal_unique", unique)
                    equal(e.panel_thin_thal(g, opt, fwd, rev, 2, 3, m.Chem.ntthal(), "end1", thr), want, key)
            finally:
                e.close()


@pytest.mark.parametrize("n_seq,L,n_seg", [(1, 400, 1), (53, 450, 53), (6, 1760, 54)])
def test_group_edges(m, eng, oracle, oracle_tables, n_seq, L, n_seg):
    g = m.synth.aligned_genomes(n_seq, L, seed=n_seg)
    assert n_seq * tm.n_partitions(L, 400, 170) == n_seg
    fwd, rev = primer_sets(np.random.default_rng(n_seg), g, 30, 13)
    res = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, 13, fwd, rev, 2, 3, "any", 35.0, oracle.ntthal_args())
    equal(eng.panel_thin_thal(g, m.KmerOpt(400, 170, 50, 13, 0, 0), fwd, rev, 2, 3, m.Chem.ntthal(), "any", 35.0,
                              form="packed"), tm.greedy(ttm.held_incidence(res)))
    assert eng.info("panel_thin_groups") == -(-n_seg // 53)


def test_one_position_per_window_and_invalid_columns(m, eng, oracle, oracle_tables):
    g = m.synth.aligned_genomes(6, 3000, seed=7)
    for k in (13, 20):   # W == k
        rng = np.random.default_rng(2 * k)
        fwd = [bytes(g[r, c:c + k]).decode() for r, c in ((0, 0), (2, 150), (4, 300))] + draw_primers(rng, g, 10, k)
        rev = [rc(bytes(g[r, c + 300 - k:c + 300]).decode()) for r, c in ((1, 0), (3, 450))]
        fwd = [w for w in fwd if not set(w) - set("ACGT")]
        rev = [w for w in rev if not set(w) - set("ACGT")]
        res = ctm.coverage_thal(oracle_tables, g, 300, 150, k, k, fwd, rev, 2, 1, "end1", 30.0, oracle.ntthal_args())
        assert res["count"] >= 3
        equal(eng.panel_thin_thal(g, m.KmerOpt(300, 150, k, k, 0, 0), fwd, rev, 2, 1, m.Chem.ntthal(), "end1", 30.0),
              tm.greedy(ttm.held_incidence(res)))
    g = m.synth.aligned_genomes(8, 2600, seed=21).copy()
    rng = np.random.default_rng(21)
    fwd, rev = primer_sets(rng, g, 60, 13)
    clean = ctm.matches(g, 400, 170, 50, 13, fwd, rev, 2, 3)[0]
    P = (2600 - 400) // 170 + 1
    for i, r in enumerate(clean[::3]):   # a '-' or an N inside every third match's own columns
        s, q = int(r["segment"]), int(r["primer"])
        col = (s % P) * 170 + (350 if q >= len(fwd) else 0) + int(r["offset"]) + int(rng.integers(13))
        g[s // P, col] = ord("-N"[i % 2])
    res = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, 13, fwd, rev, 2, 3, "any", 35.0, oracle.ntthal_args())
    assert 0 < res["count"] < len(clean)
    for form in ("host", "packed"):
        equal(eng.panel_thin_thal(g, m.KmerOpt(400, 170, 50, 13, 0, 0), fwd, rev, 2, 3, m.Chem.ntthal(), "any", 35.0,
                                  form=form), tm.greedy(ttm.held_incidence(res)), form)


def test_capacity_statuses(m, eng):
    g = m.synth.aligned_genomes(40, 6000, seed=9)
    opt = m.KmerOpt(400, 60, 50, 13, 0, 0)
    fwd, rev = primer_sets(np.random.default_rng(9), g, 995, 13)   # 2,000 primers: 71 groups x 2,048 words
    chem = m.Chem.ntthal()
    default = eng.info("panel_thin_matrix_max_mb")
    eng.set_option("panel_thin_matrix_max_mb", 1)
    try:
        with pytest.raises(m.MsspeError) as e:
            eng.panel_thin_thal(g, opt, fwd, rev, 1, 3, chem, "any", 30.0)
        assert e.value.code == 5 and "needs 2 MB" in str(e.value) and "panel_thin_matrix_max_mb is 1" in str(e.value)
    finally:
        eng.set_option("panel_thin_matrix_max_mb", default)
    keep, order, gains, covered, c_all, c_kept = eng.panel_thin_thal(g, opt, fwd, rev, 1, 3, chem, "any", 30.0)
    whole = eng.segment_coverage_thal(g, opt, fwd, rev, 1, 3, chem, "any", 30.0)
    np.testing.assert_array_equal(covered == 1, whole["held"] == 2)
    assert c_all == c_kept == int(gains.sum()) and keep.sum() == order.size > 0
    small = m.Engine(0)
    try:   # one group against one primer beyond the list: 4,196 positions of one window all match at M = k
        small.set_option("site_list_cap_log2", 12)
        one = np.frombuffer(("ACGT" * 1100)[:4300].encode(), dtype=np.uint8)[None, :]
        with pytest.raises(m.MsspeError) as e:
            small.panel_thin_thal(one, m.KmerOpt(4300, 100, 4200, 5, 0, 0), ["ACGTA"], [], 5, 0, chem, "any", 5.0)
        assert e.value.code == 5 and "site_list_cap_log2" in str(e.value) and "4196" in str(e.value)
        g2 = m.synth.aligned_genomes(10, 2600, seed=53)   # ... and the context goes on
        f2, r2 = primer_sets(np.random.default_rng(1302), g2, 60, 13)
        o2 = m.KmerOpt(400, 170, 50, 13, 0, 0)
        assert flat(small.panel_thin_thal(g2, o2, f2, r2, 2, 3, chem, "any", 30.0)) == flat(
            eng.panel_thin_thal(g2, o2, f2, r2, 2, 3, chem, "any", 30.0))
    finally:
        small.close()


def test_argument_errors_and_empties(m, eng):
    L = m.load_library()
    g = m.synth.aligned_genomes(2, 1200, seed=1)
    n, Ln = g.shape
    w = m.pack_oligos(["ACGTACGTACGTA"])
    keep, order, gains = np.zeros(2, np.uint8), np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    picked = C.c_int(-1)
    chem0 = m.Chem.ntthal()

    def call(opt, mm, thin=m.ThinOpt(1), chem=chem0, mode=1, fw=w.ctypes.data, nf=1, rw=w.ctypes.data, nr=1,
             k=keep.ctypes.data, o=order.ctypes.data, ga=gains.ctypes.data, npk=C.byref(picked), seqs=g,
             fn=L.msspe_panel_thin_thal, n_seq=n, seq_len=Ln, forced=None, cov=None, c_all=None, c_kept=None):
        return fn(eng.ptr, seqs.ctypes.data if seqs is not None else None, n_seq, seq_len,
                  C.byref(opt) if opt is not None else None, C.byref(mm) if mm is not None else None,
                  C.byref(thin) if thin is not None else None, C.byref(chem) if chem is not None else None, mode, 30.0,
                  fw, nf, rw, nr, forced, k, o, ga, npk, cov, c_all, c_kept)

    ok, mm = m.KmerOpt(500, 250, 50, 13, 0, 0), m.MismatchOpt(1, 3)
    assert call(ok, mm) == 0 and picked.value >= 0
    assert call(ok, mm, mode=2) == 0
    assert call(ok, mm, mode=0) == 1 and call(ok, mm, mode=3) == 1 and call(ok, mm, chem=None) == 1
    assert "mode must be 1 (ANY) or 2 (END1)" in (call(ok, mm, mode=3), L.msspe_last_error(eng.ptr).decode())[1]
    assert call(ok, mm, thin=None) == 1 and call(ok, mm, thin=m.ThinOpt(0)) == 1 and call(ok, mm, thin=m.ThinOpt(-4)) == 1
    assert call(ok, mm, k=None) == 1 and call(ok, mm, o=None) == 1 and call(ok, mm, ga=None) == 1
    assert call(ok, mm, npk=None) == 1 and call(None, mm) == 1 and call(ok, None) == 1
    assert call(ok, mm, fw=None) == 1 and call(ok, mm, rw=None) == 1 and call(ok, mm, seqs=None) == 1
    assert call(ok, m.MismatchOpt(-1, 3)) == 1 and call(ok, m.MismatchOpt(14, 3)) == 1
    assert call(ok, m.MismatchOpt(1, 14)) == 1 and call(ok, m.MismatchOpt(1, -1)) == 1
    for k in (0, 1, 32):
        assert call(m.KmerOpt(500, 250, 50, k, 0, 0), m.MismatchOpt(0, 0)) == 2, k
    assert call(m.KmerOpt(500, 250, 10, 13, 0, 0), mm) == 1      # window < k
    assert call(m.KmerOpt(40, 250, 50, 13, 0, 0), mm) == 1       # segment < window
    assert call(m.KmerOpt(500, 0, 50, 13, 0, 0), mm) == 1        # stride < 1
    high = np.array([1 << 26], dtype=np.uint64)                  # a base past k = 13
    assert call(ok, mm, fw=high.ctypes.data) == 1 and call(ok, mm, rw=high.ctypes.data) == 1
    assert call(ok, mm, fn=L.msspe_panel_thin_thal_dev, seqs=None) == 1
    assert call(ok, mm, fn=L.msspe_panel_thin_thal_packed_dev, seqs=None) == 1
    # a window of more than 2^26 positions: an argument rule, shown with no records
    w5 = m.pack_oligos(["ACGTA"])
    big = lambda W: call(m.KmerOpt(W, 1, W, 5, 0, 0), m.MismatchOpt(0, 0), fw=w5.ctypes.data, rw=None, nr=0, n_seq=0,
                         seq_len=W)
    assert big((1 << 26) + 4) == 0 and big((1 << 26) + 5) == 1
    assert "2^26" in L.msspe_last_error(eng.ptr).decode()
    # empties, as msspe_panel_thin: keep = the forced flags, nothing picked, both counts 0, covered zeroed
    forced = np.array([0, 1], dtype=np.uint8)
    cov = np.full(16, 9, dtype=np.uint8)
    c_all, c_kept = C.c_longlong(7), C.c_longlong(7)
    for kw, opt in ((dict(fw=None, nf=0, rw=None, nr=0), ok), ({}, m.KmerOpt(5000, 250, 50, 13, 0, 0))):
        keep[:], picked.value, cov[:], c_all.value, c_kept.value = 9, -1, 9, 7, 7
        assert call(opt, mm, forced=forced.ctypes.data, cov=cov.ctypes.data, c_all=C.byref(c_all),
                    c_kept=C.byref(c_kept), **kw) == 0
        n_prim = kw.get("nf", 1) + kw.get("nr", 1)
        P = 0 if opt.segment_size > Ln else (Ln - opt.segment_size) // opt.overlap_size + 1
        assert keep[:n_prim].tolist() == forced[:n_prim].tolist() and picked.value == 0
        assert (c_all.value, c_kept.value) == (0, 0) and not cov[:n * P].any()
    gaps = np.full((4, 1500), ord("-"), dtype=np.uint8)
    got = eng.panel_thin_thal(gaps, m.KmerOpt(400, 170, 50, 13, 0, 0), ["ACGTACGTACGTA"], ["ACGTTGCAGGATC"], 2, 3, chem0,
                              "any", 30.0, forced=forced)
    assert got[0].tolist() == [0, 1] and got[1].size == 0 and got[4:] == (0, 0) and not got[3].any()
    for f, r in ((["ACGTACGTACGTA"], []), ([], ["ACGTTGCAGGATC"])):
        for form in ("host", "dev", "packed"):
            got = eng.panel_thin_thal(g, ok, f, r, 2, 3, chem0, "any", 30.0, form=form)
            assert got[0].shape == (1,) and got[1].size <= 1


def test_refused_tables(m, grid_input, tmp_path):
    g, fwd, rev = grid_input
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem = m.Chem.ntthal()
    eng = m.Engine(0, params_path=str(pv.write_bundle(pv.variant_sections("h_frac"), tmp_path / "h_frac.bundle")))
    try:
        for form in ("host", "dev", "packed"):
            for mode in ("any", "end1"):
                with pytest.raises(m.MsspeError) as e:
                    eng.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, mode, 30.0, form=form)
                assert e.value.code == 3 and "not integral" in str(e.value), (form, mode)
        keep, order, *_ = eng.panel_thin(g, opt, fwd, rev, 2, 3)   # needs no pair table: the context goes on
        assert order.size == 10
    finally:
        eng.close()


def test_shared_state_with_the_other_calls(m, grid_input):
    """The matrix and the round state are msspe_panel_thin's, the work list the background screen's, the plane words
    msspe_segment_coverage_thal's, the hand-over lists the pair screens': each call interleaved with this one on one
    engine gives what it gives on a fresh engine, and this call gives the same answer every time."""
    g, fwd, rev = grid_input
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem = m.Chem.ntthal()
    rng = np.random.default_rng(77)
    bg = ["".join(rng.choice(list("ACGT"), 6000)), bytes(g[0, :1500]).decode().replace("-", "N")]
    pool = m.synth.pool_strings(m.synth.random_pool(64, 13))
    g2 = m.synth.aligned_genomes(6, 1760, seed=54)
    f2, r2 = primer_sets(np.random.default_rng(54), g2, 30, 13)

    def calls(e):
        new = lambda: e.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, "end1", 30.0)
        return [new,
                lambda: e.panel_thin(g, opt, fwd, rev, 2, 3),
                new,
                lambda: e.segment_coverage_thal(g, opt, fwd, rev, 2, 3, chem, "end1", 30.0, matches=True),
                lambda: e.panel_thin_thal(g2, opt, f2, r2, 2, 3, chem, "any", 35.0, form="packed"),
                lambda: e.background_thal(bg, fwd[:20] + rev[:20], 2, 3, chem, 30.0, mode="any", capacity=1 << 16),
                new,
                lambda: e.cross_dimer(pool, chem, -9000.0, want_dg=True),
                new,
                lambda: e.panel_thin(g2, opt, f2, r2, 2, 3)]

    one = m.Engine(0)
    try:
        chained = [flat(c()) for c in calls(one)]
    finally:
        one.close()
    for i in range(len(chained)):
        fresh = m.Engine(0)
        try:
            assert flat(calls(fresh)[i]()) == chained[i], f"call {i} depends on the calls before it"
        finally:
            fresh.close()
    assert chained[0] == chained[2] == chained[6] == chained[8] and chained[0] != chained[1]


# ---- the CLI ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_fasta(m, tmp_path_factory):
    g = np.concatenate([m.synth.aligned_genomes(20, 6000, seed=700 + j) for j in range(2)])
    fa = tmp_path_factory.mktemp("thin_thal_cli") / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    return fa, g


def run_cli(fa, csv, *extra):
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rows = [l.split(",") for l in Path(csv).read_text().splitlines()[1:] if l]
    return r.stdout, rows


def block_of(out):
    at = out.index("\nPanel thinning")
    return "".join(l + "\n" for l in out[at:].split("\n")[:4])


def thal_held(out):
    at = out.index("Coverage report (thal ")
    return int(re.search(r"Segments:\s+(\d+)/\d+ held", out[at:]).group(1))


COV = ("--coverage-mismatches", "2", "--coverage-tm", "30")


def cli_case(oracle, oracle_tables, fa, g, tmp_path, extra, panel=((), ()), mode="any"):
    base_out, base = run_cli(fa, tmp_path / "a.csv", *extra, *COV)
    assert "Panel thinning" not in base_out
    flags = ("--thin-panel", "true", "--thin-mismatches", "2", "--thin-tm", "30") + (
        ("--thin-thal", mode) if mode != "any" else ())
    out, rows = run_cli(fa, tmp_path / "b.csv", *extra, *COV, *flags)
    fwd = [r[2] for r in base if r[0] == "F"]
    rev = [r[2] for r in base if r[0] == "R"]
    all_f, all_r = fwd + list(panel[0]), rev + list(panel[1])
    forced = np.array([0] * len(fwd) + [1] * len(panel[0]) + [0] * len(rev) + [1] * len(panel[1]), dtype=np.uint8)
    res = ctm.coverage_thal(oracle_tables, g, 500, 250, 50, 13, all_f, all_r, 2, 3, mode, 30.0, oracle.ntthal_args())
    H = ttm.held_incidence(res)
    keep, order, gains, covered, c_all, c_kept, _ = tm.greedy(H, 1, forced)
    kf = [w for w, q in zip(fwd, keep[:len(fwd)]) if q]
    kr = [w for w, q in zip(rev, keep[len(all_f):len(all_f) + len(rev)]) if q]
    assert [r[2] for r in rows if r[0] == "F"] == kf and [r[2] for r in rows if r[0] == "R"] == kr
    assert 0 < len(kf) + len(kr) < len(fwd) + len(rev)
    block = ttm.render_block(mode, 30.0, 2, 3, 1, len(kf), len(fwd), len(kr), len(rev), int(forced.sum()), c_all, c_kept,
                             g.shape[0] * tm.n_partitions(g.shape[1], 500, 250))
    assert block_of(out) == block
    if mode == "any":   # the report right above scores with the same mode: it holds what the block says, and what
        assert thal_held(out) == c_kept == c_all == thal_held(base_out)   # the whole panel held without the switch
    return base, rows, out


def test_cli_thins_on_the_held_segments(oracle, oracle_tables, small_fasta, tmp_path):
    fa, g = small_fasta
    base, rows, out = cli_case(oracle, oracle_tables, fa, g, tmp_path, ())
    stats = {r[2]: r[3:] for r in base}
    assert all(stats[r[2]] == r[3:] for r in rows)   # a survivor's row is what it was
    assert out.index("Coverage report (thal") < out.index("Panel thinning (thal ANY, t >= 30.00 C; matches within 2 mism")
    cli_case(oracle, oracle_tables, fa, g, tmp_path, (), mode="end1")
    # without --thin-tm the thinning and its block are the string rule's, byte for byte, whatever --thin-thal says
    plain = run_cli(fa, tmp_path / "c.csv", *COV, "--thin-panel", "true", "--thin-mismatches", "2")
    ignored = run_cli(fa, tmp_path / "d.csv", *COV, "--thin-panel", "true", "--thin-mismatches", "2", "--thin-thal",
                      "end1")
    assert plain == ignored and "\nPanel thinning (up to 2 mismatches, last 3 bases exact, gain >= 1):\n" in plain[0]
    fwd = [r[2] for r in base if r[0] == "F"]
    rev = [r[2] for r in base if r[0] == "R"]
    keep, _, _, _, c_all, c_kept, _ = tm.greedy(tm.incidence(g, 500, 250, 50, 13, fwd, rev, 2, 3))
    assert block_of(plain[0]) == tm.render_block(2, 3, 1, int(keep[:len(fwd)].sum()), len(fwd),
                                                 int(keep[len(fwd):].sum()), len(rev), 0, c_all, c_kept,
                                                 g.shape[0] * tm.n_partitions(g.shape[1], 500, 250))
    # ... and without --thin-panel true none of the values is read
    off = run_cli(fa, tmp_path / "e.csv", *COV, "--thin-tm", "30", "--thin-thal", "end1")
    assert off[0] == run_cli(fa, tmp_path / "f.csv", *COV)[0] and off[1] == base


def test_cli_with_existing_primers(oracle, oracle_tables, small_fasta, tmp_path):
    fa, g = small_fasta
    _, first = run_cli(fa, tmp_path / "first.csv")
    panel_rows = [r for r in first if r[0] == "F"][:4] + [r for r in first if r[0] == "R"][:4]
    panel = tmp_path / "panel.csv"
    panel.write_text("direction,name,primers,gc,avg,std,tm\n" + "".join(",".join(r) + "\n" for r in panel_rows))
    pf = [r[2] for r in panel_rows if r[0] == "F"]
    pr = [r[2] for r in panel_rows if r[0] == "R"]
    _, rows, out = cli_case(oracle, oracle_tables, fa, g, tmp_path, ("--existing-primers", str(panel)), (pf, pr))
    assert not {r[2] for r in rows} & set(pf + pr)
    assert ", 8 forced\n" in out


def test_cli_with_tubes(oracle, oracle_tables, small_fasta, tmp_path):
    fa, g = small_fasta
    base, rows, out = cli_case(oracle, oracle_tables, fa, g, tmp_path, ("--tubes", "4"))
    tube = {r[2]: r[7] for r in base}
    assert all(tube[r[2]] == r[7] for r in rows)     # survivors keep their tube numbers
    per_tube = [l for l in out[out.index("Tube assignment"):].splitlines() if l.startswith("  Tube ")]
    assert sum(int(l.split()[2]) for l in per_tube) == len([r for r in rows if r[7]])
