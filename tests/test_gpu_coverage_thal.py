"""msspe_segment_coverage_thal* on the device against its restatement (tests/coverage_thal_model.py: the numpy match
model, the CPU oracle's thal, the background screen's stable rule).  Everything is exact: integers equal, doubles
bit-equal to the oracle.  Chemistries, modes, thresholds, oligo lengths on every scoring route, the three entry points,
the sibling's invariants, short and long windows, several LDS tiles, invalid columns, the work list at its minimum,
the caller's capacity, the context's shared state, argument errors and the CLI's --coverage-tm block."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import coverage_thal_model as ctm
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
    fwd = draw_primers(rng, g, n, k, **kw)
    rev = [rc(w) for w in draw_primers(rng, g, n, k, **kw)]
    return fwd, rev


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(got, want, records=True):
    np.testing.assert_array_equal(got["held"], want["held"])
    np.testing.assert_array_equal(bits(got["t_best"]), bits(want["t_best"]))
    np.testing.assert_array_equal(got["primer_segments"], want["primer_segments"])
    np.testing.assert_array_equal(got["primer_held"], want["primer_held"])
    if records:
        assert got["count"] == want["count"]
        a, b = got["matches"], want["matches"]
        for f in ("primer", "segment", "offset", "mismatches", "stable"):
            np.testing.assert_array_equal(a[f], b[f], err_msg=f)
        for f in ("dg", "t"):
            np.testing.assert_array_equal(bits(a[f]), bits(b[f]), err_msg=f)


@pytest.fixture(scope="module")
def grid_input(m):
    g = m.synth.aligned_genomes(10, 2600, seed=53)
    rng = np.random.default_rng(1302)
    fwd, rev = primer_sets(rng, g, 60, 13)
    return g, fwd, rev


@pytest.mark.parametrize("chem_name", ["ntthal", "primer3"])
@pytest.mark.parametrize("mode", ["any", "end1"])
def test_grid_equals_the_model(m, eng, oracle, oracle_tables, grid_input, chem_name, mode):
    g, fwd, rev = grid_input
    chem, args = chems(m, oracle)[chem_name]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    cache = {}
    for f, r in ((fwd, rev), ([], rev), (fwd, []), ([], [])):
        base = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, 13, f, r, 2, 3, mode, 30.0, args, cache=cache)
        for thr in (30.0, 40.0):
            want = ctm.rethreshold(base, thr)
            got = eng.segment_coverage_thal(g, opt, f, r, 2, 3, chem, mode, thr, matches=True)
            same(got, want)
            same(eng.segment_coverage_thal(g, opt, f, r, 2, 3, chem, mode, thr), want, records=False)
            if f and r:   # 130 matches in 77 of the 130 segments; 69 / 44 of them held (ntthal), 62 / 40 (primer3)
                assert want["count"] == 130 and set(np.unique(want["held"]).tolist()) == {0, 1, 2}
                assert int((want["held"] != 0).sum()) == 77
                assert int((want["held"] == 2).sum()) == {("ntthal", 30.0): 69, ("ntthal", 40.0): 44,
                                                          ("primer3", 30.0): 62, ("primer3", 40.0): 40}[chem_name, thr]


def split_threshold(t):
    """A threshold both stable and unstable matches exist at: the median t_match -- of the matches above 0 where the
    median of all is 0 (k = 8: most mismatched 8-mers form nothing above 0 C, and a threshold of 0 holds everything)."""
    tm = np.maximum(t, 0.0)
    thr = float(np.median(tm))
    return thr if thr > 0.0 else float(np.median(tm[tm > 0.0]))


@pytest.mark.parametrize("k", [8, 13, 16, 17, 24, 31])
def test_lengths_on_every_route(m, eng, oracle, oracle_tables, k):
    g = m.synth.aligned_genomes(10, 2600)
    rng = np.random.default_rng(k)
    fwd, rev = primer_sets(rng, g, 40, k)
    opt = m.KmerOpt(400, 170, 50, k, 0, 0)
    base = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, k, fwd, rev, 2, 3, "end1", 0.0, oracle.ntthal_args())
    thr = split_threshold(base["matches"]["t"])
    want = ctm.rethreshold(base, thr)
    stable = want["matches"]["stable"]
    assert stable.any() and not stable.all()
    same(eng.segment_coverage_thal(g, opt, fwd, rev, 2, 3, m.Chem.ntthal(), "end1", thr, matches=True), want)


@pytest.mark.parametrize("k", [13, 20])
def test_routes_give_identical_bits(m, eng, oracle, oracle_tables, k):
    g = m.synth.aligned_genomes(10, 2600)
    rng = np.random.default_rng(k)
    fwd, rev = primer_sets(rng, g, 40, k)
    opt = m.KmerOpt(400, 170, 50, k, 0, 0)
    want = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, k, fwd, rev, 2, 3, "any", 35.0, oracle.ntthal_args())
    assert want["count"] > 50
    same(eng.segment_coverage_thal(g, opt, fwd, rev, 2, 3, m.Chem.ntthal(), "any", 35.0, matches=True), want)
    for key, value in (("force_generic", 1), ("wave_kernel", 0)):
        e = m.Engine(0)
        try:
            e.set_option(key, value)
            same(e.segment_coverage_thal(g, opt, fwd, rev, 2, 3, m.Chem.ntthal(), "any", 35.0, matches=True), want)
        finally:
            e.close()


@pytest.mark.parametrize("k", [13, 24])
def test_entry_points_agree(m, eng, k):
    g = m.synth.aligned_genomes(20, 5000, seed=3)
    rng = np.random.default_rng(5)
    fwd, rev = primer_sets(rng, g, 80, k)
    opt = m.KmerOpt(500, 250, 50, k, 0, 0)
    chem = m.Chem.ntthal()
    host = eng.segment_coverage_thal(g, opt, fwd, rev, 2, 3, chem, "end1", 30.0, matches=True)
    assert host["count"] > 50
    for form in ("dev", "packed"):
        same(eng.segment_coverage_thal(g, opt, fwd, rev, 2, 3, chem, "end1", 30.0, matches=True, packed=form), host)
    hp = eng.put_rows_packed(g)
    try:   # a resident alignment, as the CLI calls it
        same(eng.segment_coverage_thal((hp, g.shape[0], g.shape[1]), opt, fwd, rev, 2, 3, chem, "end1", 30.0,
                                       matches=True, packed="packed"), host)
    finally:
        eng.device_free(hp)


def test_invariants_through_the_sibling(m, eng, oracle, oracle_tables, grid_input):
    g, fwd, rev = grid_input
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem = m.Chem.ntthal()
    best, counts = eng.segment_coverage_mm(g, opt, fwd, rev, 2, 3, per_primer=True)
    got = eng.segment_coverage_thal(g, opt, fwd, rev, 2, 3, chem, "any", 40.0, matches=True)
    np.testing.assert_array_equal(got["held"] != 0, best != 255)
    np.testing.assert_array_equal(got["primer_segments"], counts)
    assert (got["primer_held"] <= got["primer_segments"]).all()
    for thr in (0.0, -5.0):   # a threshold <= 0 makes every match stable
        zero = eng.segment_coverage_thal(g, opt, fwd, rev, 2, 3, chem, "any", thr, matches=True)
        assert set(np.unique(zero["held"]).tolist()) == {0, 2}
        np.testing.assert_array_equal(zero["primer_held"], zero["primer_segments"])
        assert zero["matches"]["stable"].all()
    exact = eng.segment_coverage_thal(g, opt, fwd, rev, 0, 0, chem, "any", 40.0, matches=True)
    assert exact["count"] > 20 and not exact["matches"]["mismatches"].any()
    primers = fwd + rev
    for r in exact["matches"]:   # M = 0: the template is the primer's reverse complement, in either direction
        u = primers[int(r["primer"])]
        res = oracle.thal(oracle_tables, u, ctm.revcomp(u), oracle.ANY, oracle.ntthal_args())
        assert not res.no_structure and bits(r["t"]) == bits(res.t) and bits(r["dg"]) == bits(res.dG)


def test_one_position_per_window(m, eng, oracle, oracle_tables):
    g = m.synth.aligned_genomes(6, 3000, seed=7)
    for k in (13, 20):
        rng = np.random.default_rng(2 * k)
        fwd = [bytes(g[r, c:c + k]).decode() for r, c in ((0, 0), (2, 150), (4, 300))] + draw_primers(rng, g, 10, k)
        rev = [rc(bytes(g[r, c + 300 - k:c + 300]).decode()) for r, c in ((1, 0), (3, 450))]
        fwd = [w for w in fwd if not set(w) - set("ACGT")]
        rev = [w for w in rev if not set(w) - set("ACGT")]
        want = ctm.coverage_thal(oracle_tables, g, 300, 150, k, k, fwd, rev, 2, 1, "end1", 30.0, oracle.ntthal_args())
        assert want["count"] >= 3 and not want["matches"]["offset"].any()
        same(eng.segment_coverage_thal(g, m.KmerOpt(300, 150, k, k, 0, 0), fwd, rev, 2, 1, m.Chem.ntthal(), "end1",
                                       30.0, matches=True), want)


def test_long_window_counts_segments_not_positions(m, eng, oracle, oracle_tables):
    """k = 5, W = 2,100: one segment per block, several rounds of positions, and every primer matches at many
    positions of a segment; the per-primer counts stay segment counts."""
    g = m.synth.aligned_genomes(2, 2400, seed=7)
    rng = np.random.default_rng(5)
    fwd, rev = primer_sets(rng, g, 6, 5, subs_max=0, random_extra=0)
    opt = m.KmerOpt(2100, 150, 2100, 5, 0, 0)
    base = ctm.coverage_thal(oracle_tables, g, 2100, 150, 2100, 5, fwd, rev, 1, 1, "any", 0.0, oracle.ntthal_args(),
                             chunk=2)
    recs = base["matches"]
    cells = {}
    for r in recs:
        cells[int(r["primer"]), int(r["segment"])] = cells.get((int(r["primer"]), int(r["segment"])), 0) + 1
    assert base["count"] > 1000 and max(cells.values()) >= 10
    assert int(base["primer_segments"].sum()) == len(cells) and base["primer_segments"].max() <= g.shape[0] * 3
    for thr in (0.0, 10.0):   # 5-mers score 0: all stable at 0, none at 10
        same(eng.segment_coverage_thal(g, opt, fwd, rev, 1, 1, m.Chem.ntthal(), "any", thr, matches=True),
             ctm.rethreshold(base, thr))


def test_more_primers_than_one_tile(m, eng, oracle, oracle_tables):
    """The listing kernel's tile holds 2,048 64-bit primer words: matches on both sides of the tile boundary, in
    both directions."""
    k = 17
    g = m.synth.aligned_genomes(3, 1500, seed=11)
    rng = np.random.default_rng(k)
    fwd, rev = primer_sets(rng, g, 2300, k, subs_max=2, random_extra=50)
    want = ctm.coverage_thal(oracle_tables, g, 300, 150, 40, k, fwd, rev, 2, 3, "end1", 45.0, oracle.ntthal_args(),
                             chunk=4)
    p = want["matches"]["primer"].astype(np.int64)
    n_f = len(fwd)
    assert n_f > 2048 and ((p < 2048).any() and ((p >= 2048) & (p < n_f)).any() and
                           ((p >= n_f) & (p < n_f + 2048)).any() and (p >= n_f + 2048).any())
    same(eng.segment_coverage_thal(g, m.KmerOpt(300, 150, 40, k, 0, 0), fwd, rev, 2, 3, m.Chem.ntthal(), "end1", 45.0,
                                   matches=True), want)


def test_invalid_columns_inside_windows(m, eng, oracle, oracle_tables):
    g = m.synth.aligned_genomes(8, 2600, seed=21).copy()
    rng = np.random.default_rng(21)
    fwd, rev = primer_sets(rng, g, 60, 13)
    clean = ctm.matches(g, 400, 170, 50, 13, fwd, rev, 2, 3)[0]
    P = (2600 - 400) // 170 + 1
    for i, r in enumerate(clean[::3]):   # a '-' or an N inside every third match's own columns
        s, q = int(r["segment"]), int(r["primer"])
        col = (s % P) * 170 + (350 if q >= len(fwd) else 0) + int(r["offset"]) + int(rng.integers(13))
        g[s // P, col] = ord("-N"[i % 2])
    want = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, 13, fwd, rev, 2, 3, "any", 35.0, oracle.ntthal_args())
    assert 0 < want["count"] < len(clean)
    for form in ("host", "packed"):
        same(eng.segment_coverage_thal(g, m.KmerOpt(400, 170, 50, 13, 0, 0), fwd, rev, 2, 3, m.Chem.ntthal(), "any",
                                       35.0, matches=True, packed=form), want)


def test_work_list_at_its_minimum(m, eng):
    """2^12 entries and more than ten times as many matches: slabs are split by groups and by primers, and every
    output is what the default list gives."""
    g = m.synth.aligned_genomes(24, 4000, seed=9)
    rng = np.random.default_rng(8)
    fwd, rev = primer_sets(rng, g, 30, 8)
    opt = m.KmerOpt(400, 170, 50, 8, 0, 0)
    chem = m.Chem.primer3()
    want = eng.segment_coverage_thal(g, opt, fwd, rev, 3, 0, chem, "any", 5.0, matches=True)
    assert want["count"] > 40000 and eng.info("coverage_thal_redone") == 0
    assert eng.info("coverage_thal_matches") == want["count"] and eng.info("coverage_thal_slabs") == 1
    small = m.Engine(0)
    try:
        small.set_option("site_list_cap_log2", 12)
        same(small.segment_coverage_thal(g, opt, fwd, rev, 3, 0, chem, "any", 5.0, matches=True), want)
        assert small.info("coverage_thal_redone") > 0 and small.info("coverage_thal_slabs") > 10
        assert small.info("coverage_thal_matches") == want["count"]
        # one group against one primer beyond the list: 4,196 positions of one window all match at M = k
        one = np.frombuffer(("ACGT" * 1100)[:4300].encode(), dtype=np.uint8)[None, :]
        with pytest.raises(m.MsspeError) as e:
            small.segment_coverage_thal(one, m.KmerOpt(4300, 100, 4200, 5, 0, 0), ["ACGTA"], [], 5, 0, chem, "any", 5.0)
        assert e.value.code == 5 and "site_list_cap_log2" in str(e.value) and "4196" in str(e.value)
        # ... and the context goes on: the same call as before, the same answer
        same(small.segment_coverage_thal(g, opt, fwd, rev, 3, 0, chem, "any", 5.0, matches=True), want)
    finally:
        small.close()


def test_callers_capacity(m, eng, grid_input):
    g, fwd, rev = grid_input
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem = m.Chem.ntthal()
    full = eng.segment_coverage_thal(g, opt, fwd, rev, 2, 3, chem, "any", 30.0, matches=True)
    n = full["count"]
    assert n == 130
    keys = {(int(r["primer"]), int(r["segment"]), int(r["offset"])): r for r in full["matches"]}
    for cap in (0, 1, n - 1):
        with pytest.raises(m.MsspeError) as e:
            eng.segment_coverage_thal(g, opt, fwd, rev, 2, 3, chem, "any", 30.0, matches=True, capacity=cap)
        assert e.value.code == 5 and e.value.count == n and len(e.value.matches) == cap
        same(e.value.result, full, records=False)
        kept = e.value.matches   # the first arrivals, sorted: each one a record of the full list
        order = [(int(r["primer"]), int(r["segment"]), int(r["offset"])) for r in kept]
        assert order == sorted(order) and len(set(order)) == cap
        for key, r in zip(order, kept):
            assert r.tobytes() == keys[key].tobytes()
        same(eng.segment_coverage_thal(g, opt, fwd, rev, 2, 3, chem, "any", 30.0, matches=True,
                                       capacity=e.value.count), full)


def test_shared_state_with_the_other_calls(m, grid_input):
    """The work list, the site pool and the hand-over lists are the background screen's and the pair screens': this
    call, background_thal, cross_dimer and this call again on one engine, each against a fresh engine."""
    g, fwd, rev = grid_input
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem = m.Chem.ntthal()
    rng = np.random.default_rng(77)
    bg = ["".join(rng.choice(list("ACGT"), 6000)), bytes(g[0, :1500]).decode().replace("-", "N")]
    pool = m.synth.pool_strings(m.synth.random_pool(64, 13))

    def calls(e):
        return [lambda: e.segment_coverage_thal(g, opt, fwd, rev, 2, 3, chem, "end1", 30.0, matches=True),
                lambda: e.background_thal(bg, fwd[:20] + rev[:20], 2, 3, chem, 30.0, mode="any", capacity=1 << 16),
                lambda: e.cross_dimer(pool, chem, -9000.0, want_dg=True),
                lambda: e.segment_coverage_thal(g, opt, fwd, rev, 2, 3, chem, "end1", 30.0, matches=True)]

    def flat(x):
        vals = x.values() if isinstance(x, dict) else x
        return [np.asarray(v).tobytes() for v in vals if isinstance(v, (np.ndarray, int))]

    one = m.Engine(0)
    try:
        chained = [flat(c()) for c in calls(one)]
    finally:
        one.close()
    for i in range(4):
        fresh = m.Engine(0)
        try:
            assert flat(calls(fresh)[i]()) == chained[i], f"call {i} depends on the calls before it"
        finally:
            fresh.close()
    assert chained[0] == chained[3] and len(chained[1]) >= 4 and len(chained[2]) >= 2


def test_argument_errors_and_empties(m, eng):
    L = m.load_library()
    g = m.synth.aligned_genomes(2, 1200, seed=1)
    n, Ln = g.shape
    w = m.pack_oligos(["ACGTACGTACGTA"])
    held = np.full(16, 9, dtype=np.uint8)
    tb = np.full(16, 9.0)
    cnt = np.full((2, 2), 7, dtype=np.uint32)
    recs = np.zeros(4, dtype=ctm.SCORED_MATCH_DTYPE)
    count = C.c_uint64(99)
    chem = m.Chem.ntthal()
    mm = m.MismatchOpt(1, 3)

    def call(opt, mm=mm, fw=w.ctypes.data, nf=1, rw=w.ctypes.data, nr=1, chem=chem, mode=1, out=held.ctypes.data,
             seqs=g, lst=None, cnt_out=None, fn=L.msspe_segment_coverage_thal, ctx=eng.ptr):
        return fn(ctx, seqs.ctypes.data if seqs is not None else None, n, Ln,
                  C.byref(opt) if opt is not None else None, C.byref(mm) if mm is not None else None, fw, nf, rw, nr,
                  C.byref(chem) if chem is not None else None, mode, 30.0, out, tb.ctypes.data, cnt[0].ctypes.data,
                  cnt[1].ctypes.data, lst, 4 if lst else 0, cnt_out)

    ok = m.KmerOpt(500, 250, 50, 13, 0, 0)
    assert call(ok) == 0
    assert call(ok, lst=recs.ctypes.data, cnt_out=C.byref(count)) == 0 and count.value == 0
    assert call(None) == 1 and call(ok, mm=None) == 1 and call(ok, chem=None) == 1 and call(ok, out=None) == 1
    assert call(ok, fw=None) == 1 and call(ok, rw=None) == 1 and call(ok, seqs=None) == 1
    assert call(ok, mode=0) == 1 and call(ok, mode=3) == 1 and call(ok, mode=2) == 0
    assert call(ok, lst=recs.ctypes.data) == 1                                  # a list without count_out
    assert call(ok, mm=m.MismatchOpt(-1, 3)) == 1 and call(ok, mm=m.MismatchOpt(14, 3)) == 1
    assert call(ok, mm=m.MismatchOpt(1, -1)) == 1 and call(ok, mm=m.MismatchOpt(1, 14)) == 1
    for k in (0, 1, 32):
        assert call(m.KmerOpt(500, 250, 50, k, 0, 0), mm=m.MismatchOpt(0, 0)) == 2
    assert call(m.KmerOpt(500, 250, 10, 13, 0, 0)) == 1      # window < k
    assert call(m.KmerOpt(40, 250, 50, 13, 0, 0)) == 1       # segment < window
    assert call(m.KmerOpt(500, 0, 50, 13, 0, 0)) == 1        # stride < 1
    high = np.array([1 << 26], dtype=np.uint64)              # a base past k = 13
    assert call(ok, fw=high.ctypes.data) == 1 and call(ok, rw=high.ctypes.data) == 1
    assert call(ok, ctx=None) == 1
    for fn in (L.msspe_segment_coverage_thal_dev, L.msspe_segment_coverage_thal_packed_dev):
        assert call(ok, seqs=None, fn=fn) == 1
    # no primers / no segments: OK, every output zeroed, count 0
    for kw, opt in ((dict(fw=None, nf=0, rw=None, nr=0), ok), ({}, m.KmerOpt(5000, 250, 50, 13, 0, 0))):
        held[:], tb[:], cnt[:], count.value = 9, 9.0, 7, 99
        assert call(opt, lst=recs.ctypes.data, cnt_out=C.byref(count), **kw) == 0
        P = 0 if opt.segment_size > Ln else (Ln - opt.segment_size) // opt.overlap_size + 1
        n_prim = kw.get("nf", 1) + kw.get("nr", 1)
        assert not held[:n * P].any() and not tb[:n * P].any() and count.value == 0
        assert not cnt[:, :n_prim].any()


def test_refused_tables_and_a_non_stock_table(m, oracle, grid_input, tmp_path):
    """The table gating of every dimer call: a stack enthalpy that is no integer (param_variants' h_frac) makes all
    three forms MSSPE_ERR_TABLES with "not integral", nothing is written, and the context goes on serving a call
    that needs no pair table; tables the engine does compute with (h_mod10: the dense kernel alone) give the oracle's
    bits under the same tables."""
    g, fwd, rev = grid_input
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem = m.Chem.ntthal()
    eng = m.Engine(0, params_path=str(pv.write_bundle(pv.variant_sections("h_frac"), tmp_path / "h_frac.bundle")))
    try:
        hp = eng.put_rows_packed(g)
        try:
            for form, aln in (("host", g), ("dev", g), ("packed", g), ("packed", (hp, g.shape[0], g.shape[1]))):
                for mode in ("any", "end1"):
                    with pytest.raises(m.MsspeError) as e:
                        eng.segment_coverage_thal(aln, opt, fwd, rev, 2, 3, chem, mode, 30.0, matches=True,
                                                  capacity=256, packed=form)
                    assert e.value.code == 3 and "not integral" in str(e.value), (form, mode)
                    assert e.value.count == 0 and not e.value.result["held"].any()
                    assert not e.value.result["primer_segments"].any() and not e.value.result["t_best"].any()
        finally:
            eng.device_free(hp)
        best, counts = eng.segment_coverage_mm(g, opt, fwd, rev, 2, 3, per_primer=True)   # needs no pair table
        assert int((best != 255).sum()) == 77 and int(counts.sum()) > 0
    finally:
        eng.close()
    path = pv.write_bundle(pv.variant_sections("h_mod10"), tmp_path / "h_mod10.bundle")
    tables = oracle.Tables(path)
    eng = m.Engine(0, params_path=str(path))
    try:
        stock = ctm.coverage_thal(oracle.Tables(), g, 400, 170, 50, 13, fwd, rev, 2, 3, "end1", 30.0,
                                  oracle.ntthal_args())
        want = ctm.coverage_thal(tables, g, 400, 170, 50, 13, fwd, rev, 2, 3, "end1", 30.0, oracle.ntthal_args())
        assert (bits(want["matches"]["t"]) != bits(stock["matches"]["t"])).any()   # the tables do change the scores
        same(eng.segment_coverage_thal(g, opt, fwd, rev, 2, 3, chem, "end1", 30.0, matches=True), want)
    finally:
        eng.close()


def test_a_window_beyond_the_offset_field_is_an_argument_error(m, eng):
    """Offsets travel in 26 bits: a window of 2^26 positions is the largest taken, one more is MSSPE_ERR_ARG.  The
    rule is an argument rule, so it shows without an alignment of that size: the calls are made with no records."""
    L = m.load_library()
    w = m.pack_oligos(["ACGTA"])
    held = np.zeros(4, dtype=np.uint8)
    chem, mm = m.Chem.ntthal(), m.MismatchOpt(0, 0)
    g = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)[None, :]

    def call(W, seq_len):
        opt = m.KmerOpt(W, 1, W, 5, 0, 0)
        return L.msspe_segment_coverage_thal(eng.ptr, g.ctypes.data, 0, seq_len, C.byref(opt), C.byref(mm),
                                             w.ctypes.data, 1, None, 0, C.byref(chem), 1, 30.0, held.ctypes.data, None,
                                             None, None, None, 0, None)

    # no records (n_seq 0): the argument rules run, nothing is uploaded or read
    assert call((1 << 26) + 4, (1 << 26) + 4) == 0          # 2^26 positions: offsets 0 .. 2^26 - 1 fit
    assert call((1 << 26) + 5, (1 << 26) + 5) == 1          # one more
    assert "2^26" in L.msspe_last_error(eng.ptr).decode()


@pytest.fixture(scope="module")
def small_fasta(m, tmp_path_factory):
    g = np.concatenate([m.synth.aligned_genomes(30, 9000, seed=500 + j) for j in range(2)])
    fa = tmp_path_factory.mktemp("thal_cli") / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    return fa, g


def run_cli(fa, csv, *extra, ok=True):
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                       capture_output=True, text=True, timeout=600)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr
    return r.stdout, Path(csv).read_bytes()


def test_cli_block(m, oracle, oracle_tables, small_fasta, tmp_path):
    fa, g = small_fasta
    base_out, base_csv = run_cli(fa, tmp_path / "a.csv", "--coverage-mismatches", "2", "--coverage-3p-exact", "3")
    ignored = run_cli(fa, tmp_path / "b.csv", "--coverage-mismatches", "2", "--coverage-3p-exact", "3",
                      "--coverage-thal", "end1")   # without --coverage-tm the mode is not read
    assert ignored == (base_out, base_csv)
    out, csv = run_cli(fa, tmp_path / "c.csv", "--coverage-mismatches", "2", "--coverage-3p-exact", "3",
                       "--coverage-tm", "35", "--coverage-thal", "end1")
    assert csv == base_csv and out.startswith(base_out)
    rows = [l.split(",") for l in csv.decode().splitlines()[1:] if l]
    fwd = [r[2] for r in rows if r[0] == "F"]
    rev = [r[2] for r in rows if r[0] == "R"]
    want = ctm.coverage_thal(oracle_tables, g, 500, 250, 50, 13, fwd, rev, 2, 3, "end1", 35.0, oracle.ntthal_args())
    block = ctm.render([f"g{i}" for i in range(len(g))], [g.shape[1]] * len(g), want["held"], want["primer_held"],
                       500, 250, 2, 3, "end1", 35.0)
    assert out[len(base_out):] == block
    assert "Coverage report (thal END1, t >= 35.00 C; matches within 2 mismatches, last 3 bases exact):" in block
    r = run_cli(fa, tmp_path / "d.csv", "--coverage-tm", "35", "--devices", "0", ok=False)
    assert r.returncode == 2 and "'--coverage-tm' runs on one device" in r.stderr
