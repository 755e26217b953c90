"""msspe_panel_thin_reach* on the device against the model (tests/panel_thin_reach_model.py: one boolean array per
primer): keep, order, gains, n_picked, every primer's own reach, both counts and every field of every record, exactly;
the records also against msspe_stream_reach on the kept words, the site counts against it on the whole panel.  Planted
near-copies in both modes and chemistries and with a template flank, interval and record geometry, the greedy rule, the sizes at which a carry or
a buffer takes another step, one context across calls, the edge calls and the CLI."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import background_model as bm
import background_thal_model as btm
import panel_thin_reach_model as trm
import stream_reach_model as srm
import test_gpu_stream_reach as tsr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"
TILE = 4096


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


def assert_thin_equal(got, want, what=""):
    for f in ("keep", "order", "gains", "primer_reach"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what}: {f}")
    assert (got["reached_all"], got["reached_kept"]) == (want["reached_all"], want["reached_kept"]), what
    if "counts" in want:
        np.testing.assert_array_equal(got["counts"], want["counts"], err_msg=f"{what}: counts")
        np.testing.assert_array_equal(got["stable"], want["stable"], err_msg=f"{what}: stable")
    tsr.assert_records_equal(got["records"], want["records"], what)


def check(eng, records, primers, M, E, chem, mode, thr, D, want, min_gain=1, forced=None, cross=True, flank=0):
    """One host call against the model, and against stream_reach: the kept words' records, the whole panel's counts."""
    what = f"{mode} thr {thr} D {D} min_gain {min_gain}" + (f" flank {flank}" if flank else "")
    got = eng.panel_thin_reach(records, primers, M, E, chem, thr, mode, D, min_gain=min_gain, forced=forced, flank=flank)
    print(f"{what}: kept {int(got['keep'].sum())} of {len(primers)}, {len(got['order'])} picks, reached "
          f"{got['reached_kept']} of {got['reached_all']}, {eng.info('thin_reach_sites')} sites, "
          f"{eng.info('thin_reach_intervals')} intervals, {eng.info('thin_reach_rounds')} rounds")
    np.testing.assert_array_equal(got["starts"], bm.record_starts(records)[0])
    assert_thin_equal(got, want, what)
    assert eng.info("thin_reach_sites") == int(want["stable"].sum())
    assert eng.info("thin_reach_intervals") <= eng.info("thin_reach_sites")
    # the picks and the round that stopped; without an interval no round runs
    assert eng.info("thin_reach_rounds") == (len(want["order"]) + 1 if eng.info("thin_reach_intervals") else 0)
    if cross:
        k = len(primers[0])
        kept = [p for p, f in zip(primers, got["keep"]) if f]
        _c, _s, recs, _st = eng.stream_reach(records, kept, M, E, chem, thr, mode, D, k=k, flank=flank)
        tsr.assert_records_equal(got["records"], recs, what + " (stream_reach on the kept words)")
        c, s, whole, _st = eng.stream_reach(records, primers, M, E, chem, thr, mode, D, flank=flank)
        np.testing.assert_array_equal(got["counts"], c)
        np.testing.assert_array_equal(got["stable"], s)
        if min_gain == 1:   # the guarantee on its own
            assert got["reached_kept"] == got["reached_all"] == int(whole["reached_either"].sum())
            np.testing.assert_array_equal(got["records"]["reached_either"], whole["reached_either"])
    return got


def site_want(k, sites, counts, records, n, D, min_gain=1, forced=None):
    want = trm.thin_of_sites(k, sites, records, n, D, min_gain, forced)
    want["counts"] = want["stable"] = counts
    return want


# ---- planted near-copies --------------------------------------------------------------------------------------------
def planted(rng, k, n, M, E):
    primers = [tsr.random_seq(rng, k) for _ in range(n)]
    records = tsr.plant(rng, [tsr.random_seq(rng, 9000), tsr.random_seq(rng, 4099), tsr.random_seq(rng, 700)], primers,
                        6, M, E)
    records.insert(2, "")
    return primers, records


@pytest.mark.parametrize("chem_name", ["ntthal", "primer3"])
@pytest.mark.parametrize("mode", ["any", "end1"])
@pytest.mark.parametrize("k,n", [(13, 24), (20, 40)])
def test_planted_scored(m, eng, oracle, oracle_tables, k, n, mode, chem_name):
    rng = np.random.default_rng(4000 + k)
    M, E = 2, 2
    primers, records = planted(rng, k, n, M, E)
    chem, args = tsr.chems(m, oracle)[chem_name]
    scored = btm.scored_sites(oracle_tables, records, primers, M, E, mode, 30.0, args)
    # a threshold from the oracle's own doubles with sites on both sides: the median t_site as its "%.2f" float32
    mid = float(np.float32(oracle.round_fixed_f32(float(np.median(np.maximum(scored[2]["t"], 0.0))), 2)))
    s = tsr.restable(scored, n, mid)
    assert 0 < s[1].sum() < s[0].sum()
    stable_sites = s[2][s[2]["stable"] != 0]
    for D in tsr.reaches(k):
        want = trm.thin_of_sites(k, stable_sites, records, n, D)
        want["counts"], want["stable"] = s[0], s[1]
        got = check(eng, records, primers, M, E, chem, mode, mid, D, want, cross=D in (k, 500))
    assert len(got["order"]) >= 1 and got["reached_all"] > 0


# ---- planted near-copies, scored with a template flank --------------------------------------------------------------
def check_flanked_thin(eng, chem, case, k, f, mode, D=500):
    """panel_thin_reach at flank f against the model on the flanked sites (the input and the threshold of
    test_gpu_stream_reach.flank_case) at min_gain 1 and 3 and once with a forced primer; the flank must show in every
    primer's own reach."""
    records, primers, M, E, thr, flips, blunt, flanked = case
    n = len(primers)
    assert flips >= 5 and 0 < flanked[1].sum() < flanked[0].sum()
    forced = np.zeros(n, dtype=np.uint8)
    forced[n - 1] = 1
    for min_gain, forced_now in ((1, None), (3, None), (1, forced)):
        want = trm.thin(None, records, primers, M, E, mode, thr, D, min_gain, forced_now, scored=flanked)
        got = check(eng, records, primers, M, E, chem, mode, thr, D, want, min_gain, forced_now, flank=f)
    assert len(got["order"]) >= 1 and got["reached_all"] > 0
    at_flank_0 = trm.thin(None, records, primers, M, E, mode, thr, D, scored=blunt)
    assert (want["primer_reach"] != at_flank_0["primer_reach"]).any()


@pytest.mark.parametrize("mode", ["any", "end1"])
@pytest.mark.parametrize("k,f", [(13, 2), (20, 4)])
def test_planted_scored_with_a_flank(m, eng, oracle, oracle_tables, k, f, mode):
    case = tsr.flank_case(oracle, oracle_tables, "stock", k, f, mode)
    check_flanked_thin(eng, m.Chem.ntthal(), case, k, f, mode)


def test_flanked_thin_on_both_sides_of_wave_max_k(m, oracle, tmp_path):
    """The stack_x3 tables of tests/param_variants.py (one wave per pair up to 28 bases), k = 24 and flank 4: one
    thinning call whose template classes are scored on different routes."""
    import param_variants as pv
    k, f, mode = 24, 4, "any"
    path = pv.write_bundle(pv.variant_sections("stack_x3"), tmp_path / "stack_x3.bundle")
    wave_max_k = m.capi.host_table_routes(path)["wave_max_k"]
    case = tsr.flank_case(oracle, oracle.Tables(path), "stack_x3", k, f, mode, truncated=True)
    lengths = tsr.template_lengths(case, k, f)
    assert k < wave_max_k < k + 2 * f and (lengths <= wave_max_k).any() and (lengths > wave_max_k).any()
    e = m.Engine(0, params_path=str(path))
    try:
        check_flanked_thin(e, m.Chem.ntthal(), case, k, f, mode)
    finally:
        e.close()


@pytest.mark.parametrize("k,n", [(13, 24), (13, 40), (20, 24), (20, 40)])
def test_planted_every_site_stable(m, eng, k, n):
    rng = np.random.default_rng(4100 + k + n)
    M, E = 2, 2
    primers, records = planted(rng, k, n, M, E)
    counts, sites = bm.sites(records, primers, M, E)
    chem = m.Chem.ntthal()
    for D in tsr.reaches(k):
        got = check(eng, records, primers, M, E, chem, "any", 0.0, D, site_want(k, sites, counts, records, n, D),
                    cross=D in (k, 64))
        if D == k and n == 40:
            assert len(got["order"]) > 16                     # more picks than one batch of rounds
    forced = (rng.integers(0, 4, n) == 0).astype(np.uint8)
    assert 0 < forced.sum() < n
    for min_gain in (1, 2, 1000):
        for f in (None, forced):
            check(eng, records, primers, M, E, chem, "any", 0.0, 65,
                  site_want(k, sites, counts, records, n, 65, min_gain, f), min_gain, f)


# ---- interval geometry ----------------------------------------------------------------------------------------------
F12, V12, PAL, POLY = "GATTACAGATTC", "CCATGGTTACGA", "ACGTACGTACGT", "A" * 12


def put(body, at, word):
    assert at >= 0 and at + len(word) <= len(body)
    return body[:at] + word + body[at + len(word):]


def interval_records(rng, D):
    """Exact sites of four 12-mers placed for the interval code: word and tile edges, both clips, the nested case, one
    primer's sites 1, D - 1, D and D + 1 apart, a palindrome."""
    k = 12
    rv = bm.revcomp(V12)
    body = lambda n: tsr.random_seq(rng, n, "CGT")            # no A: POLY has no accidental site
    recs = []
    r = body(3 * TILE + 70)                                    # the stream's first record: positions are columns
    r = put(r, 64, F12)                                        # lo' at bit 0; with D = 64 hi at bit 63
    r = put(r, 63 + 128, F12)                                  # lo' at bit 63
    r = put(r, 320 + 63 - (k - 1), rv)                         # a minus interval's hi at bit 63
    r = put(r, 448 - (k - 1) + D - 1 if D <= 64 else 448, rv)  # ... its lo' at bit 0 of word 7 where D fits a few words
    r = put(r, 640 + 2, V12)                                   # D = 12 .. 14: inside one word
    r = put(r, TILE - 5, F12)                                  # over the tile boundary
    r = put(r, 2 * TILE - 1 - (k - 1) + 3, rv)                 # a minus interval down over a tile boundary
    r = put(r, 2 * TILE + 1000, POLY + "A")                    # POLY's sites 1 apart
    recs.append(r)
    if D <= 1000:                                              # F12's sites D - 1, D and D + 1 apart
        chain, at = body(4 * D + 200), 10
        for step in ([D - 1] if D - 1 >= k else []) + [D, D + 1]:
            chain = put(chain, at, F12)
            at += step
        recs.append(put(chain, at, F12))
    recs.append(F12 + body(20) + rv)                           # D above the record: both clips
    recs.append(F12 + "T" + bm.revcomp(F12) + "TT")            # a clipped plus interval holds a minus interval
    recs.append(body(30) + PAL + body(30))                     # both strands at one position
    recs.append("")
    recs.append(PAL)
    return recs


@pytest.mark.parametrize("D", [12, 13, 14, 63, 64, 65, 500, 1 << 20])
def test_interval_geometry(m, eng, D):
    rng = np.random.default_rng(31)
    primers = [F12, V12, PAL, POLY]
    records = interval_records(rng, D)
    counts, sites = bm.sites(records, primers, 0, 0)
    assert counts[2, 0] == counts[2, 1] >= 2 and counts[3, 0] >= 2 and (counts.sum(axis=1) > 0).all()
    assert counts[0, 1] >= 1 and counts[1, 1] >= 3
    for forced in (None, [0, 0, 1, 0]):
        check(eng, records, primers, 0, 0, m.Chem.ntthal(), "any", 0.0, D,
              site_want(12, sites, counts, records, 4, D, 1, forced), 1, forced)


@pytest.mark.parametrize("D", tsr.reaches(13))
def test_record_geometry(m, eng, D):
    """The records of the reach tests: boundaries at multiples of 64 and of the tile, minus one, plus zero and plus
    one, records shorter than k, empty records, several records in one word."""
    rng = np.random.default_rng(11)
    k, f, v = 13, "GATTACAGATTCC", "CCATGGTTACGAT"
    records = tsr.geometry_records(rng, k, f, v)
    primers = [v, f, v]                                        # the duplicate: the same intervals twice
    counts, sites = bm.sites(records, primers, 0, 0)
    check(eng, records, primers, 0, 0, m.Chem.ntthal(), "any", 0.0, D, site_want(k, sites, counts, records, 3, D))
    check(eng, records, primers, 0, 0, m.Chem.ntthal(), "any", 0.0, D,
          site_want(k, sites, counts, records, 3, D, 2, [0, 0, 1]), 2, [0, 0, 1], cross=False)


# ---- the greedy rule ------------------------------------------------------------------------------------------------
def test_greedy_rule(m, eng):
    u, v, w = "AACCGGATCAGTC", "GATTCCAGGACTA", "ACCGGATCAGTCT"      # w is u moved on by one base
    chem = m.Chem.ntthal()

    def run(records, primers, D, min_gain=1, forced=None):
        counts, sites = bm.sites(records, primers, 0, 0)
        return check(eng, records, primers, 0, 0, chem, "any", 0.0, D,
                     site_want(13, sites, counts, records, len(primers), D, min_gain, forced), min_gain, forced)

    tie = [u + "T" * 30 + v + "T" * 30]
    for primers in ([u, v], [v, u]):
        got = run(tie, primers, 13)
        assert got["order"].tolist() == [0, 1] and got["gains"].tolist() == [13, 13]
    got = run(tie, [u, v, u], 20)                                   # the duplicated word
    assert got["keep"].tolist() == [1, 1, 0] and got["primer_reach"].tolist() == [20, 20, 20]
    whole = [u + "TT" + bm.revcomp(v)]                               # forced alone covers everything
    got = run(whole, [u, v], 28, forced=[1, 0])
    assert got["order"].tolist() == [] and got["keep"].tolist() == [1, 0] and got["reached_kept"] == 28
    got = run(whole, [u, v], 28, forced=[1, 1])
    assert got["order"].tolist() == []
    step = [u + "T" + "C" * 20]                                      # w adds one column to u
    assert run(step, [u, w], 13, 1)["gains"].tolist() == [13, 1]
    assert run(step, [u, w], 13, 2)["keep"].tolist() == [1, 0]
    assert run(step, [u, w], 13, 1000)["keep"].tolist() == [0, 0]
    got = run(["CCCC" * 50, "", "GGGT" * 20], [u, v], 500)           # a panel with no site at all
    assert got["order"].tolist() == [] and got["reached_all"] == 0 and eng.info("thin_reach_sites") == 0
    got = run(["CCCC" * 50], [u, v], 500, forced=[0, 1])
    assert got["keep"].tolist() == [0, 1] and got["reached_kept"] == 0


# ---- larger sizes ---------------------------------------------------------------------------------------------------
def test_more_tiles_than_one_scan_step(m, eng):
    """About 5 x 10^6 columns: the reach report's tile carry takes its second step there, and the cover's rank tiles
    (1024 words each) pass their 64th.  The records of the reach test of the same name."""
    rng = np.random.default_rng(23)
    k, f, v = 13, "GATTACAGATTCC", "CCATGGTTACGAT"
    rv = bm.revcomp(v)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    body = lambda n: acgt[rng.integers(0, 4, size=n, dtype=np.uint8)].tobytes().decode()
    long = body(635 * TILE + 77)
    long = long[:100] + f + long[100 + k:300] + rv + long[300 + k:-400] + f + long[-400 + k:-50] + rv + long[-50 + k:]
    mid = list(body(290 * TILE))
    for a in range(1000, len(mid) - 2 * k, 37 * TILE + 5):
        mid[a:a + k] = f
        mid[a + 700:a + 700 + k] = rv
    across = body(200 * TILE + 3)
    across = across[:10] + f + across[10 + k:-30] + rv + across[-30 + k:]
    records = [long, "".join(mid), across, f + body(90 * TILE) + rv, "", body(50)]
    assert bm.record_starts(records)[1] > 1100 * TILE
    counts, sites = bm.sites(records, [f, v], 0, 0)
    for D in (500, 1 << 20):
        check(eng, records, [f, v], 0, 0, m.Chem.ntthal(), "any", 0.0, D, site_want(k, sites, counts, records, 2, D),
              cross=D == 500)


def test_key_buffer_growth_and_context_reuse(m, oracle, oracle_tables):
    rng = np.random.default_rng(41)
    primers = [tsr.random_seq(rng, 13) for _ in range(24)]
    records = tsr.plant(rng, [tsr.random_seq(rng, 40000), tsr.random_seq(rng, 20000)], primers, 6, 3, 2)
    chem, args = tsr.chems(m, oracle)["ntthal"]
    M, E = 4, 0
    counts, sites = bm.sites(records, primers, M, E)
    assert counts.sum() > 2 * 1024
    want = site_want(13, sites, counts, records, 24, 500)
    small = tsr.plant(rng, [tsr.random_seq(rng, 6000), tsr.random_seq(rng, 3000)], primers, 4, 2, 2)
    scored = btm.scored_sites(oracle_tables, small, primers, 2, 2, "any", 25.0, args)
    assert 0 < scored[1].sum() < scored[0].sum()
    want_small = trm.thin_of_sites(13, scored[2][scored[2]["stable"] != 0], small, 24, 300)
    want_small["counts"], want_small["stable"] = scored[0], scored[1]
    e = m.Engine(0)
    try:
        e.set_option("amplicon_keys_cap_log2", 10)
        check(e, records, primers, M, E, chem, "any", 0.0, 500, want)
        assert e.info("amplicon_key_grows") > 0 and e.info("thin_reach_sites") == int(counts.sum())
        for key in ("thin_reach_prepare_us", "thin_reach_gain0_us", "thin_reach_rounds_us", "thin_reach_report_us"):
            assert e.info(key) >= 0
        # a smaller call behind the larger one, other calls of the same buffers in between
        check(e, small, primers, 2, 2, chem, "any", 25.0, 300, want_small)
        assert e.info("amplicon_key_grows") == 0
        e.background_amplicons(small, primers, 2, 2, chem, 25.0, "any", 40, 400)
        check(e, small, primers, 2, 2, chem, "any", 25.0, 300, want_small)
        e.stream_reach(records, primers, M, E, chem, 0.0, "any", 65)
        check(e, records, primers, M, E, chem, "any", 0.0, 500, want)
        got = e.panel_thin_reach(small, primers, 2, 2, chem, 25.0, "any", 300, want_records=False)
        assert got["records"] is None
        for f in ("keep", "order", "gains", "primer_reach"):
            np.testing.assert_array_equal(got[f], want_small[f])
    finally:
        e.close()


# ---- edge calls -----------------------------------------------------------------------------------------------------
def test_null_record_start_is_one_record(m, eng):
    rng = np.random.default_rng(11)
    k, f, v = 13, "GATTACAGATTCC", "CCATGGTTACGAT"
    records = tsr.geometry_records(rng, k, f, v)
    chem = m.Chem.ntthal()
    counts, sites = bm.sites(records, [f, v], 0, 0)
    one = ["-".join(records)]
    d, total_len, d_starts = eng.put_stream_packed(records)
    try:
        for D in (13, 500):
            got = eng.panel_thin_reach_packed(d, total_len, [f, v], 0, 0, chem, 0.0, "any", D, record_start=d_starts)
            assert_thin_equal(got, site_want(k, sites, counts, records, 2, D), f"packed D {D}")
            got = eng.panel_thin_reach_packed(d, total_len, [f, v], 0, 0, chem, 0.0, "any", D)
            assert len(got["records"]) == 1
            assert_thin_equal(got, site_want(k, sites, counts, one, 2, D), f"one record D {D}")
    finally:
        eng.device_free(d)


def test_no_primers_and_a_stream_shorter_than_k(m, eng):
    chem = m.Chem.ntthal()
    records = ["ACGTACGTACGTACGTACGTACGT", "", "ACGTA"]
    got = eng.panel_thin_reach(records, [], 1, 1, chem, 30.0, "any", 100, k=13)
    assert got["keep"].shape == (0,) and len(got["order"]) == 0 and got["reached_all"] == got["reached_kept"] == 0
    none = np.zeros(0, dtype=bm.SITE_DTYPE)
    tsr.assert_records_equal(got["records"], srm.reach_of_sites(13, none, records, 100), "n == 0")
    short = ["ACGT", "", "ACGTAC"]                                       # 12 columns in all
    got = eng.panel_thin_reach(short, ["ACGTACGTACGTA", "ACGTACGTACGTT"], 1, 1, chem, 30.0, "any", 100, forced=[0, 1])
    assert got["keep"].tolist() == [0, 1] and len(got["order"]) == 0 and got["counts"].sum() == 0
    assert got["reached_all"] == got["reached_kept"] == 0 and got["primer_reach"].tolist() == [0, 0]
    tsr.assert_records_equal(got["records"], srm.reach_of_sites(13, none, short, 100), "total_len < k")


def test_argument_errors(m, eng):
    import ctypes as C
    from msspe_amd.capi import REACH_RECORD_DTYPE, MismatchOpt, ReachOpt, ThinOpt
    records, chem, primers = ["ACGTACGTACGTACGTACGTACGT"], m.Chem.ntthal(), ["ACGTACGTACGTA"]
    for D in (12, 0, 1 << 31, (1 << 32) - 1):                                   # reach outside [k, 2^31)
        with pytest.raises(m.MsspeError) as e:
            eng.panel_thin_reach(records, primers, 1, 1, chem, 30.0, "any", D)
        assert e.value.code == 1
    for min_gain in (0, -1):
        with pytest.raises(m.MsspeError) as e:
            eng.panel_thin_reach(records, primers, 1, 1, chem, 30.0, "any", 100, min_gain=min_gain)
        assert e.value.code == 1
    for bad_m, bad_e in ((14, 0), (0, 14)):                                     # the scored call's errors
        with pytest.raises(m.MsspeError) as e:
            eng.panel_thin_reach(records, primers, bad_m, bad_e, chem, 30.0, "any", 100)
        assert e.value.code == 1
    for k in (1, 32):
        with pytest.raises(m.MsspeError) as e:
            eng.panel_thin_reach(records, np.zeros(1, dtype=np.uint64), 0, 0, chem, 30.0, "any", 100, k=k)
        assert e.value.code == 2
    with pytest.raises(m.MsspeError) as e:
        eng.panel_thin_reach(records, primers, 1, 1, chem, 30.0, 3, 100)          # mode
    assert e.value.code == 1
    with pytest.raises(m.MsspeError) as e:
        eng.panel_thin_reach(records, primers, 1, 1, chem, 30.0, "any", 100, flank=5)
    assert e.value.code == 1
    mm, opt, thin = MismatchOpt(1, 1), ReachOpt(100), ThinOpt(1)
    out, words = (C.c_uint64 * 2)(), (C.c_uint64 * 1)(0)
    keep, order, gains = (C.c_uint8 * 1)(), (C.c_uint32 * 1)(), (C.c_uint32 * 1)()
    picked, a, b = C.c_int(0), C.c_longlong(0), C.c_longlong(0)
    recs = np.zeros(2, dtype=REACH_RECORD_DTYPE)
    L = eng.L
    d, total_len, _starts = eng.put_stream_packed(["ACGTACGTACGTACGTACGT", "ACGTACGTACGTACGT"])
    try:
        def call(opt_p=C.byref(opt), thin_p=C.byref(thin), keep_p=keep, order_p=order, gains_p=gains,
                 picked_p=C.byref(picked), starts=None, n_starts=0):
            return L.msspe_panel_thin_reach_packed_dev(
                eng.ptr, C.c_void_p(d), total_len, 13, C.byref(mm), words, 1, C.byref(chem), 1, 30.0, 0, opt_p, thin_p,
                None, starts, n_starts, keep_p, order_p, gains_p, picked_p, None, C.byref(a), C.byref(b), out, out,
                recs.ctypes.data)
        assert call() == 0
        for bad in (dict(opt_p=None), dict(thin_p=None), dict(keep_p=None), dict(order_p=None), dict(gains_p=None),
                    dict(picked_p=None)):
            assert call(**bad) == 1, bad
        for bad in ([0, 21, 21], [5, 3], [1, 21], [0, total_len + 1]):    # not ascending / not from 0 / beyond the stream
            arr = np.array(bad, dtype=np.uint64)
            assert call(starts=arr.ctypes.data, n_starts=len(bad)) == 1, bad
        arr = np.array([0, 21], dtype=np.uint64)
        assert call(starts=arr.ctypes.data, n_starts=2) == 0
        assert call(starts=arr.ctypes.data, n_starts=0) == 1
    finally:
        eng.device_free(d)


# ---- the CLI --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_inputs(m, tmp_path_factory):
    g = m.synth.aligned_genomes(24, 7000, seed=700)
    d = tmp_path_factory.mktemp("thin_reach_cli")
    fa = d / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    names = [f"g{i}" for i in range(len(g))]
    genomes = [bytes(r).decode().replace("-", "") for r in g]
    return fa, names, genomes


def test_cli_blocks_and_csv(cli_inputs, tmp_path, oracle, oracle_tables):
    fa, names, genomes = cli_inputs
    base_out, base_csv = tsr.run_cli(fa, tmp_path / "a.csv")
    words = tsr.csv_words(base_csv)
    assert words and all(len(w) == 13 for w in words)
    # without --thin-reach nothing changes
    plain_out, plain_csv = tsr.run_cli(fa, tmp_path / "p.csv", "--reach", "500")
    off_out, off_csv = tsr.run_cli(fa, tmp_path / "q.csv", "--reach", "500", "--thin-reach", "false")
    assert plain_csv == off_csv == base_csv and plain_out == off_out
    _c, _s, recs = srm.reach(None, genomes, words, 2, 3, "any", 0.0, 500)
    assert plain_out == base_out + srm.render(names, genomes, recs, 500, 2, 3)
    # the string rule with the defaults, M = 2 and E = 3
    out, csv = tsr.run_cli(fa, tmp_path / "b.csv", "--reach", "500", "--thin-reach", "true", "--reach-out",
                           str(tmp_path / "r.csv"))
    res = trm.thin(None, genomes, words, 2, 3, "any", 0.0, 500)
    assert out == base_out + trm.render(res, 500, 1, 2, 3) + srm.render(names, genomes, res["records"], 500, 2, 3)
    assert (tmp_path / "r.csv").read_text() == srm.render_csv(names, genomes, res["records"])
    assert tsr.csv_words(csv) == [w for w, f in zip(words, res["keep"]) if f]
    assert 0 < res["keep"].sum() < len(words) and res["reached_kept"] == res["reached_all"]
    print(out[len(base_out):])
    # scored, END1 at 30 C under the screen's chemistry, another rule, reach and min gain
    args = oracle.ntthal_args(mv=50.0, dv=3.0, dntp=0.0, dna_conc=250.0, temp_c=25.0)
    out, csv = tsr.run_cli(fa, tmp_path / "c.csv", "--reach", "64", "--reach-tm", "30", "--reach-thal", "end1",
                           "--reach-mismatches", "1", "--reach-3p-exact", "2", "--thin-reach", "true",
                           "--thin-reach-min-gain", "40", "--reach-out", str(tmp_path / "s.csv"))
    res = trm.thin(oracle_tables, genomes, words, 1, 2, "end1", 30.0, 64, 40, None, args)
    assert out == (base_out + trm.render(res, 64, 40, 1, 2, "end1", 30.0) +
                   srm.render(names, genomes, res["records"], 64, 1, 2, "end1", 30.0))
    assert (tmp_path / "s.csv").read_text() == srm.render_csv(names, genomes, res["records"])
    assert tsr.csv_words(csv) == [w for w, f in zip(words, res["keep"]) if f]
    assert res["stable"].sum() > 0
