"""msspe_stream_reach* on the device against the model (tests/stream_reach_model.py: one boolean array per record):
every field of every record, exactly, and sites_out / stable_out equal to msspe_background_thal's.  Planted near-copies
in both modes and chemistries at a threshold that splits the sites, the same with a template flank at the threshold
where the flank changes most stable flags (and on tables whose wave kernel ends inside the templates' lengths), every
site stable, every reach from k to beyond the stream, record and tile geometry, the plumbing options, argument errors and the CLI's block."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import background_flank_model as bfm
import background_model as bm
import background_thal_model as btm
import stream_reach_model as srm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"
TILE = 4096


def reaches(k):
    return [k, k + 1, 63, 64, 65, 500, 1 << 20]


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    assert e.info("reach_tile_columns") == TILE
    yield e
    e.close()


def random_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n)) if n else ""


def chems(m, oracle):
    return {"ntthal": (m.Chem.ntthal(), oracle.ntthal_args()), "primer3": (m.Chem.primer3(), oracle.p3_args())}


def near_copy(rng, p, max_subs, keep_3p):
    w = list(p)
    for q in rng.choice(len(p) - keep_3p, int(rng.integers(0, max_subs + 1)), replace=False):
        w[q] = "ACGT"[int(rng.integers(0, 4))]
    return "".join(w)


def plant(rng, records, primers, copies, max_subs, keep_3p):
    """The idiom of tests/test_gpu_background_amplicons.py: `copies` near-copies of every primer, every other one as
    its reverse complement, at random places."""
    recs = [list(r) for r in records]
    k = len(primers[0])
    for i, p in enumerate(primers):
        for c in range(copies):
            w = near_copy(rng, p, max_subs, keep_3p)
            if (i + c) % 2:
                w = bm.revcomp(w)
            r = recs[int(rng.integers(0, len(recs)))]
            a = int(rng.integers(0, len(r) - k + 1))
            r[a:a + k] = w
    return ["".join(r) for r in recs]


def assert_records_equal(got, want, what=""):
    assert got.shape == want.shape, what
    for f in srm.FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert not len(bad), (f"{what}: {f} differs in {len(bad)} records, first {int(bad[0])}: device "
                              f"{got[bad[0]]} model {want[bad[0]]}")


def check(eng, records, primers, M, E, chem, mode, thr, D, counts, stable, want, thal=None, flank=0):
    """One host call against the model's records and the scored call's counts."""
    g_counts, g_stable, recs, starts = eng.stream_reach(records, primers, M, E, chem, thr, mode, D, flank=flank)
    np.testing.assert_array_equal(g_counts, counts)
    np.testing.assert_array_equal(g_stable, stable)
    np.testing.assert_array_equal(starts, bm.record_starts(records)[0])
    assert_records_equal(recs, want, f"{mode} thr {thr} D {D}")
    if thal is not None:
        np.testing.assert_array_equal(g_counts, thal[0])
        np.testing.assert_array_equal(g_stable, thal[1])
    return recs


def restable(scored, n, thr):
    counts, _stable, recs = scored
    recs = recs.copy()
    recs["stable"] = [btm.is_stable(float(t), thr) for t in recs["t"]]
    return counts, btm.stable_counts(n, recs), recs


# ---- planted near-copies, scored ------------------------------------------------------------------------------------
@pytest.mark.parametrize("chem_name", ["ntthal", "primer3"])
@pytest.mark.parametrize("mode", ["any", "end1"])
@pytest.mark.parametrize("k", [13, 20])
def test_planted_scored(m, eng, oracle, oracle_tables, k, mode, chem_name):
    rng = np.random.default_rng(3000 + k)
    M, E = 2, 2
    primers = [random_seq(rng, k) for _ in range(24)]
    records = plant(rng, [random_seq(rng, 9000), random_seq(rng, 4099), random_seq(rng, 700)], primers, 6, M, E)
    records.insert(2, "")
    chem, args = chems(m, oracle)[chem_name]
    scored = btm.scored_sites(oracle_tables, records, primers, M, E, mode, 30.0, args)
    n = len(primers)
    # a threshold from the oracle's own doubles with sites on both sides: the median t_site as its "%.2f" float32
    mid = float(np.float32(oracle.round_fixed_f32(float(np.median(np.maximum(scored[2]["t"], 0.0))), 2)))
    s = restable(scored, n, mid)
    assert 0 < s[1].sum() < s[0].sum()
    thal = eng.background_thal(records, primers, M, E, chem, mid, mode)
    for D in reaches(k):
        want = srm.reach_of_scored(k, s[2], records, D)
        check(eng, records, primers, M, E, chem, mode, mid, D, s[0], s[1], want, thal)
    print(f"k {k} {mode} {chem_name} thr {mid}: {int(s[0].sum())} sites, {int(s[1].sum())} stable")
    assert want["reached_either"].sum() > 0 and (want["sites_plus"] > 0).any() and (want["sites_minus"] > 0).any()


# ---- planted near-copies, scored with a template flank --------------------------------------------------------------
FLANK_GRID = [(13, 1), (13, 2), (20, 4), (24, 4)]
_flank_cases = {}


def flank_input(k, truncate=0):
    """The input of test_planted_scored with 10 copies of each primer.  truncate = f: written over the first record
    every 180 columns, exact copies whose flanks an N cuts short at every distance 0 .. f on either side, on both
    strands and of one primer after the other, so that templates of every length k .. k + 2 f occur (planted copies
    alone have whole flanks)."""
    rng = np.random.default_rng(3100 + k)
    M, E = 2, 2
    primers = [random_seq(rng, k) for _ in range(24)]
    records = plant(rng, [random_seq(rng, 9000), random_seq(rng, 4099), random_seq(rng, 700)], primers, 10, M, E)
    records.insert(2, "")
    if truncate:
        first, q = list(records[0]), 0
        for dl in range(truncate + 1):
            for dr in range(truncate + 1):
                for s in (0, 1):
                    p = primers[q % len(primers)]
                    piece = "N" + random_seq(rng, dl) + (bm.revcomp(p) if s else p) + random_seq(rng, dr) + "N"
                    first[180 * q + 10:180 * q + 10 + len(piece)] = piece
                    q += 1
        assert 180 * q <= len(first)
        records[0] = "".join(first)
    return records, primers, M, E


def flank_threshold(oracle, t_blunt, t_flanked):
    """(threshold, flips): among the "%.2f" float32 values of the flanked t_site, the one at which most sites are
    stable at one of flank 0 and flank f and not at the other (the lowest of equals); only thresholds that leave
    stable and unstable sites at either flank are looked at.  (None, 0) without one."""
    r0 = np.array([oracle.round_fixed_f32(float(t), 2) for t in np.maximum(t_blunt, 0.0)])
    rf = np.array([oracle.round_fixed_f32(float(t), 2) for t in np.maximum(t_flanked, 0.0)])
    best = (None, 0)
    for thr in sorted({float(np.float32(x)) for x in rf}):
        s0, sf = ~(r0 < thr), ~(rf < thr)
        if 0 < s0.sum() < len(s0) and 0 < sf.sum() < len(sf) and (s0 != sf).sum() > best[1]:
            best = (thr, int((s0 != sf).sum()))
    return best


def flank_case(oracle, tables, name, k, f, mode, truncated=False):
    """The model's side of a flank case under these tables (name: their key in the cache), computed once: the input,
    the threshold at which the flank matters most, the flips there, and the scored sites at flank 0 and f at it."""
    key = (name, k, f, mode, truncated)
    if key not in _flank_cases:
        records, primers, M, E = flank_input(k, f if truncated else 0)
        args = oracle.ntthal_args()
        blunt = bfm.scored_sites(tables, records, primers, M, E, mode, 30.0, args, 0)
        flanked = bfm.scored_sites(tables, records, primers, M, E, mode, 30.0, args, f)
        for fld in ("primer", "pos", "strand"):
            assert (blunt[2][fld] == flanked[2][fld]).all()               # the sites do not depend on the flank
        thr, flips = flank_threshold(oracle, blunt[2]["t"], flanked[2]["t"])
        assert thr is not None
        n = len(primers)
        _flank_cases[key] = (records, primers, M, E, thr, flips, restable(blunt, n, thr), restable(flanked, n, thr))
        print(f"{name} k {k} flank {f} {mode}: threshold {thr}, the stable flag of {flips} of {len(blunt[2])} sites "
              f"differs between flank 0 and flank {f}")
    return _flank_cases[key]


def check_flanked_reach(eng, chem, case, k, f, mode, Ds):
    """stream_reach at flank f against the model on the flanked sites, its counts against background_thal at flank f,
    and the flank must show: the model's records differ from those of flank 0 at some reach."""
    records, primers, M, E, thr, flips, blunt, flanked = case
    assert flips >= 5
    assert 0 < flanked[1].sum() < flanked[0].sum() and 0 < blunt[1].sum() < blunt[0].sum()
    thal = eng.background_thal(records, primers, M, E, chem, thr, mode, flank=f)
    differs = 0
    for D in Ds:
        want = srm.reach_of_scored(k, flanked[2], records, D)
        check(eng, records, primers, M, E, chem, mode, thr, D, flanked[0], flanked[1], want, thal, flank=f)
        differs += int(want.tobytes() != srm.reach_of_scored(k, blunt[2], records, D).tobytes())
    assert differs > 0


@pytest.mark.parametrize("mode", ["any", "end1"])
@pytest.mark.parametrize("k,f", FLANK_GRID)
def test_planted_scored_with_a_flank(m, eng, oracle, oracle_tables, k, f, mode):
    case = flank_case(oracle, oracle_tables, "stock", k, f, mode)
    check_flanked_reach(eng, m.Chem.ntthal(), case, k, f, mode, reaches(k))


def test_packed_with_a_flank(m, eng, oracle, oracle_tables):
    k, f, mode = 13, 2, "any"
    records, primers, M, E, thr, _flips, _blunt, flanked = flank_case(oracle, oracle_tables, "stock", k, f, mode)
    d, total_len, d_starts = eng.put_stream_packed(records)
    try:
        for D in (k, 500):
            c, s, recs = eng.stream_reach_packed(d, total_len, primers, M, E, m.Chem.ntthal(), thr, mode, D,
                                                 record_start=d_starts, flank=f)
            np.testing.assert_array_equal(c, flanked[0])
            np.testing.assert_array_equal(s, flanked[1])
            assert_records_equal(recs, srm.reach_of_scored(k, flanked[2], records, D), f"packed flank {f} D {D}")
    finally:
        eng.device_free(d)


def template_lengths(case, k, f):
    records, primers = case[0], case[1]
    return k + bfm.site_classes(records, primers, case[7][2], f).sum(1)


def test_flanked_reach_on_both_sides_of_wave_max_k(m, oracle, tmp_path):
    """Tables whose one-wave-per-pair kernel ends at 28 bases (tests/param_variants.py stack_x3), k = 24 and flank 4:
    templates of 24 .. 32 bases, so one reach call scores its classes on different routes."""
    import param_variants as pv
    k, f, mode = 24, 4, "any"
    path = pv.write_bundle(pv.variant_sections("stack_x3"), tmp_path / "stack_x3.bundle")
    wave_max_k = m.capi.host_table_routes(path)["wave_max_k"]
    case = flank_case(oracle, oracle.Tables(path), "stack_x3", k, f, mode, truncated=True)
    lengths = template_lengths(case, k, f)
    assert k < wave_max_k < k + 2 * f and (lengths <= wave_max_k).any() and (lengths > wave_max_k).any()
    e = m.Engine(0, params_path=str(path))
    try:
        check_flanked_reach(e, m.Chem.ntthal(), case, k, f, mode, (k, 500))
    finally:
        e.close()


# ---- every site stable: no oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.0, -5.0])
def test_threshold_zero_reaches_from_the_site_list(m, eng, thr):
    rng = np.random.default_rng(7)
    pal = "ACGTACAGTACGT"      # its reverse complement differs in the middle base only: a site on both strands
    primers = [random_seq(rng, 13) for _ in range(16)] + [pal, pal]
    records = plant(rng, [random_seq(rng, 60000), random_seq(rng, 5000)], primers, 10, 3, 1)
    records[1] = pal + records[1] + pal
    chem = m.Chem.ntthal()
    counts, sites = bm.sites(records, primers, 3, 1)
    thal = eng.background_thal(records, primers, 3, 1, chem, thr, "any")
    for D in reaches(13):
        want = srm.reach_of_sites(13, sites, records, D)
        check(eng, records, primers, 3, 1, chem, "any", thr, D, counts, counts, want, thal)
    # the same from the device's own site list
    _c, _s, dev_sites = eng.background_sites(records, primers, 3, 1, capacity=int(counts.sum()) + 16)
    recs = check(eng, records, primers, 3, 1, chem, "any", thr, 500, counts, counts,
                 srm.reach_of_sites(13, dev_sites, records, 500))
    assert recs["sites_plus"].sum() < counts[:, 0].sum()         # the duplicate primer's sites count once
    assert recs["reached_both"].sum() > 0


# ---- geometry -------------------------------------------------------------------------------------------------------
def geometry_records(rng, k, f, v):
    """Records around every path of the reach pass; f and v: two primers, their exact copies are the only sites."""
    rf, rv = bm.revcomp(f), bm.revcomp(v)
    body = lambda n: random_seq(rng, n)
    recs = []

    def start():                      # the stream position the next record starts at
        return sum(len(r) for r in recs) + len(recs)

    def fill_to(target, with_sites=True):
        """One record that ends so that the NEXT record starts at `target`; sites at its first and last positions."""
        n = target - 1 - start()
        assert n >= 0
        r = body(n)
        if with_sites and n >= 2 * k:
            r = (f if len(recs) % 2 else rv) + r[k:n - k] + (rv if len(recs) % 3 else f)
        recs.append(r)

    # record lengths 0, 1, k - 1, k, 63, 64, 65: with a site wherever one fits
    for n in (0, 1, k - 1, k, 63, 64, 65):
        recs.append(f if n == k else (body(n) if n < k else f + body(n - 2 * k) + rv))
    # several records inside one word, consecutive empty records
    recs += ["", "", "", "A", "", f, "", "", rv, "C", "", ""]
    # a record boundary at multiples of 64 and of the tile, each - 1, + 0 and + 1
    for target in (640 - 1, 1280, 1920 + 1, TILE - 1, TILE - 1 + 2 * 64, 2 * TILE, 3 * TILE + 1):
        fill_to(target)
    assert start() == 3 * TILE + 1
    # a record that spans three tiles and more with its only sites in the first and the last tile it touches
    long = body(3 * TILE + 500)
    long = long[:40] + f + long[40 + k:100] + rv + long[100 + k:]
    long = long[:-300] + f + long[-300 + k:-200] + rv + long[-200 + k:]
    recs.append(long)
    # records without a site over two tiles, between records with sites: no carry may cross the boundaries
    recs += [rv + body(30) + f, body(2 * TILE + 77), "", f + body(30) + rv]
    # runs of N inside a record; sites at a record's first and last possible positions
    recs.append(f + "N" * 100 + body(200) + "NRN" + rv + "N" * 70 + rf + body(10) + v)
    recs += [f + body(150) + f, rv + body(150) + rv, f + rv, rv + f]
    fill_to(start() + 2 * TILE + 64 + 1, with_sites=False)
    recs += [f, "", rv, ""]
    return recs


@pytest.fixture(scope="module")
def geometry(m):
    rng = np.random.default_rng(11)
    k = 13
    f, v = "GATTACAGATTCC", "CCATGGTTACGAT"
    records = geometry_records(rng, k, f, v)
    counts, sites = bm.sites(records, [f, v], 0, 0)
    return k, [f, v], records, counts, sites


@pytest.mark.parametrize("D", reaches(13))
def test_geometry(m, eng, geometry, D):
    k, primers, records, counts, sites = geometry
    starts, total = bm.record_starts(records)
    assert total <= 300000 and {0, 1, k - 1, k, 63, 64, 65} <= {len(r) for r in records}
    s = set(starts.tolist())
    assert {640 - 1, 1280, 1920 + 1, TILE - 1, 2 * TILE, 3 * TILE + 1} <= s
    want = srm.reach_of_sites(k, sites, records, D)
    recs = check(eng, records, primers, 0, 0, m.Chem.ntthal(), "any", 0.0, D, counts, counts, want)
    long = int(np.argmax([len(r) for r in records]))
    if D == 500:
        assert recs[long]["gap_either_len"] > 2 * TILE                   # the run crosses whole tiles
    if D == 1 << 20:
        assert recs[long]["reached_both"] > 3 * TILE                     # ... and so does the carried reach
        empty = [i for i, r in enumerate(records) if not r]
        assert (recs["reached_either"][empty] == 0).all() and (recs["gap_either_pos"][empty] == starts[empty]).all()


def test_stream_without_a_site(m, eng):
    rng = np.random.default_rng(13)
    primers = ["GATCGATCGATCG", "TTGCATGCATGCA"]                         # G and T on either strand: none in an A/C stream
    records = [random_seq(rng, n, "AC") for n in (5000, 0, 64, 4096, 1, 9000)]
    counts, sites = bm.sites(records, primers, 2, 0)
    assert counts.sum() == 0
    want = srm.reach_of_sites(13, sites, records, 500)
    recs = check(eng, records, primers, 2, 0, m.Chem.ntthal(), "any", 0.0, 500, counts, counts, want)
    starts = bm.record_starts(records)[0]
    for name in ("plus", "minus", "either"):
        np.testing.assert_array_equal(recs[f"gap_{name}_len"], [len(r) for r in records])
        np.testing.assert_array_equal(recs[f"gap_{name}_pos"], starts)


def test_more_tiles_than_one_scan_step(m, eng):
    """The tile scan takes 1024 tiles per step, and 1024 tiles are 2^22 columns: the one size in this file above 3 x 10^5
    columns, because the step from one chunk of tiles to the next exists only there.  A record whose only sites lie 635
    tiles apart, and a record of 200 tiles that holds the 1024th tile with its only sites at its two ends."""
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
    starts, total = bm.record_starts(records)
    assert total > 1100 * TILE and starts[2] + 50 * TILE < 1024 * TILE < starts[3] - 50 * TILE
    counts, sites = bm.sites(records, [f, v], 0, 0)
    for D in (500, 1 << 20):
        want = srm.reach_of_sites(k, sites, records, D)
        recs = check(eng, records, [f, v], 0, 0, m.Chem.ntthal(), "any", 0.0, D, counts, counts, want)
        if D == 500:
            assert recs["gap_either_len"][2] > 199 * TILE            # the run crosses the 1024th tile
    assert recs["gap_either_len"][0] > 100 * TILE and recs["reached_both"][0] > 0
    assert recs["gap_either_len"][2] == 0 and recs["reached_both"][2] > 0 and recs["reached_both"][3] > 0


# ---- independence from the plumbing ---------------------------------------------------------------------------------
def test_plumbing_options_change_nothing(m, eng, geometry, oracle, oracle_tables):
    rng = np.random.default_rng(17)
    primers = [random_seq(rng, 13) for _ in range(24)]
    records = plant(rng, [random_seq(rng, 90000) for _ in range(3)], primers, 6, 3, 2)
    chem, args = chems(m, oracle)["ntthal"]
    M, E = 4, 0
    counts, sites = bm.sites(records, primers, M, E)
    assert counts.sum() > 3 * 4096
    want = srm.reach_of_sites(13, sites, records, 500)
    # a scored case for force_generic: the threshold decides, so the scoring route could show
    small = plant(rng, [random_seq(rng, 6000), random_seq(rng, 3000)], primers, 4, 2, 2)
    scored = btm.scored_sites(oracle_tables, small, primers, 2, 2, "any", 25.0, args)
    assert 0 < scored[1].sum() < scored[0].sum()
    want_small = srm.reach_of_scored(13, scored[2], small, 300)
    gk, gprimers, grecords, gcounts, gsites = geometry
    gwant = srm.reach_of_sites(gk, gsites, grecords, 65)
    for options in ({}, {"site_list_cap_log2": 12}, {"force_generic": 1}):
        e = m.Engine(0)
        try:
            for key, value in options.items():
                e.set_option(key, value)
            assert e.info("reach_plane_bytes") == 0
            check(e, records, primers, M, E, chem, "any", 0.0, 500, counts, counts, want)
            assert e.info("reach_grows") == 1
            bytes_large = e.info("reach_plane_bytes")
            assert bytes_large == 3 * 8 * ((bm.record_starts(records)[1] + 63) // 64)
            if "site_list_cap_log2" in options:
                assert e.info("background_thal_slabs") > 3 and e.info("background_thal_redone") >= 1
            # smaller calls on the same context: the planes are kept, and cleared
            check(e, small, primers, 2, 2, chem, "any", 25.0, 300, scored[0], scored[1], want_small)
            assert e.info("reach_grows") == 0 and e.info("reach_plane_bytes") == bytes_large
            check(e, grecords, gprimers, 0, 0, chem, "any", 0.0, 65, gcounts, gcounts, gwant)
            assert e.info("reach_grows") == 0
            check(e, records, primers, M, E, chem, "any", 0.0, 500, counts, counts, want)
        finally:
            e.close()


def test_null_record_start_is_one_record(m, eng, geometry):
    k, primers, records, counts, sites = geometry
    chem = m.Chem.ntthal()
    starts = bm.record_starts(records)[0]
    one = ["-".join(records)]
    d, total_len, d_starts = eng.put_stream_packed(records)
    try:
        np.testing.assert_array_equal(d_starts, starts)
        for D in (13, 500):
            c, s, recs = eng.stream_reach_packed(d, total_len, primers, 0, 0, chem, 0.0, "any", D, record_start=d_starts)
            np.testing.assert_array_equal(c, counts)
            assert_records_equal(recs, srm.reach_of_sites(k, sites, records, D), f"packed D {D}")
            c1, s1, recs1 = eng.stream_reach_packed(d, total_len, primers, 0, 0, chem, 0.0, "any", D)
            np.testing.assert_array_equal(c1, counts)
            assert len(recs1) == 1
            assert_records_equal(recs1, srm.reach_of_sites(k, sites, one, D), f"one record D {D}")
            assert recs1["reached_either"][0] >= recs["reached_either"].sum()
    finally:
        eng.device_free(d)


# ---- argument errors ------------------------------------------------------------------------------------------------
def test_argument_errors(m, eng):
    import ctypes as C
    from msspe_amd.capi import REACH_RECORD_DTYPE, MismatchOpt, ReachOpt
    records, chem, primers = ["ACGTACGTACGTACGTACGTACGT"], m.Chem.ntthal(), ["ACGTACGTACGTA"]
    for D in (12, 0, 1 << 31, (1 << 32) - 1):                                   # reach outside [k, 2^31)
        with pytest.raises(m.MsspeError) as e:
            eng.stream_reach(records, primers, 1, 1, chem, 30.0, "any", D)
        assert e.value.code == 1
    eng.stream_reach(records, primers, 1, 1, chem, 30.0, "any", (1 << 31) - 1)
    # the scored call's errors
    for bad_m, bad_e in ((14, 0), (0, 14)):
        with pytest.raises(m.MsspeError) as e:
            eng.stream_reach(records, primers, bad_m, bad_e, chem, 30.0, "any", 100)
        assert e.value.code == 1
    for k in (1, 32):
        with pytest.raises(m.MsspeError) as e:
            eng.stream_reach(records, np.zeros(1, dtype=np.uint64), 0, 0, chem, 30.0, "any", 100, k=k)
        assert e.value.code == 2
    with pytest.raises(m.MsspeError) as e:
        eng.stream_reach(records, primers, 1, 1, chem, 30.0, 3, 100)               # mode
    assert e.value.code == 1
    with pytest.raises(m.MsspeError) as e:
        eng.stream_reach(records, primers, 1, 1, chem, 30.0, "any", 100, flank=5)
    assert e.value.code == 1
    mm, opt = MismatchOpt(1, 1), ReachOpt(100)
    out, words = (C.c_uint64 * 2)(), (C.c_uint64 * 1)(0)
    recs = np.zeros(1, dtype=REACH_RECORD_DTYPE)
    L = eng.L
    assert L.msspe_stream_reach(eng.ptr, None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1, 30.0, 0, None,
                                out, out, recs.ctypes.data, None) == 1                        # reach_opt
    assert L.msspe_stream_reach(eng.ptr, None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1, 30.0, 0,
                                C.byref(opt), out, out, None, None) == 1                      # records_out
    d, total_len, _starts = eng.put_stream_packed(["ACGTACGTACGTACGTACGT", "ACGTACGTACGTACGT"])
    try:
        assert L.msspe_stream_reach_packed_dev(eng.ptr, C.c_void_p(d), total_len, 13, C.byref(mm), words, 1,
                                               C.byref(chem), 1, 30.0, 0, None, None, 0, out, out,
                                               recs.ctypes.data) == 1
        assert L.msspe_stream_reach_packed_dev(eng.ptr, C.c_void_p(d), total_len, 13, C.byref(mm), words, 1,
                                               C.byref(chem), 1, 30.0, 0, C.byref(opt), None, 0, out, out, None) == 1
        for bad in ([0, 21, 21], [5, 3], [1, 21], [0, total_len + 1]):    # not ascending / not from 0 / beyond the stream
            with pytest.raises(m.MsspeError) as e:
                eng.stream_reach_packed(d, total_len, primers, 1, 1, chem, 30.0, "any", 100,
                                        record_start=np.array(bad, dtype=np.uint64))
            assert e.value.code == 1
        for D in (12, 1 << 31):
            with pytest.raises(m.MsspeError) as e:
                eng.stream_reach_packed(d, total_len, primers, 1, 1, chem, 30.0, "any", D)
            assert e.value.code == 1
        _c, _s, recs2 = eng.stream_reach_packed(d, total_len, primers, 1, 1, chem, 0.0, "any", 100,
                                                record_start=np.array([0, total_len], dtype=np.uint64))
        assert len(recs2) == 2 and recs2["reached_plus"][1] == 0 and recs2["gap_plus_pos"][1] == total_len
    finally:
        eng.device_free(d)


def test_no_primers_and_a_stream_shorter_than_k(m, eng):
    chem = m.Chem.ntthal()
    records = ["ACGTACGTACGTACGTACGTACGT", "", "ACGTA"]
    counts, stable, recs, starts = eng.stream_reach(records, [], 1, 1, chem, 30.0, "any", 100, k=13)
    assert counts.shape == stable.shape == (0, 2)
    want = srm.reach_of_sites(13, np.zeros(0, dtype=bm.SITE_DTYPE), records, 100)
    assert_records_equal(recs, want, "n == 0")
    np.testing.assert_array_equal(recs["gap_either_len"], [24, 0, 5])
    np.testing.assert_array_equal(recs["gap_either_pos"], starts)
    short = ["ACGT", "", "ACGTAC"]                                       # 12 columns in all
    counts, stable, recs, starts = eng.stream_reach(short, ["ACGTACGTACGTA"], 1, 1, chem, 30.0, "any", 100)
    assert counts.sum() == stable.sum() == 0
    assert_records_equal(recs, srm.reach_of_sites(13, np.zeros(0, dtype=bm.SITE_DTYPE), short, 100), "total_len < k")
    np.testing.assert_array_equal(recs["gap_plus_len"], [4, 0, 6])


# ---- the CLI --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_inputs(m, tmp_path_factory):
    g = m.synth.aligned_genomes(24, 7000, seed=700)
    assert (g == ord("-")).any() and (g == ord("N")).any()
    d = tmp_path_factory.mktemp("reach_cli")
    fa = d / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    names = [f"g{i}" for i in range(len(g))]
    genomes = [bytes(r).decode().replace("-", "") for r in g]
    return fa, names, genomes


def run_cli(fa, csv, *extra):
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout, Path(csv).read_bytes()


def csv_words(csv):
    return [l.split(",")[2] for l in csv.decode().splitlines()[1:] if l]


def test_cli_block(cli_inputs, tmp_path, oracle, oracle_tables):
    fa, names, genomes = cli_inputs
    base_out, base_csv = run_cli(fa, tmp_path / "a.csv")
    words = csv_words(base_csv)
    assert words and all(len(w) == 13 for w in words)
    # the string rule with the defaults, M = 2 and E = 3
    out, csv = run_cli(fa, tmp_path / "b.csv", "--reach", "500", "--reach-out", str(tmp_path / "r.csv"))
    assert csv == base_csv and out.startswith(base_out)        # report only: the rest of the run is byte for byte
    _c, _s, recs = srm.reach(None, genomes, words, 2, 3, "any", 0.0, 500)
    assert out[len(base_out):] == srm.render(names, genomes, recs, 500, 2, 3)
    assert (tmp_path / "r.csv").read_text() == srm.render_csv(names, genomes, recs)
    print(out[len(base_out):])
    assert recs["reached_either"].sum() > 0 and (recs["gap_either_len"] > 0).any()
    # scored, END1 at 30 C under the screen's chemistry, another rule and reach
    args = oracle.ntthal_args(mv=50.0, dv=3.0, dntp=0.0, dna_conc=250.0, temp_c=25.0)
    out, csv = run_cli(fa, tmp_path / "c.csv", "--reach", "64", "--reach-tm", "30", "--reach-thal", "end1",
                       "--reach-mismatches", "1", "--reach-3p-exact", "2", "--reach-out", str(tmp_path / "s.csv"))
    assert csv == base_csv and out.startswith(base_out)
    _c, stable, recs = srm.reach(oracle_tables, genomes, words, 1, 2, "end1", 30.0, 64, args)
    assert out[len(base_out):] == srm.render(names, genomes, recs, 64, 1, 2, "end1", 30.0)
    assert (tmp_path / "s.csv").read_text() == srm.render_csv(names, genomes, recs)
    assert stable.sum() > 0


def test_cli_usage_errors(cli_inputs, tmp_path):
    fa, _names, _genomes = cli_inputs
    for flags, why in ((("--reach", "12"), "'--reach 12' is smaller than '--kmer-size 13'"),
                       (("--reach-mismatches", "1"), "'--reach-mismatches' needs '--reach <D>'"),
                       (("--reach-3p-exact", "1"), "'--reach-3p-exact' needs '--reach <D>'"),
                       (("--reach-tm", "30"), "'--reach-tm' needs '--reach <D>'"),
                       (("--reach-thal", "end1"), "'--reach-thal' needs '--reach <D>'"),
                       (("--reach-out", "r.csv"), "'--reach-out' needs '--reach <D>'"),
                       (("--reach", "500", "--reach-thal", "end1"), "'--reach-thal' needs '--reach-tm <C>'"),
                       (("--reach", "500", "--kmer-size", "1"), "'--reach' needs '--kmer-size' of at least 2")):
        r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(tmp_path / "x.csv"), "--do-align", "false", *flags],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and why in r.stderr, (flags, r.stderr)
    # a k the engine refuses
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(tmp_path / "x.csv"), "--do-align", "false", "--kmer-size",
                        "32", "--reach", "500"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
