"""Every thermodynamic entry point on tables other than the shipped ones (tests/param_variants.py), against the oracle
on the same file, doubles compared bit for bit.  Which kernel answers a pair is decided from the tables at run time
(fast_ok, int_ok, row_ok, split_max_k, wave_max_k: include/msspe_hip.h at msspe_create); the variants unset them one
at a time, and the oligo lengths sit on both sides of every bound:

    wc_missing          a Watson-Crick stack is missing: every flag 0, the dense kernel alone restates maxTM() for it
    dangle_holes        end terms with only the 3' or only the 5' dangle
    loops_and_bonuses   other loop rows; tri- and tetraloop keys dropped, shifted, added (loops_only: the control)
    stack_x1.5          fast_ok 0, split_max_k 21: split kernel to 21 bases, one wave per pair above; <= 16 dense
    stack_x3            split_max_k 10, wave_max_k 28: dense kernel from 29 bases
    h_mod10             every flag 0: dense kernel alone
    h_frac              refused: every dimer call is MSSPE_ERR_TABLES

Rectangles -- a row oligo against a column oligo or template of another length -- go by the longer of the two:

    g   cross_dimer_ab on every computed variant, the longer oligo on and one above split_max_k and wave_max_k, the
        long oligo on the rows and on the columns, with the wave kernel off and with the dense kernel alone
    h   cross_dimer_end_ab on the same variants
    i   flanked site scoring (templates of k + fl + fr bases): every (fl, fr) class, both modes; on stack_x3 at
        k = 24, flank 4 one call whose classes lie on both sides of wave_max_k; dangle_holes removes the very terms a
        flank brings into play
    (j: the flank through the reach entry points, tests/test_gpu_stream_reach.py and test_gpu_panel_thin_reach.py)

tests/test_param_variants.py pins the flags, which of these lengths lie on which side of a bound, and checks that each
variant moves the oracle's numbers."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import param_variants as pv
from helpers import stage_b_pool
from test_gpu_thermo_parity import bitmap_to_bool, check_pool

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "open-msspe-design_amd" / "bin"
COMPUTED = [v for v in pv.VARIANTS if v not in ("stock", "loops_only", "bonus_caps", "h_frac")]
assert tuple(COMPUTED) == pv.COMPUTED


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


class Variant:
    def __init__(self, m, oracle, name, path):
        self.name, self.path = name, path
        self.tables = oracle.Tables(path)
        self.eng = m.Engine(0, params_path=str(path))
        self.routes = m.capi.host_table_routes(path)


@pytest.fixture(scope="module")
def variants(m, oracle, tmp_path_factory):
    """One engine and one oracle table set per variant, made on first use from the same bundle file."""
    d = tmp_path_factory.mktemp("tables")
    made = {}

    def get(name):
        if name not in made:
            made[name] = Variant(m, oracle, name, pv.write_bundle(pv.variant_sections(name), d / (name + ".bundle")))
        return made[name]

    yield get
    for v in made.values():
        v.eng.close()


@pytest.fixture(scope="module")
def bonus_dir(tmp_path_factory):
    return pv.write_directory(pv.variant_sections("loops_and_bonuses"), tmp_path_factory.mktemp("p3") / "primer3_config")


def any_pool(m, oracle, k):
    """The pool of test_every_oligo_length: 125 random oligos, homopolymers, dinucleotide repeats, palindromes and
    A/T-only oligos."""
    rng = np.random.default_rng(2000 + k)
    pool = m.synth.pool_strings(m.synth.random_pool(125, k, seed=300 + k))
    pool += [b * k for b in "ACGT"] + [(u * k)[:k] for u in ("AT", "TA", "GC", "CG", "AC", "GT")]
    for _ in range(16):
        half = "".join(rng.choice(list("ACGT"), k // 2))
        pool.append(half + ("G" if k % 2 else "") + oracle.reverse_complement(half))
    pool += ["".join(rng.choice(list("AT"), k)) for _ in range(6)]
    assert len(pool) == 157
    return pool


# ---- a. ANY: planes, decisions and counts ----------------------------------------------------------------------------

ANY_CASES = (
    [("wc_missing", k, {}) for k in (9, 13, 14, 15, 16, 20)]
    + [("wc_missing", 13, {"pair_kernel": "int"})]      # an option cannot force a route that has stood down
    + [(v, k, {}) for v in ("dangle_holes", "loops_and_bonuses") for k in (8, 13, 15, 16, 24, 32)]
    + [("stack_x1.5", k, {}) for k in (13, 16, 17, 21, 22, 32)]
    + [("stack_x3", 8, {}), ("stack_x3", 8, {"split_min_k": 2})] + [("stack_x3", k, {}) for k in (10, 11, 28, 29, 32)]
    + [("h_mod10", k, {}) for k in (8, 13, 20, 32)])
# first stage by variant and length at the default options (split_min_k 16): the bounds split_max_k and wave_max_k have
# a length on either side, fast_ok 0 sends 16 bases and fewer to the dense kernel
EXPECTED_FIRST_STAGE = {
    "wc_missing": {9: "dense", 13: "dense", 14: "dense", 15: "dense", 16: "dense", 20: "dense"},
    "dangle_holes": {8: "int", 13: "int", 15: "int", 16: "split", 24: "split", 32: "split"},
    "loops_and_bonuses": {8: "int", 13: "int", 15: "int", 16: "split", 24: "split", 32: "split"},
    "stack_x1.5": {13: "dense", 16: "split", 17: "split", 21: "split", 22: "wave", 32: "wave"},
    "stack_x3": {8: "dense", 10: "dense", 11: "dense", 28: "wave", 29: "dense", 32: "dense"},
    "h_mod10": {8: "dense", 13: "dense", 20: "dense", 32: "dense"},
}
OPTION_RESET = {"pair_kernel": "auto", "short_chain": 1, "split_min_k": 16}


def first_stage(routes, k, opts):
    """The first stage cross_dimer_impl (csrc/capi.cpp) picks for a square block of k-mers at max_loop 30 under these
    flags: the split-table kernel from split_min_k bases (16) up to split_max_k, else one wave per pair above 16 bases
    up to wave_max_k, else up to 16 bases the integer or the f64 register-table kernel where fast_ok, else dense."""
    f64 = opts.get("pair_kernel") == "f64"
    if k <= routes["split_max_k"] and not f64 and (k >= opts.get("split_min_k", 16) or 30 < 2 * k - 4):
        return "split"
    if 16 < k <= routes["wave_max_k"]:
        return "wave"
    if k <= 16 and routes["fast_ok"]:
        return "int" if routes["int_ok"] and not f64 else "f64"
    return "dense"


@pytest.mark.parametrize("variant,k,opts", ANY_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_any_planes_decisions_and_counts(m, oracle, variants, variant, k, opts):
    v = variants(variant)
    eng = v.eng
    pool = any_pool(m, oracle, k)
    thr = -300.0 * k
    eng.pair_stage_stats()
    eng.hand_over_lists()
    try:
        for key, val in opts.items():
            eng.set_option(key, val)
        out, cnt = check_pool(eng, m, oracle, v.tables, pool, {}, thr)
        stats, lists = eng.pair_stage_stats(), eng.hand_over_lists()
        row_kernel = eng.info("row_kernel")
        # the screen proper: decisions and counts without the planes
        fast = eng.cross_dimer(pool, m.Chem.ntthal(), thr, want_dg=False)
    finally:
        for key in opts:
            eng.set_option(key, OPTION_RESET[key])
    cf = oracle.pool_pairs(v.tables, pool, oracle.ntthal_args(), thr, want_dg=False)[2]
    np.testing.assert_array_equal(bitmap_to_bool(fast["bitmap"], len(pool)), cf.astype(bool))
    np.testing.assert_array_equal(fast["row_conflicts"], cf.sum(1).astype(np.uint32))
    assert 0 < cnt < len(pool) ** 2
    assert np.isinf(out["dg"][125, 125]) and np.isfinite(out["dg"][126, 127])     # poly-A x poly-A, poly-C x poly-G
    print(f"route {variant} k={k} {opts}: first stage {first_stage(v.routes, k, opts)}, row_kernel {row_kernel}, hand-over lists {lists}, "
          f"deferred {stats['deferred']}, list stage deferred {stats['list']['deferred']}")
    assert stats["replay_mismatch"] == 0 and stats["list"]["replay_mismatch"] == 0
    first = first_stage(v.routes, k, opts)
    if variant == "wc_missing":
        assert row_kernel == 0                      # no block of this engine goes to the row kernel
    if first in ("int", "split"):
        assert stats["deferred"] > 0                # the integer recurrence ran and handed pairs on
    if first == "wave":
        # one wave per pair writes no integer statistics and hands the pairs of two self-complementary oligos (the
        # pool's palindromes: k is even in these cases) to the dense kernel through list 0
        assert k % 2 == 0 and lists[0] > 0 and stats["deferred"] == 0
    if first == "dense":
        assert lists[0] == 0 and stats["deferred"] == 0     # no list: the dense kernel takes the block
    assert first == EXPECTED_FIRST_STAGE[variant][k] or opts


def test_any_from_a_directory(m, oracle, tmp_path):
    """The wc_missing tables as Primer3's 16 files, what ntthal reads with -path."""
    d = pv.write_directory(pv.variant_sections("wc_missing"), tmp_path / "primer3_config")
    tables = oracle.Tables(d)
    eng = m.Engine(0, params_path=str(d))
    try:
        for k in (13, 20):
            check_pool(eng, m, oracle, tables, any_pool(m, oracle, k), {}, -300.0 * k)
    finally:
        eng.close()


# ---- b. the END screen --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant,k", [(v, k) for v in COMPUTED for k in (13, 20)] + [("stack_x3", 29)])
def test_end_screen(m, oracle, variants, variant, k):
    import test_gpu_end_dimer as te
    v = variants(variant)
    pool = te.end_pool(k, 157, 3)
    for name, (chem, args) in te.CHEMS.items():
        dg, tt = te.oracle_square(oracle, v.tables, pool, args(oracle))
        tend = te.t_end(tt)
        mid = float(np.float32(oracle.round_fixed_f32(float(np.median(tend[tend > 0])), 2)))
        for thr in (47.0, mid):
            out = v.eng.cross_dimer_end(pool, chem(m), thr, want_dg=True, want_tm=True)
            cf = te.check(oracle, out, dg, tt, thr)
            dec = v.eng.cross_dimer_end(pool, chem(m), thr, want_dg=False, want_tm=False)
            np.testing.assert_array_equal(te.bits(dec["bitmap"], len(pool)), cf)
        assert 0 < cf.sum() < cf.size


# ---- c. stage B ------------------------------------------------------------------------------------------------------------

def stage_b_oligos(variant, k):
    pool = stage_b_pool(k, 1000 + k)
    if variant == "loops_and_bonuses" and k in (13, 14):
        pool = pool + pv.bonus_oligos(k)
    return pool


@pytest.mark.parametrize("max_loop", [30, 7])
@pytest.mark.parametrize("k", [13, 14, 16, 24])
@pytest.mark.parametrize("variant", COMPUTED)
def test_oligo_stats(m, oracle, variants, variant, k, max_loop):
    """Tm, GC %, SELF_ANY_TH, SELF_END_TH and HAIRPIN_TH on the four routes of the stage-B chemistry tests, and each
    statistic asked for alone."""
    import test_gpu_stage_b_chemistry as tb
    v = variants(variant)
    pool = stage_b_oligos(variant, k)
    ref = oracle.check_primers(v.tables, pool, oracle.p3_args(max_loop=max_loop))
    chem = m.Chem.primer3(max_loop=max_loop)
    for route, got in tb.routes(v.eng, pool, chem).items():
        tb.assert_stats(got, ref, f"{variant} k={k} max_loop={max_loop} {route}")
    tb.assert_stats(tb.stats_alone(v.eng, m, pool, chem), ref, f"{variant} k={k} alone")
    assert (ref["hairpin_th"] > 0).sum() >= 10 and (ref["self_any_th"] > 0).sum() >= 10


def test_bonus_keys_decide_hairpins_on_the_device(m, oracle, variants):
    """The designed pool of test_every_bonus_oligo_feels_its_key: the engine under loops_and_bonuses and under its
    control loops_only equals the oracle under each, and the two differ wherever the oracle's do -- a bonus table
    with stock keys or values in it, a capped count or an ignored triloop entropy would show here."""
    a, b = variants("loops_and_bonuses"), variants("loops_only")
    for k in (13, 14):
        pool = pv.bonus_oligos(k)
        want_a = oracle.check_primers(a.tables, pool)["hairpin_th"]
        want_b = oracle.check_primers(b.tables, pool)["hairpin_th"]
        assert (want_a != want_b).sum() >= (18 if k == 13 else 43)
        np.testing.assert_array_equal(a.eng.oligo_stats(pool)["hairpin"], want_a)
        np.testing.assert_array_equal(b.eng.oligo_stats(pool)["hairpin"], want_b)


def test_bonus_tables_at_their_caps_on_the_device(m, oracle, variants):
    """32 triloop and 128 tetraloop keys, the most the device tables hold: the keys bonus_caps adds sort behind the
    shipped ones, into slots 16 .. 31 and 75 .. 127 of the sorted device tables, and each carries an entropy and an
    enthalpy of its own.  A kernel that scans the shipped count of keys, or drops the triloop entropy (zero in the
    shipped file), gives the control's value for them.  Both hairpin kernels: one wave per oligo and one lane per oligo."""
    import test_gpu_stage_b_chemistry as tb
    v, control = variants("bonus_caps"), variants("loops_only")
    for k in (13, 14):
        pool = pv.caps_oligos(k) + pv.bonus_oligos(k)
        ref = oracle.check_primers(v.tables, pool)
        base = oracle.check_primers(control.tables, pool)["hairpin_th"]
        n_new = len(pv.caps_oligos(k))
        assert n_new == (16 if k == 13 else 51) and (ref["hairpin_th"][:n_new] != base[:n_new]).all()
        for route, got in tb.routes(v.eng, pool, m.Chem.primer3()).items():
            tb.assert_stats(got, ref, f"caps k={k} {route}")


def test_oligo_stats_of_a_large_pool_under_other_bonuses(m, oracle, variants):
    """Above 8,192 oligos HAIRPIN_TH runs one lane per oligo."""
    import test_gpu_stage_b_chemistry as tb
    v = variants("loops_and_bonuses")
    pool = stage_b_pool(13, 4242, n_random=6000, n_stem_loops=3000) + pv.bonus_oligos(13)
    assert len(pool) >= 8192
    ref = oracle.check_primers(v.tables, pool)
    for route, got in tb.routes(v.eng, pool, m.Chem.primer3()).items():
        tb.assert_stats(got, ref, route)


# ---- d. the full record ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [13, 20])
@pytest.mark.parametrize("variant", ["wc_missing", "loops_and_bonuses", "stack_x3"])
def test_thal_detail(m, oracle, variants, variant, k):
    import test_gpu_thal_detail as td
    v = variants(variant)
    a, b = td.random_pairs(k, 64, 7300 + k)
    for mode in td.MODES:
        want = td.oracle_records(oracle, v.tables, a, b, mode)
        td.assert_records(v.eng.thal_detail(a, b, None, mode), want, k, (variant, k, mode))
        assert (want["no_structure"] == 0).sum() >= 32


# ---- e. background sites scored with thal -------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [13, 20])
@pytest.mark.parametrize("variant", ["wc_missing", "loops_and_bonuses", "stack_x3"])
def test_background_thal(m, oracle, variants, variant, k):
    import test_gpu_background_thal as tb
    v = variants(variant)
    rng = np.random.default_rng(100 + k)
    M, E = max(1, k // 6), min(3, k // 4)
    primers = [tb.random_seq(rng, k) for _ in range(24)]
    records = tb.plant(rng, [tb.random_seq(rng, 20000)], primers, 16, M, E)
    chem, args = tb.chems(m, oracle)["ntthal"]
    for mode in ("any", "end1"):
        want = tb.check_against_model(v.eng, v.tables, records, primers, M, E, chem, args, mode, 30.0)
        t_site = np.maximum(want[2]["t"], 0.0)
        mid = float(np.float32(oracle.round_fixed_f32(float(np.median(t_site)), 2)))
        _c, _s, recs = tb.check_against_model(v.eng, v.tables, records, primers, M, E, chem, args, mode, mid,
                                              want=tb.restable(want, len(primers), mid))
        assert len(recs) >= 200 and 0 < recs["stable"].sum() < len(recs)


# ---- f. the process boundaries ---------------------------------------------------------------------------------------------------

def test_ntthal_shim_with_a_path(oracle, bonus_dir):
    import test_gpu_shims as ts
    tables = oracle.Tables(bonus_dir)
    argv, okw = ts.NTTHAL_RUNS["reference_argv"]
    # ten pairs: the first nine of a mixed-length draw whose block the loop tables change, and one without structure
    drawn = ts.mixed_length_pairs(8300, n=400)
    both = zip(drawn, ts.expected_ntthal_blocks(oracle, tables, drawn, "ANY", oracle.ntthal_args(**okw)),
               ts.expected_ntthal_blocks(oracle, oracle.Tables(), drawn, "ANY", oracle.ntthal_args(**okw)))
    pairs = [p for p, a, b in both if a != b][:9] + [("A" * 13, "A" * 13)]
    assert len(pairs) == 10 and {len(a) for a, _ in pairs} >= {13, 20}
    blocks = ts.expected_ntthal_blocks(oracle, tables, pairs, "ANY", oracle.ntthal_args(**okw))
    res = subprocess.run([str(BIN / "ntthal-hip"), "-a", "ANY"] + argv + ["-path", str(bonus_dir) + "/", "-i"],
                         input="\n".join(f"{a},{b}" for a, b in pairs), capture_output=True, text=True,
                         timeout=ts.SHIM_TIMEOUT)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    shown = [b for b in blocks if b is not None]
    assert len(shown) == 9 and len(lines) == 5 * len(shown)
    for q, (head, rows, _) in enumerate(shown):
        assert lines[5 * q] == head, q
        assert [r.replace("\t", " ").rstrip() for r in lines[5 * q + 1:5 * q + 5]] == rows, q


def test_primer3_shim_with_a_path(oracle, bonus_dir):
    import os
    import test_gpu_shims as ts
    tables = oracle.Tables(bonus_dir)
    oligos = pv.bonus_oligos(13) + pv.bonus_oligos(14)
    stdin = "".join(f"SEQUENCE_ID={p}\nSEQUENCE_PRIMER={p}\nPRIMER_TASK=check_primers\n=\n" for p in oligos)
    res = subprocess.run([str(BIN / "primer3_core-hip")], input=stdin, capture_output=True, text=True,
                         timeout=ts.SHIM_TIMEOUT, env=dict(os.environ, MSSPE_PARAMS_PATH=str(bonus_dir)))
    assert res.returncode == 0, res.stderr
    records = res.stdout.split("\n=\n")
    assert records[-1] == "" and len(records) == len(oligos) + 1
    differ = 0
    for q, p in enumerate(oligos):
        kv = dict(l.split("=", 1) for l in records[q].splitlines())
        w = oracle.check_primers(tables, [p])[0]
        got = tuple(kv["PRIMER_LEFT_0_" + t] for t in ("TM", "GC_PERCENT", "SELF_ANY_TH", "SELF_END_TH", "HAIRPIN_TH"))
        assert kv["SEQUENCE_ID"] == p and got == ("%.3f" % w["tm"], "%.3f" % w["gc"], "%.2f" % w["self_any_th"],
                                                  "%.2f" % w["self_end_th"], "%.2f" % w["hairpin_th"]), (q, p)
        differ += got[4] != "%.2f" % oracle.check_primers(oracle.Tables(), [p])[0]["hairpin_th"]
    assert differ >= 90


def test_cli_with_a_path(m, oracle, bonus_dir, tmp_path, monkeypatch):
    """od-msspe-hip --params-path on the small alignment of the host-layer tests: another CSV than the shipped
    tables give, the same as with MSSPE_PARAMS_PATH set instead, and the one the restated pipeline gives on those
    tables."""
    import ctypes as C
    import ref_pipeline
    from test_host_layer import LIB, argv, call
    m.load_library()
    host = C.CDLL(str(LIB))
    # a looser hairpin limit and a tighter dG cut at 37 C: the loop tables then decide which primers are kept
    g = m.synth.aligned_genomes(24, 3200)
    fasta = "".join(f">genome{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g))
    fa = tmp_path / "in.fa"
    fa.write_text(fasta)
    extra = ["--max-hairpin-tm", "40", "--delta-g-threshold", "-4000", "--annealing-temp", "37"]
    kw = dict(max_hairpin=40.0, dg=-4000.0, temp=37.0)

    def run(name, *more):
        csv = tmp_path / name
        rc, report = call(host.odm_run_cli, *argv("-i", str(fa), "-o", str(csv), "--do-align", "false", *extra, *more))
        assert rc == 0, report
        return csv.read_text(), report

    stock_csv, _ = run("stock.csv")
    flag_csv, flag_report = run("flag.csv", "--params-path", str(bonus_dir))
    monkeypatch.setenv("MSSPE_PARAMS_PATH", str(bonus_dir))
    env_csv, env_report = run("env.csv")
    monkeypatch.delenv("MSSPE_PARAMS_PATH")
    assert (env_csv, env_report) == (flag_csv, flag_report)
    want_csv, want_report, _ = ref_pipeline.run(fasta, tables=bonus_dir, **kw)
    assert flag_csv == want_csv and flag_report == want_report
    assert ref_pipeline.run(fasta, **kw)[0] == stock_csv
    assert flag_csv != stock_csv and flag_csv.count("\n") > 3


# ---- g. rectangular ANY screens ------------------------------------------------------------------------------------------------

ROUTE_OPTION_RESET = {"wave_kernel": 1, "force_generic": 0}


def route_settings(routes):
    """The default route, and where the tables leave a first stage to switch off: without the wave kernel, and the
    dense kernel alone."""
    return [{}] + ([{"wave_kernel": 0}, {"force_generic": 1}] if routes["wave_max_k"] > 0 else [])


def any_decisions(oracle, dg, thr):
    cf = np.zeros(dg.shape, dtype=np.uint8)
    for i, j in zip(*np.nonzero(np.isfinite(dg))):
        cf[i, j] = oracle.edge_decision(float(dg[i, j]), thr)
    return cf


def rect_any_reference(oracle, tables, k_a, k_b):
    """The 48 x 64 block of test_gpu_mixed_length.pools under these tables, and a threshold from the oracle's own
    values: the float32 of the 5th percentile of the finite dG (at the stock -9000 cal/mol most pairs of
    a block conflict under stack_x3)."""
    import test_gpu_mixed_length as tm
    A, B = tm.pools(k_a, k_b, 48, 64)
    dg, tt, _ = tm.oracle_block(oracle, tables, A, B, oracle.ntthal_args())
    thr = float(np.float32(np.percentile(dg[np.isfinite(dg)], 5)))
    return A, B, dg, tt, thr, any_decisions(oracle, dg, thr)


@pytest.mark.parametrize("variant,k_a,k_b", pv.RECT_ANY_CASES)
def test_rectangular_any_screen(m, oracle, variants, variant, k_a, k_b):
    import test_gpu_mixed_length as tm
    v = variants(variant)
    kmax = max(k_a, k_b)
    first = pv.rect_stage(v.routes, kmax)
    assert first == pv.EXPECTED_RECT_STAGE[variant][0][kmax]
    if (variant, k_a, k_b) in pv.RECT_ANY_ON_BOUND:   # the longer oligo on a bound of these tables, or one base above it
        bound, above = pv.RECT_ANY_ON_BOUND[(variant, k_a, k_b)]
        assert kmax == v.routes[bound] + above
    elif (k_a, k_b) == (8, 32):
        assert v.routes["split_max_k"] == v.routes["wave_max_k"] == 0       # the dense kernel alone
    A, B, dg, tt, thr, cf = rect_any_reference(oracle, v.tables, k_a, k_b)
    finite = int(np.isfinite(dg).sum())
    print(f"{variant} ({k_a}, {k_b}): first stage {first}, threshold {thr}, {int(cf.sum())} conflicts among {finite} finite pairs")
    assert 0 < cf.sum() < finite                    # (a 2-mer's duplexes included: 130 to 150 of some 3,000 lie below)
    chem = m.Chem.ntthal()
    try:
        for opts in route_settings(v.routes):
            for key, val in opts.items():
                v.eng.set_option(key, val)
            out = v.eng.cross_dimer_ab(A, B, chem, thr, want_dg=True, want_tm=True)
            np.testing.assert_array_equal(out["dg"], dg, err_msg=str(opts))
            np.testing.assert_array_equal(out["tm"], tt, err_msg=str(opts))
            np.testing.assert_array_equal(tm.bits(out["bitmap"], len(B)), cf, err_msg=str(opts))
            np.testing.assert_array_equal(out["row_conflicts"], cf.sum(1).astype(np.uint32), err_msg=str(opts))
            fast = v.eng.cross_dimer_ab(A, B, chem, thr, want_dg=False)        # decisions only
            np.testing.assert_array_equal(tm.bits(fast["bitmap"], len(B)), cf, err_msg=str(opts))
            np.testing.assert_array_equal(fast["row_conflicts"], cf.sum(1).astype(np.uint32), err_msg=str(opts))
            for key in opts:
                v.eng.set_option(key, ROUTE_OPTION_RESET[key])
    finally:
        for key, val in ROUTE_OPTION_RESET.items():
            v.eng.set_option(key, val)


# ---- h. rectangular END1 screens -----------------------------------------------------------------------------------------------

def rect_end_reference(oracle, tables, k_a, k_b):
    """The pools of test_gpu_end_dimer.test_ab_shapes_match_the_oracle at 48 x 64, and a Tm threshold from the oracle's
    own values: the "%.2f" float32 of the 90th percentile of max(t, 0)."""
    import test_gpu_end_dimer as te
    A, B = te.end_pool(k_a, 48, 8), te.end_pool(k_b, 64, 9)
    for j in range(12):                       # B oligos pairing with A's 3' ends
        tail = A[j][-min(k_a, k_b):]
        B[j] = (te.rc(tail) + B[j])[:k_b]
    dg, tt = te.oracle_ab(oracle, tables, A, B, oracle.ntthal_args())
    tend = te.t_end(tt)
    thrs = [float(np.float32(oracle.round_fixed_f32(float(np.percentile(tend, 90)), 2)))]
    if thrs[0] <= 0.0:
        # 13-mers at 25 C under tables near the shipped ones: fewer than a tenth of the pairs melt above 0 C, the
        # percentile is 0 and every pair conflicts at it.  That threshold is run all the same; the one that splits the
        # pairs is the same percentile among the pairs with a positive t
        thrs.append(float(np.float32(oracle.round_fixed_f32(float(np.percentile(tend[tend > 0], 90)), 2))))
    return A, B, dg, tt, thrs


@pytest.mark.parametrize("k_a,k_b", pv.RECT_END_SHAPES)
@pytest.mark.parametrize("variant", COMPUTED)
def test_rectangular_end_screen(m, oracle, variants, variant, k_a, k_b):
    import test_gpu_end_dimer as te
    v = variants(variant)
    first = pv.rect_stage(v.routes, max(k_a, k_b), end=True)
    assert first == pv.EXPECTED_RECT_STAGE[variant][1][max(k_a, k_b)]
    A, B, dg, tt, thrs = rect_end_reference(oracle, v.tables, k_a, k_b)
    chem = m.Chem.ntthal()
    try:
        for opts in route_settings(v.routes)[:2]:
            for key, val in opts.items():
                v.eng.set_option(key, val)
            for thr in thrs:
                out = v.eng.cross_dimer_end_ab(A, B, chem, thr, want_dg=True, want_tm=True)
                cf = te.check(oracle, out, dg, tt, thr)
                fast = v.eng.cross_dimer_end_ab(A, B, chem, thr, want_dg=False, want_tm=False)
                np.testing.assert_array_equal(te.bits(fast["bitmap"], len(B)), cf, err_msg=f"{opts} {thr}")
                np.testing.assert_array_equal(fast["row_conflicts"], cf.sum(1).astype(np.uint32), err_msg=f"{opts} {thr}")
                assert cf.all() if thr <= 0.0 else 0 < cf.sum() < cf.size
            for key in opts:
                v.eng.set_option(key, ROUTE_OPTION_RESET[key])
    finally:
        v.eng.set_option("wave_kernel", 1)
    print(f"{variant} ({k_a}, {k_b}) END1: first stage {first}, thresholds {thrs}, {int(cf.sum())} conflicts of {cf.size}")
    assert thrs[-1] > 0.0 and 0 < cf.sum() < cf.size


# ---- i. flanked site scoring -----------------------------------------------------------------------------------------------------

def flank_case(k, f):
    """24 primers, three records of 3,000 bases with 8 planted near-copies of each (test_gpu_background_flank.base_case
    in small), and the truncation block of test_every_truncation_class for this k and f: an N at every distance 0 .. f
    on either side of exact copies of primer 0 on both strands, and a stream that starts and ends flush with a copy --
    every (fl, fr) class occurs, so every template length k .. k + 2 f does."""
    import test_gpu_background_flank as tf
    from background_model import revcomp
    rng = np.random.default_rng(7000 + 10 * k + f)
    M, E = 3, 2
    primers = [tf.random_seq(rng, k) for _ in range(24)]
    records = tf.plant(rng, [tf.random_seq(rng, 3000) for _ in range(3)], primers, 8, M, E)
    copy = [primers[0], revcomp(primers[0])]
    gap = lambda d: d if d < f else f + 3       # base columns between the copy and the N: d, and "f or more"
    body = []
    for dl in range(f + 1):
        for dr in range(f + 1):
            for s in (0, 1):
                body.append("N" + tf.random_seq(rng, gap(dl)) + copy[s] + tf.random_seq(rng, gap(dr)) + "N")
                body.append(tf.random_seq(rng, 40))
    records.insert(0, copy[0] + tf.random_seq(rng, 30) + copy[1])
    records.append("".join(body))
    records.append(copy[1] + tf.random_seq(rng, 30) + copy[0])
    return records, primers, M, E


def flanked_model(oracle, v, k, f, mode):
    """The model's scored sites at 30 C and at the threshold that splits them (the "%.2f" float32 of the median t_site,
    as test_background_thal builds it), once per variant, shape and mode."""
    import background_flank_model as bfm
    import test_gpu_background_thal as tb
    cache = v.__dict__.setdefault("flanked", {})
    if (k, f, mode) not in cache:
        records, primers, M, E = flank_case(k, f)
        want = bfm.scored_sites(v.tables, records, primers, M, E, mode, 30.0, oracle.ntthal_args(), f)
        mid = float(np.float32(oracle.round_fixed_f32(float(np.median(np.maximum(want[2]["t"], 0.0))), 2)))
        cache[(k, f, mode)] = (want, mid, tb.restable(want, len(primers), mid))
    return cache[(k, f, mode)]


@pytest.mark.parametrize("mode", ["any", "end1"])
@pytest.mark.parametrize("k,f", pv.FLANK_GRID)
@pytest.mark.parametrize("variant", pv.FLANK_VARIANTS)
def test_flanked_sites(m, oracle, oracle_tables, variants, variant, k, f, mode):
    import background_flank_model as bfm
    import test_gpu_background_flank as tf
    v = variants(variant)
    records, primers, M, E = flank_case(k, f)
    chem, args = m.Chem.ntthal(), oracle.ntthal_args()
    want, mid, split = flanked_model(oracle, v, k, f, mode)
    recs = want[2]
    tf.check_against_model(v.eng, v.tables, records, primers, M, E, chem, args, mode, 30.0, f, want=want)
    classes, truncated = tf.check_info(v.eng, records, primers, recs, f)
    assert classes == (f + 1) ** 2 and 0 < truncated < len(recs)
    tf.check_against_model(v.eng, v.tables, records, primers, M, E, chem, args, mode, mid, f, want=split)
    assert tf.check_info(v.eng, records, primers, recs, f) == (classes, truncated)
    n_stable = int(split[2]["stable"].sum())
    print(f"{variant} k={k} f={f} {mode}: {len(recs)} sites, {classes} classes, {truncated} truncated, threshold {mid}: "
          f"{n_stable} stable")
    assert len(recs) >= 150 and 0 < n_stable < len(recs)      # 153 to 209 sites: planted copies overwrite one another
    lengths = k + bfm.site_classes(records, primers, recs, f).sum(1)
    assert set(lengths.tolist()) == set(range(k, k + 2 * f + 1))
    wave_max_k = v.routes["wave_max_k"]
    if variant == "stack_x3" and (k, f) == (24, 4):
        # one call whose classes take different routes: one wave per pair up to wave_max_k bases, the dense kernel above
        assert k < wave_max_k < k + 2 * f and (lengths <= wave_max_k).any() and (lengths > wave_max_k).any()
        v.eng.set_option("wave_kernel", 0)
        try:
            tf.check_against_model(v.eng, v.tables, records, primers, M, E, chem, args, mode, mid, f, want=split)
        finally:
            v.eng.set_option("wave_kernel", 1)
    if variant == "dangle_holes":
        # a blunt k x k site has no overhang; the flank brings in the dangle terms this variant takes away
        stock = bfm.scored_sites(oracle_tables, records, primers, M, E, mode, 30.0, args, f)[2]
        moved = int((stock["dg"] != recs["dg"]).sum())
        print(f"dangle_holes k={k} f={f} {mode}: dG differs from the stock tables' at {moved} of {len(recs)} sites")
        assert moved >= len(recs) / 10


def test_amplicons_of_flanked_sites_on_both_sides_of_wave_max_k(m, oracle, variants):
    """stack_x3 at k = 24, flank 4: the amplicons of the stable flanked sites, as test_amplicons_of_the_flanked_sites."""
    import background_amplicon_model as bam
    import background_model as bm
    v = variants("stack_x3")
    k, f = 24, 4
    records, primers, M, E = flank_case(k, f)
    _want, mid, scored = flanked_model(oracle, v, k, f, "any")
    w_amp, w_total, w_list = bam.amplicons_of(len(primers), k, scored[2], records, k, 2000)
    counts, stable, amps, total, starts, lst = v.eng.background_amplicons(records, primers, M, E, m.Chem.ntthal(), mid, "any",
                                                                         k, 2000, capacity=w_total + 8, flank=f)
    np.testing.assert_array_equal(counts, scored[0])
    np.testing.assert_array_equal(stable, scored[1])
    np.testing.assert_array_equal(amps, w_amp)
    assert total == w_total > 0
    np.testing.assert_array_equal(lst, w_list)
    np.testing.assert_array_equal(starts, bm.record_starts(records)[0])


# ---- k. tables the engine refuses ----------------------------------------------------------------------------------------------

def test_non_integral_enthalpies_are_refused_by_every_dimer_call(m, oracle, variants):
    """ntthal computes with stack.dh CG/GC = -10600.5; the engine's kernels carry enthalpies as integers and refuse:
    MSSPE_ERR_TABLES with "not integral" from every call that scores a dimer, no number returned, and the context
    goes on serving the calls that need no pair table: Tm, GC % and HAIRPIN_TH alone, stage A, the background scan."""
    import torch
    v = variants("h_frac")
    eng = v.eng
    assert v.routes["pair_tables"] == 0
    pool = m.synth.pool_strings(m.synth.random_pool(40, 13, seed=1))
    other = m.synth.pool_strings(m.synth.random_pool(12, 20, seed=2))
    chem = m.Chem.ntthal()
    rng = np.random.default_rng(9)
    record = "".join(rng.choice(list("ACGT"), 5000)) + pool[0] + "".join(rng.choice(list("ACGT"), 500))
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    d_out = torch.full((len(pool),), -1.0, dtype=torch.float64, device="cuda")
    calls = {
        "any": lambda: eng.cross_dimer(pool, chem, -9000.0, want_dg=True),
        "any_decisions": lambda: eng.cross_dimer(pool, chem, -9000.0, want_dg=False),
        "edges": lambda: eng.cross_dimer_edges(pool, chem, -9000.0),
        "ab": lambda: eng.cross_dimer_ab(pool, other, chem, -9000.0),
        "ab_edges": lambda: eng.cross_dimer_ab_edges(pool, other, chem, -9000.0),
        "edges_mixed": lambda: eng.cross_dimer_edges_mixed(pool + other, chem, -9000.0),
        "end": lambda: eng.cross_dimer_end(pool, chem, 47.0),
        "end_edges": lambda: eng.cross_dimer_end_edges(pool, chem, 47.0),
        "end_ab": lambda: eng.cross_dimer_end_ab(pool, other, chem, 47.0),
        "cover": lambda: eng.conflict_cover(pool, chem, -9000.0),
        "tubes": lambda: eng.conflict_tubes(pool, chem, -9000.0),
        "detail_any": lambda: eng.thal_detail(pool[:8], pool[8:16], chem, "any"),
        "detail_end1": lambda: eng.thal_detail(pool[:8], pool[8:16], chem, "end1"),
        "background_thal": lambda: eng.background_thal([record], pool[:8], 2, 2, chem, 30.0, "any", capacity=4096),
        "background_thal_end1": lambda: eng.background_thal([record], pool[:8], 2, 2, chem, 30.0, "end1", capacity=4096),
        "background_amplicons": lambda: eng.background_amplicons([record], pool[:8], 2, 2, chem, 30.0, "any", 50, 2000,
                                                                 capacity=4096),
        "oligo_stats": lambda: eng.oligo_stats(pool),
        "self_any_alone": lambda: eng.oligo_stats_dev(d_pool.data_ptr(), len(pool), 13, m.Chem.primer3(),
                                                      d_self_any=d_out.data_ptr()),
        "self_end_alone": lambda: eng.oligo_stats_dev(d_pool.data_ptr(), len(pool), 13, m.Chem.primer3(),
                                                      d_self_end=d_out.data_ptr()),
    }
    for name, fn in calls.items():
        with pytest.raises(m.MsspeError) as e:
            fn()
        assert e.value.code == 3 and "not integral" in str(e.value), name
    # Tm, GC % and HAIRPIN_TH need no pair tables: asked for without the self-dimers they are served, and are the oracle's
    ref = oracle.check_primers(v.tables, pool)
    for key, field in (("d_tm", "tm"), ("d_gc", "gc"), ("d_hairpin", "hairpin_th")):
        d_out.fill_(-1.0)
        eng.oligo_stats_dev(d_pool.data_ptr(), len(pool), 13, m.Chem.primer3(), **{key: d_out.data_ptr()})
        eng.synchronize()
        np.testing.assert_array_equal(d_out.cpu().numpy(), ref[field], err_msg=field)
    # a refused call leaves no number behind
    d_out.fill_(-1.0)
    with pytest.raises(m.MsspeError):
        eng.oligo_stats_dev(d_pool.data_ptr(), len(pool), 13, m.Chem.primer3(), d_tm=d_out.data_ptr(),
                            d_self_any=d_out.data_ptr())
    eng.synchronize()
    assert (d_out.cpu().numpy() == -1.0).all()
    # the context is still good: stage A and the table-free background scan answer as ever
    genomes = m.synth.aligned_genomes(12, 3000)
    words, freqs = eng.kmer_candidates(genomes, m.KmerOpt(500, 250, 50, 13, 40, 1), 0)
    want = oracle.Segments([bytes(r).decode() for r in genomes], 500, 250, 50, 13).candidates(0, 40, 1)
    assert list(zip(words, freqs.tolist())) == want
    assert int(np.asarray(eng.background_sites([record], pool[:8], 2, 2)[0]).sum()) >= 1
    with pytest.raises(m.MsspeError) as e:
        eng.cross_dimer(pool, chem, -9000.0)
    assert e.value.code == 3
