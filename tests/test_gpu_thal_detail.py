"""The full thal record (msspe_thal_detail_pairs: dS, dH, dG, t, no_structure, n_pairs and the traced base pairs) against
the CPU oracle, field by field.

The screens read only dG and t of a pair; `bin/ntthal-hip` prints this record, and an unmodified od-msspe reads the
header line and the drawing built from ps1 / ps2 (od-msspe/src/delta_g.rs:206-230).  Bar: dS, dH, dG and t equal as
doubles (both sides evaluate the same IEEE-754 operations in the same order), the traced pairs identical, everything
behind the oligo's length zero, and a record without a structure all zero.
"""
import ctypes as C
import json
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LANES = 65536                     # workspace lanes of the dense kernel: problem w runs on lane w % LANES
N_RANDOM = 300
KS = (2, 3, 5, 9, 13, 16, 17, 24, 32)
MODES = ("any", "end1")
DOUBLES = ("dS", "dH", "dG", "t")

# (msspe_chem keywords == pyoracle argument keywords, base chemistry)
CHEMS = {
    "primer3": ("primer3", {}),
    "mv100_dv0_dna50": ("ntthal", dict(mv=100.0, dv=0.0, dntp=0.0, dna_conc=50.0)),   # test_chemistry_and_threshold_variants
    "loop0": ("ntthal", dict(max_loop=0)),                                             # test_loop_size_limit_on_short_oligos
    "loop3": ("ntthal", dict(max_loop=3)),
    "loop8": ("ntthal", dict(max_loop=8)),
}


@pytest.fixture(scope="module")
def eng():
    import msspe_amd
    e = msspe_amd.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


def random_oligos(rng, k, n):
    return ["".join(rng.choice("ACGT") for _ in range(k)) for _ in range(n)]


def random_pairs(k, n, seed):
    rng = random.Random(seed)
    return random_oligos(rng, k, n), random_oligos(rng, k, n)


def oracle_mode(oracle, mode):
    return {"any": oracle.ANY, "end1": oracle.END1}[mode]


def oracle_records(oracle, tables, a, b, mode, args=None, full=True):
    """oracle.thal of every pair as a record array of the binding's dtype (full=False: without ps1 / ps2)."""
    from msspe_amd.capi import THAL_DETAIL_DTYPE
    want = np.zeros(len(a), dtype=THAL_DETAIL_DTYPE)
    omode = oracle_mode(oracle, mode)
    for q, (x, y) in enumerate(zip(a, b)):
        r = oracle.thal(tables, x, y, omode, args)
        want[q] = (r.dS, r.dH, r.dG, r.t, r.no_structure, r.n_pairs, 0, 0)
        if full and not r.no_structure:
            assert len(x) <= 32 and not any(r.ps1[len(x):len(x) + 8]) and not any(r.ps2[len(y):len(y) + 8])
            want["ps1"][q, :len(x)] = r.ps1[:len(x)]
            want["ps2"][q, :len(y)] = r.ps2[:len(y)]
    return want


def assert_records(got, want, k, what=""):
    """Every field of every record; the first differing record is named."""
    assert got.shape == want.shape
    for f in DOUBLES + ("no_structure", "n_pairs"):
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (what, f, int(bad[0]), got[f][bad[0]], want[f][bad[0]], int(bad.size))
    for f in ("ps1", "ps2"):
        bad = np.flatnonzero((got[f][:, :k] != want[f][:, :k]).any(axis=1))
        assert bad.size == 0, (what, f, int(bad[0]), got[f][bad[0]].tolist(), want[f][bad[0]].tolist(), int(bad.size))
        assert not got[f][:, k:].any(), (what, f, "bytes behind the oligo")
    none = got["no_structure"] != 0
    for f in DOUBLES:
        assert (got[f][none] == 0.0).all(), (what, f, "no structure")
    assert not got["ps1"][none].any() and not got["ps2"][none].any(), (what, "no structure: ps bytes")
    assert (got["n_pairs"][none] == 0).all(), (what, "no structure: n_pairs")


def not_contiguous(rec, k):
    """The traced structure is not one run of stacked pairs: two consecutive pairs differ by more than (1, 1)."""
    i = np.flatnonzero(rec["ps1"][:k])
    j = rec["ps1"][:k][i].astype(int)
    return bool(((np.diff(i) != 1) | (np.diff(j) != 1)).any())


def chem_pair(m, oracle, name):
    base, kw = CHEMS[name]
    if base == "primer3":
        return m.Chem.primer3(**kw), oracle.p3_args(**kw)
    return m.Chem.ntthal(**kw), oracle.ntthal_args(**kw)


# ---- a. random pairs at every kind of length, both modes ---------------------------------------------------------------

def random_case(oracle, tables, k, mode):
    a, b = random_pairs(k, N_RANDOM, 7100 + k)
    want = oracle_records(oracle, tables, a, b, mode)
    return a, b, want


def check_random_case_inputs(want, k, mode):
    """Floors on the oracle's results alone: the pairs exercise the no-structure exit and loops in the traceback."""
    n = len(want)
    if k <= 3:
        assert (want["no_structure"] != 0).sum() >= 0.10 * n, (k, mode)
    if k >= 9:
        structured = [r for r in want if not r["no_structure"]]
        assert sum(not_contiguous(r, k) for r in structured) >= 0.05 * len(structured), (k, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", KS)
def test_random_pairs_full_record(eng, oracle, oracle_tables, k, mode):
    """k 2..32: below / at / above the lengths where the screens change kernels, the shortest and the longest oligo."""
    a, b, want = random_case(oracle, oracle_tables, k, mode)
    check_random_case_inputs(want, k, mode)
    assert_records(eng.thal_detail(a, b, None, mode), want, k, (k, mode))


# ---- b. chemistries ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", (13, 24))
@pytest.mark.parametrize("name", list(CHEMS))
def test_chemistries_full_record(eng, m, oracle, oracle_tables, name, k, mode):
    """Primer3's chemistry, an off-default salt / DNA one, and loop limits that cut the predecessor scan: the record's
    traceback walks the same d <= max_loop + 2 band as the fill."""
    a, b = random_pairs(k, N_RANDOM, 7300 + k)
    chem, oargs = chem_pair(m, oracle, name)
    want = oracle_records(oracle, oracle_tables, a, b, mode, oargs)
    if name.startswith("loop") and k == 24:     # the limit bites: traced structures differ from the unlimited ones
        free = oracle_records(oracle, oracle_tables, a, b, mode)
        assert (want["ps1"] != free["ps1"]).any(axis=1).any(), (name, k, mode)
    assert_records(eng.thal_detail(a, b, chem, mode), want, k, (name, k, mode))


# ---- c. designed pairs, in one batch with ordinary pairs between them ---------------------------------------------------

def revcomp(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("a,b", [("ACGCGT", "ACGCGT"), ("GAATTC", "GGATCC"), ("ACGT", "ACGT")])
def test_two_self_complementary_oligos(eng, oracle, oracle_tables, a, b, mode):
    """Both oligos self-complementary: the second table set and RC constant (thal.c symmetry correction)."""
    want = oracle_records(oracle, oracle_tables, [a], [b], mode)
    assert_records(eng.thal_detail([a], [b], None, mode), want, len(a), (a, b, mode))


@pytest.mark.parametrize("mode", MODES)
def test_self_complementary_pairs_between_random_hexamers(eng, oracle, oracle_tables, mode):
    rng = random.Random(7406)
    sym = [("ACGCGT", "ACGCGT"), ("GAATTC", "GGATCC"), ("GGATCC", "GAATTC"), ("GAATTC", "GAATTC")]
    a, b = [], []
    for q in range(48):
        if q % 2 == 0:
            x, y = sym[(q // 2) % len(sym)]
        else:
            x, y = random_oligos(rng, 6, 2)
        a.append(x)
        b.append(y)
    # one self-complementary oligo against an ordinary one does not take the second table set
    a += ["ACGCGT", "CCGTAG"]
    b += ["CCGTAG", "ACGCGT"]
    want = oracle_records(oracle, oracle_tables, a, b, mode)
    assert_records(eng.thal_detail(a, b, None, mode), want, 6, mode)


@pytest.mark.parametrize("mode", MODES)
def test_records_do_not_depend_on_their_neighbours_13(eng, oracle, oracle_tables, mode):
    """Poly-A x poly-A (no structure) directly behind a 13-pair duplex; the END1 fallback to cell (1, 1); the golden
    13-mers; random pairs between them.  The same batch reversed gives the reversed records."""
    rng = random.Random(7413)
    full = "AGTCCTGCGTGAT"
    rnd = random_oligos(rng, 13, 12)
    a = [rnd[0], full, "A" * 13, rnd[1], "CCCCCCCCCCCCA", rnd[2], revcomp(full), "A" * 13, "T" * 13, "A" * 13,
         "AGGCCTATATCCA", rnd[3], "A" * 13, "G" * 13]
    b = [rnd[4], revcomp(full), "A" * 13, rnd[5], "GGGGGGGGGGGGG", rnd[6], full, "A" * 13, "A" * 13, "C" * 13,
         "GAAGCAGTATTTT", rnd[7], "A" * 13, "G" * 13]
    want = oracle_records(oracle, oracle_tables, a, b, mode)
    assert want["n_pairs"][1] == 13 and want["no_structure"][2] == 1          # the long structure, then none
    if mode == "end1":
        r = want[4]
        assert (r["no_structure"], r["n_pairs"], r["ps1"][0], r["ps2"][0]) == (0, 1, 1, 1)
        assert r["dH"] == 200.0 and r["dS"] == pytest.approx(-5.7, abs=1e-9)
    got = eng.thal_detail(a, b, None, mode)
    assert_records(got, want, 13, mode)
    assert_records(eng.thal_detail(a[::-1], b[::-1], None, mode), want[::-1], 13, (mode, "reversed"))


def test_end1_fallback_and_no_structure_on_pentamers(eng, oracle, oracle_tables):
    a = ["GGCAT", "CCCCA", "AAAAA", "ACCCA", "ATGCC", "CCCCA", "AAAAA"]
    b = ["ATGCC", "GGGGG", "AAAAA", "CCCCC", "GGCAT", "GGGGG", "TTTTT"]
    want = oracle_records(oracle, oracle_tables, a, b, "end1")
    r = want[1]
    assert (r["no_structure"], r["n_pairs"], r["ps1"][0], r["ps2"][0]) == (0, 1, 1, 1)     # thal's fallback cell
    assert r["dH"] == 200.0 and r["dS"] == pytest.approx(-5.7, abs=1e-9)
    assert want["no_structure"][2] == 1 and want["no_structure"][3] == 1
    assert_records(eng.thal_detail(a, b, None, "end1"), want, 5, "end1")
    assert_records(eng.thal_detail(a, b, None, "any"), oracle_records(oracle, oracle_tables, a, b, "any"), 5, "any")


def test_golden_dimers_through_the_binding(eng, m, oracle, oracle_tables, golden_dir):
    """od-msspe/src/delta_g.rs:196-230: the "%g" text of all four values and the traced pairs of the five vectors."""
    g = json.loads((golden_dir / "ntthal_dimer.json").read_text())
    vecs = g["vectors"]
    for temp in sorted({v["temp_c"] for v in vecs}):
        sel = [v for v in vecs if v["temp_c"] == temp]
        a, b = [v["oligo1"] for v in sel], [v["oligo2"] for v in sel]
        got = eng.thal_detail(a, b, m.Chem.ntthal(temp_c=temp), "any")
        assert_records(got, oracle_records(oracle, oracle_tables, a, b, "any", oracle.ntthal_args(temp_c=temp)), 13, temp)
        for v, r in zip(sel, got):
            assert tuple("%g" % r[f] for f in DOUBLES) == (v["dS"], v["dH"], v["dG"], v["t"]), v["id"]
            assert [[i + 1, int(j)] for i, j in enumerate(r["ps1"]) if j] == v["pairs"], v["id"]
            assert r["n_pairs"] == len(v["pairs"])


# ---- d. more problems than workspace lanes ------------------------------------------------------------------------------

def test_more_pairs_than_workspace_lanes(eng, oracle, oracle_tables):
    """65,536 + 300 pentamer pairs: lanes 0..299 run a second problem and write a second record."""
    n = LANES + 300
    rng = random.Random(7505)
    bases = rng.choices("ACGT", k=2 * 5 * n)
    a = ["".join(bases[5 * q:5 * q + 5]) for q in range(n)]
    b = ["".join(bases[5 * (n + q):5 * (n + q) + 5]) for q in range(n)]
    got = eng.thal_detail(a, b, None, "any")
    assert got.shape == (n,)
    for lo in (0, LANES):
        want = oracle_records(oracle, oracle_tables, a[lo:lo + 300], b[lo:lo + 300], "any")
        assert_records(got[lo:lo + 300], want, 5, lo)
    want = oracle_records(oracle, oracle_tables, a, b, "any", full=False)
    for f in ("dG", "t", "no_structure"):
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (f, int(bad[0]), got[f][bad[0]], want[f][bad[0]], int(bad.size))
    assert 0 < (want["no_structure"] != 0).sum() < n


# ---- e. the record agrees with the screens ------------------------------------------------------------------------------

@pytest.mark.parametrize("k,n", [(13, 64), (20, 24)])
def test_record_agrees_with_the_screens(eng, m, k, n):
    """What the shim prints is what the fast kernels decide on: dG and t of msspe_cross_dimer / msspe_cross_dimer_end
    over all ordered pairs of a pool equal the record's."""
    pool = random_oligos(random.Random(7600 + k), k, n)
    a = [pool[i] for i in range(n) for j in range(n)]
    b = [pool[j] for i in range(n) for j in range(n)]
    chem = m.Chem.ntthal()
    screens = {"any": eng.cross_dimer(pool, chem, -9000.0, want_dg=True, want_tm=True),
               "end1": eng.cross_dimer_end(pool, chem, want_dg=True, want_tm=True)}
    for mode, out in screens.items():
        det = eng.thal_detail(a, b, chem, mode)
        dg, tm = out["dg"].reshape(-1), out["tm"].reshape(-1)
        finite = np.isfinite(dg)
        assert (dg[~finite] == np.inf).all()
        assert finite.any() and (mode == "any" or k != 13 or (~finite).any()), mode   # 13-mers: both branches met
        np.testing.assert_array_equal(det["no_structure"], (~finite).astype(np.int32), err_msg=mode)
        np.testing.assert_array_equal(det["dG"][finite], dg[finite], err_msg=mode)
        np.testing.assert_array_equal(det["t"], tm, err_msg=mode)
        assert (tm[~finite] == 0.0).all(), mode


# ---- f. argument statuses -----------------------------------------------------------------------------------------------

def test_argument_statuses(eng, m):
    from msspe_amd.capi import THAL_DETAIL_DTYPE
    ERR_ARG, ERR_K = 1, 2
    assert (m.STATUS[ERR_ARG], m.STATUS[ERR_K]) == ("MSSPE_ERR_ARG", "MSSPE_ERR_K")
    chem = m.Chem.ntthal()
    out = np.zeros(2, dtype=THAL_DETAIL_DTYPE)
    call = lambda a, b, n, k, mode: eng.L.msspe_thal_detail_pairs(eng.ptr, a, b, n, k, C.byref(chem), mode,
                                                                  out.ctypes.data)
    ok = b"ACGTACGTAC"
    assert call(ok, ok, 2, 5, 1) == 0 and call(ok, ok, 2, 5, 2) == 0
    assert call(ok, ok, 2, 5, 0) == ERR_ARG and call(ok, ok, 2, 5, 3) == ERR_ARG
    assert call(None, ok, 2, 5, 1) == ERR_ARG and call(ok, None, 2, 5, 1) == ERR_ARG
    assert eng.L.msspe_thal_detail_pairs(eng.ptr, ok, ok, 2, 5, C.byref(chem), 1, None) == ERR_ARG
    assert call(ok, ok, 2, 1, 1) == ERR_K
    assert call(b"A" * 66, b"T" * 66, 2, 33, 1) == ERR_K
    assert call(b"ACGTNCGTAC", ok, 2, 5, 1) == ERR_ARG and call(ok, b"ACGTACGTAU", 2, 5, 1) == ERR_ARG
    out.view(np.uint8)[:] = 0xA5
    assert call(ok, ok, 0, 5, 1) == 0
    assert (out.view(np.uint8) == 0xA5).all()                      # n == 0: MSSPE_OK, nothing written
    # the same through Engine.thal_detail
    for mode in (0, 3):
        with pytest.raises(m.MsspeError) as e:
            eng.thal_detail(["ACGTA"], ["ACGTA"], None, mode)
        assert e.value.code == ERR_ARG
    for k in (1, 33):
        with pytest.raises(m.MsspeError) as e:
            eng.thal_detail(["A" * k], ["T" * k])
        assert e.value.code == ERR_K
    with pytest.raises(m.MsspeError) as e:
        eng.thal_detail(["ACGTN"], ["ACGTA"])
    assert e.value.code == ERR_ARG
    with pytest.raises(m.MsspeError):
        eng.thal_detail(["ACGTA", "ACGTA"], ["ACGTA"])
    with pytest.raises(m.MsspeError):
        eng.thal_detail(["ACGTA"], ["ACGT"])
    assert eng.thal_detail([], []).shape == (0,)
