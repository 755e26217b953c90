"""The model of the flanked background score (tests/background_flank_model.py) against first principles, the C ABI's
four new symbols and the CLI's --background-flank; no GPU."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import background_flank_model as bfm
import background_model as bm
import background_thal_model as btm

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["msspe_background_thal_flank_packed_dev", "msspe_background_thal_flank",
         "msspe_background_amplicons_flank_packed_dev", "msspe_background_amplicons_flank"]


@pytest.fixture(scope="module")
def host():
    p = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
    if not p.exists():
        pytest.fail(f"{p} is missing: run open-msspe-design_amd/build.sh")
    return C.CDLL(str(p))


def random_seq(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def test_flank_0_is_the_scored_site_model(oracle, oracle_tables):
    rng = np.random.default_rng(11)
    primers = [random_seq(rng, 9) for _ in range(6)]
    records = [random_seq(rng, 3000) + "N" + primers[0] + "n" + bm.revcomp(primers[1]), "", random_seq(rng, 400)]
    args = oracle.ntthal_args()
    for mode in ("any", "end1"):
        want = btm.scored_sites(oracle_tables, records, primers, 2, 1, mode, 20.0, args)
        got = bfm.scored_sites(oracle_tables, records, primers, 2, 1, mode, 20.0, args, flank=0)
        assert len(want[2]) > 20
        for a, b in zip(want, got):
            np.testing.assert_array_equal(a, b)
    sites = bm.sites(records, primers, 2, 1)[1]
    assert bfm.template_oligos(records, primers, sites, 0) == btm.template_oligos(records, primers, sites)
    assert bfm.class_stats(records, primers, sites, 0) == (1, 0)


# k = 5 windows in a stream of two records: columns 0..9 record 0, 10 the separator, 11..31 record 1, whose column 19
# is a lower-case base and whose column 25 is an N
STREAM_RECORDS = ["GATTACAGGC", "TTGACGTAnCCGGANACGTCA"]
HAND = [
    # (pos, f, (fl, fr), extended window)
    (0, 2, (0, 2), "GATTACA"),          # stream column 0
    (0, 4, (0, 4), "GATTACAGG"),
    (27, 2, (1, 0), "ACGTCA"),          # ends at the last column; the N two columns to the left
    (26, 2, (0, 1), "ACGTCA"),          # next to the N; one column from the stream's end
    (5, 2, (2, 0), "TACAGGC"),          # ends at the separator
    (4, 2, (2, 1), "TTACAGGC"),         # one column from it
    (3, 2, (2, 2), "ATTACAGGC"),        # two columns from it
    (3, 4, (3, 2), "GATTACAGGC"),       # the stream's start on the left, the separator on the right
    (11, 2, (0, 2), "TTGACGT"),         # begins behind the separator
    (12, 2, (1, 2), "TTGACGTA"),        # one column behind it
    (13, 2, (2, 1), "TTGACGTA"),        # two columns behind it; the lower-case base two columns to the right
    (14, 2, (2, 0), "TGACGTA"),         # next to the lower-case base
    (20, 2, (0, 0), "CCGGA"),           # between the lower-case base and the N
    (2, 1, (1, 1), "ATTACAG"),          # in the clear
    (2, 2, (2, 2), "GATTACAGG"),
]


@pytest.mark.parametrize("pos,f,want,window", HAND)
def test_hand_written_flanks(pos, f, want, window):
    stream = btm.stream_text(STREAM_RECORDS)
    assert len(stream) == 32 and stream[10] == "-" and stream[19] == "n" and stream[25] == "N"
    k = 5
    assert bfm.flanks(stream, k, pos, f) == want
    fl, fr = want
    assert stream[pos - fl:pos + k + fr] == window
    assert bfm.template_oligo(stream, k, pos, 1, f) == window
    assert bfm.template_oligo(stream, k, pos, 0, f) == bm.revcomp(window)
    assert set(window) <= set("ACGT")
    assert len(window) == k + fl + fr


def test_flanks_next_to_iupac_and_gap():
    stream = "ACGTRACGTAC-ACGTACGTYAC"
    assert bfm.flanks(stream, 4, 5, 3) == (0, 2)      # R on the left, '-' two columns to the right
    assert bfm.flanks(stream, 4, 14, 3) == (2, 2)     # '-' two columns to the left, Y two to the right
    assert bfm.flanks(stream, 4, 16, 4) == (4, 0)


def test_an_exact_site_with_full_flanks_holds_the_reverse_complement_of_the_primer():
    rng = np.random.default_rng(4)
    k, f = 11, 3
    u = random_seq(rng, k)
    records = [random_seq(rng, 40) + u + random_seq(rng, 40), random_seq(rng, 30) + bm.revcomp(u) + random_seq(rng, 30)]
    _counts, sites = bm.sites(records, [u], 0, 0)
    assert set(sites["strand"].tolist()) == {0, 1}
    for r, o2 in zip(sites, bfm.template_oligos(records, [u], sites, f)):
        assert len(o2) == k + 2 * f and o2[f:f + k] == bm.revcomp(u)
    assert bfm.class_stats(records, [u], sites, f) == (1, 0)


# The seed of test_the_flank_changes_a_decision: the first seed of 0, 1, 2, ... at which the case below holds a site
# whose stable bit at 30 C differs between flank 0 and flank 2 (found on the CPU with the oracle).
FLANK_SEED = 2


def flank_case(seed):
    rng = np.random.default_rng(seed)
    primers = [random_seq(rng, 13) for _ in range(8)]
    recs = [list(random_seq(rng, 4000))]
    for j, p in enumerate(primers):   # one exact copy and one one-mismatch copy of each, alternating strands
        for c in range(2):
            w = list(p)
            if c:
                q = int(rng.integers(0, 10))
                w[q] = "ACGT"[("ACGT".index(w[q]) + 1) % 4]
            w = "".join(w)
            a = 100 + 230 * (2 * j + c)
            recs[0][a:a + 13] = w if (j + c) % 2 else bm.revcomp(w)
    return ["".join(recs[0])], primers


def test_the_flank_changes_a_decision(oracle, oracle_tables):
    records, primers = flank_case(FLANK_SEED)
    args = oracle.ntthal_args()
    _c, s0, r0 = bfm.scored_sites(oracle_tables, records, primers, 2, 2, "any", 30.0, args, flank=0)
    _c, s2, r2 = bfm.scored_sites(oracle_tables, records, primers, 2, 2, "any", 30.0, args, flank=2)
    for f in ("primer", "pos", "mismatches", "strand"):
        np.testing.assert_array_equal(r0[f], r2[f])          # the sites do not depend on the flank
    differ = np.flatnonzero(r0["stable"] != r2["stable"])
    print(f"{len(r0)} sites, {len(differ)} change their stable bit with flank 2; "
          f"t moves by up to {np.abs(r2['t'] - r0['t']).max():.2f} C")
    assert len(differ) >= 1
    assert (r0["t"] != r2["t"]).sum() > len(r0) // 2


def test_render():
    base = btm.render(["Primer_0_F"], [[7, 5]], [[2, 1]], 2, 3, "any", 30.0)
    assert bfm.render(["Primer_0_F"], [[7, 5]], [[2, 1]], 2, 3, "any", 30.0, 0) == base
    text = bfm.render(["Primer_0_F"], [[7, 5]], [[2, 1]], 2, 3, "any", 30.0, 2)
    assert text == ("\nBackground sites (up to 2 mismatches, last 3 bases exact; stable: thal ANY t >= 30.00 C, "
                    "template flank 2):\n"
                    "  Primer_0_F: plus 7, minus 5, stable plus 2, minus 1\n"
                    "  Total: 1 primers, plus 7, minus 5, stable plus 2, minus 1\n")


def test_symbols_bindings_and_null_context():
    import inspect

    import msspe_amd
    from msspe_amd import capi
    lib = msspe_amd.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    for key in ('"background_thal_flank_classes"', '"background_thal_truncated"'):
        assert key in header
    for method in ("background_thal", "background_thal_packed", "background_amplicons", "background_amplicons_packed"):
        p = inspect.signature(getattr(capi.Engine, method)).parameters
        assert "flank" in p and p["flank"].default == 0, method
    mm, chem, amp = capi.MismatchOpt(2, 3), capi.Chem.ntthal(), capi.AmpliconOpt(13, 500)
    out = (C.c_uint64 * 2)()
    words = (C.c_uint64 * 1)(0)
    count, total = C.c_uint64(), C.c_uint64()
    assert lib.msspe_background_thal_flank_packed_dev(None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1, 30.0,
                                                      2, out, out, None, 0, None) == 1
    assert lib.msspe_background_thal_flank(None, None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1, 30.0, 2,
                                           out, out, None, 0, C.byref(count), None) == 1
    assert lib.msspe_background_amplicons_flank_packed_dev(None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1,
                                                           30.0, 2, C.byref(amp), None, 0, out, out, out,
                                                           C.byref(total), None, 0, None) == 1
    assert lib.msspe_background_amplicons_flank(None, None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1, 30.0,
                                                2, C.byref(amp), out, out, out, C.byref(total), None, 0,
                                                C.byref(count), None) == 1


def parse(host, *a):
    argv = (C.c_char_p * (len(a) + 1))(b"od-msspe-hip", *[x.encode() for x in a])
    buf = C.create_string_buffer(1 << 16)
    rc = host.odm_parse_args(len(a) + 1, argv, buf, 1 << 16)
    out = buf.value.decode()
    return rc, (dict(l.split("=", 1) for l in out.splitlines()) if rc == 0 else out)


ENV = ["BACKGROUND", "BACKGROUND_MISMATCHES", "BACKGROUND_3P_EXACT", "MAX_BACKGROUND_SITES", "BACKGROUND_TM",
       "BACKGROUND_THAL", "BACKGROUND_FLANK", "KMER_SIZE"]


def test_cli_flag(host, monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    base = ("-i", "a.fa", "-o", "b.csv")
    rc, kv = parse(host, *base, "--background", "h.fa", "--background-tm", "30")
    assert rc == 0 and kv["background_flank"] == "0"
    rc, kv = parse(host, *base, "--background", "h.fa", "--background-tm", "30", "--background-flank", "2")
    assert rc == 0 and kv["background_flank"] == "2"
    rc, out = parse(host, *base, "--background-flank", "2")
    assert rc == 2 and "'--background-flank' needs '--background <FASTA>'" in out
    rc, out = parse(host, *base, "--background", "h.fa", "--background-flank", "2")
    assert rc == 2 and "'--background-flank' needs '--background-tm <C>'" in out
    for bad in ("5", "-1", "two"):
        rc, out = parse(host, *base, "--background", "h.fa", "--background-tm", "30", "--background-flank", bad)
        assert rc == 2 and f"invalid value '{bad}' for '--background-flank" in out, bad
    rc, out = parse(host, *base, "--background", "h.fa", "--background-tm", "30", "--kmer-size", "26",
                    "--background-flank", "4")
    assert rc == 2 and "'--kmer-size 26' with '--background-flank 4' is longer than 32 bases" in out
    rc, kv = parse(host, *base, "--background", "h.fa", "--background-tm", "30", "--kmer-size", "24",
                   "--background-flank", "4")
    assert rc == 0 and kv["background_flank"] == "4"
    monkeypatch.setenv("BACKGROUND_FLANK", "3")
    rc, kv = parse(host, *base, "--background", "h.fa", "--background-tm", "30")
    assert rc == 0 and kv["background_flank"] == "3"
    rc, kv = parse(host, *base, "--background", "h.fa", "--background-tm", "30", "--background-flank=1")
    assert rc == 0 and kv["background_flank"] == "1"            # the command line wins
    rc, out = parse(host, *base, "--help")
    assert rc == 2 and "--background-flank <...>  [env: BACKGROUND_FLANK=]" in out
