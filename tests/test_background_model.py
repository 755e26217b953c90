"""The background screen without a GPU: the numpy model (tests/background_model.py) against a string-compare triple
loop and hand-made cases; the library exports msspe_background_sites* and rejects a NULL context; the CLI takes
--background, --background-mismatches, --background-3p-exact and --max-background-sites with their env names, defaults
and usage errors."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import background_model as bm

ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
NAMES = ["msspe_device_put_stream_packed", "msspe_background_sites_packed_dev", "msspe_background_sites"]


def random_seq(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


# ---- the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,M,E", [(5, 0, 0), (5, 1, 2), (6, 2, 0), (6, 2, 3), (7, 3, 7), (4, 4, 0)])
def test_model_equals_the_triple_loop(k, M, E):
    rng = np.random.default_rng(100 * k + 10 * M + E)
    records = [random_seq(rng, 60), "", random_seq(rng, 3), random_seq(rng, 40) + "NN" + random_seq(rng, 30).lower()
               + random_seq(rng, 25), random_seq(rng, k)]
    primers = [random_seq(rng, k) for _ in range(6)] + [records[0][10:10 + k], bm.revcomp(records[3][5:5 + k])]
    counts, sites = bm.sites(records, primers, M, E)
    want_counts, want_sites = bm.naive_sites(records, primers, M, E)
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_array_equal(sites, want_sites)
    assert counts.sum() > 0
    # a wider candidate pass filtered down gives the same
    c2, s2 = bm.sites(records, primers, M, E, cand=bm.candidates(records, primers, min(k, M + 1)))
    np.testing.assert_array_equal(c2, counts)
    np.testing.assert_array_equal(s2, sites)


PRIMER = "ACGGTCATTGCA"   # 12 bases, not a palindrome, far from the filler below
FILL = "TTTTTTTTTTTTTTTTTTTT"


def mutate(s, positions):
    out = list(s)
    for q in positions:
        out[q] = "ACGT"[("ACGT".index(out[q]) + 1) % 4]
    return "".join(out)


def test_planted_perfect_site_on_each_strand():
    rec = FILL + PRIMER + FILL + bm.revcomp(PRIMER) + FILL
    counts, sites = bm.sites([rec], [PRIMER], 0, 0)
    assert counts.tolist() == [[1, 1]]
    assert sites.tolist() == [(0, 20, 0, 0), (0, 52, 0, 1)]


def test_exactly_m_and_m_plus_one_mismatches():
    M = 2
    rec = FILL + mutate(PRIMER, [1, 4]) + FILL + mutate(PRIMER, [1, 4, 6]) + FILL
    counts, sites = bm.sites([rec], [PRIMER], M, 0)
    assert counts.tolist() == [[1, 0]] and sites.tolist() == [(0, 20, 2, 0)]
    assert bm.sites([rec], [PRIMER], M + 1, 0)[0].tolist() == [[2, 0]]


def test_mismatch_inside_and_just_outside_the_3p_end():
    k, E = len(PRIMER), 3
    inside, outside = mutate(PRIMER, [k - E]), mutate(PRIMER, [k - E - 1])
    rec = FILL + inside + FILL + outside + FILL
    counts, sites = bm.sites([rec], [PRIMER], 1, E)
    assert sites.tolist() == [(0, 20 + k + 20, 1, 0)]
    assert bm.sites([rec], [PRIMER], 1, 0)[0].tolist() == [[2, 0]]
    # minus strand: the primer's 3' end is the window's FIRST bases
    rec = FILL + bm.revcomp(inside) + FILL + bm.revcomp(outside) + FILL
    assert bm.sites([rec], [PRIMER], 1, E)[1].tolist() == [(0, 20 + k + 20, 1, 1)]


def test_invalid_columns_and_record_borders():
    k = len(PRIMER)
    with_n = PRIMER[:5] + "N" + PRIMER[6:]
    counts, _ = bm.sites([FILL + with_n + FILL], [PRIMER], 1, 0)
    assert counts.tolist() == [[0, 0]]          # one mismatch would do, but N is not a base
    counts, _ = bm.sites([FILL + PRIMER.lower() + FILL], [PRIMER], 0, 0)
    assert counts.tolist() == [[0, 0]]          # lower case is not a base either
    counts, _ = bm.sites([FILL + PRIMER[:6], PRIMER[6:] + FILL], [PRIMER], 1, 0)
    assert counts.tolist() == [[0, 0]]          # the window would straddle two records
    counts, sites = bm.sites([FILL + PRIMER[:6], PRIMER[6:] + FILL, PRIMER], [PRIMER], 0, 0)
    starts, total = bm.record_starts([FILL + PRIMER[:6], PRIMER[6:] + FILL, PRIMER])
    assert starts.tolist() == [0, 27, 54] and total == 66 and sites.tolist() == [(0, 54, 0, 0)]


def test_palindrome_counts_on_both_strands_and_duplicates_independently():
    pal = "ACGTACGTACGT"
    assert bm.revcomp(pal) == pal
    counts, sites = bm.sites([FILL + pal + FILL], [pal, PRIMER, pal], 0, 0)
    assert counts.tolist() == [[1, 1], [0, 0], [1, 1]]
    assert sites.tolist() == [(0, 20, 0, 0), (0, 20, 0, 1), (2, 20, 0, 0), (2, 20, 0, 1)]


def overlapping_count(hay, needle):
    return sum(hay.startswith(needle, p) for p in range(len(hay) - len(needle) + 1))


def test_exact_counts_are_overlapping_occurrences():
    rng = np.random.default_rng(5)
    records = [random_seq(rng, 3000), "AAAAAAAAAAAAAAAAAAAA", random_seq(rng, 500)]
    primers = ["AAAA", "ACGT", "GATC", "TTTT", "CCGA", records[0][7:11]]
    counts, _ = bm.sites(records, primers, 0, 0)
    for i, p in enumerate(primers):
        assert counts[i, 0] == sum(overlapping_count(r, p) for r in records)
        assert counts[i, 1] == sum(overlapping_count(r, bm.revcomp(p)) for r in records)
    assert counts[0, 0] >= 17 and counts[3, 1] == counts[0, 0]


def test_render():
    text = bm.render(["Primer_0_F", "Primer_0_R"], np.array([[3, 0], [1, 2]], dtype=np.uint64), 2, 3)
    assert text == ("\nBackground sites (up to 2 mismatches, last 3 bases exact):\n  Primer_0_F: plus 3, minus 0\n"
                    "  Primer_0_R: plus 1, minus 2\n  Total: 2 primers, plus 4, minus 2\n")


# ---- the library and the CLI ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import msspe_amd
    return msspe_amd.load_library()


@pytest.fixture(scope="module")
def host(lib):
    return C.CDLL(str(HOST_LIB))


def test_library_exports_the_background_screen(lib):
    for name in NAMES:
        assert hasattr(lib, name), name


def test_binding_lists_the_background_screen():
    from msspe_amd import capi
    for name in NAMES:
        assert name in capi.EXPORTS, name
    assert capi.SITE_DTYPE.itemsize == 12 and capi.SITE_DTYPE == bm.SITE_DTYPE
    for method in ("put_stream_packed", "background_sites", "background_sites_packed"):
        assert hasattr(capi.Engine, method)
    assert "msspe_site" in (ROOT / "include" / "msspe_hip.h").read_text()


def test_null_context_is_an_argument_error(lib):
    from msspe_amd.capi import MismatchOpt
    mm = MismatchOpt(2, 3)
    out = (C.c_uint64 * 2)()
    words = (C.c_uint64 * 1)(0)
    dev, total, count = C.c_void_p(), C.c_size_t(), C.c_uint64()
    assert lib.msspe_device_put_stream_packed(None, None, None, 0, C.byref(dev), C.byref(total), None) == 1
    assert lib.msspe_background_sites_packed_dev(None, None, 0, 13, C.byref(mm), words, 1, out, None, 0, None) == 1
    assert lib.msspe_background_sites(None, None, None, 0, 13, C.byref(mm), words, 1, out, None, 0, C.byref(count),
                                      None) == 1


def parse(host, *a):
    argv = (C.c_char_p * (len(a) + 1))(b"od-msspe-hip", *[x.encode() for x in a])
    buf = C.create_string_buffer(1 << 16)
    rc = host.odm_parse_args(len(a) + 1, argv, buf, 1 << 16)
    out = buf.value.decode()
    return rc, (dict(l.split("=", 1) for l in out.splitlines()) if rc == 0 else out)


ENV = ["BACKGROUND", "BACKGROUND_MISMATCHES", "BACKGROUND_3P_EXACT", "MAX_BACKGROUND_SITES"]


def test_cli_flags_defaults_and_env(host, monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    rc, kv = parse(host, "-i", "a.fa", "-o", "b.csv")
    assert rc == 0 and kv["background"] == "" and kv["background_mismatches"] == "2"
    assert kv["background_3p_exact"] == "3" and kv["max_background_sites"] == "-1"
    rc, kv = parse(host, "-i", "a.fa", "-o", "b.csv", "--background", "host.fa")
    assert rc == 0 and kv["background"] == "host.fa" and kv["background_mismatches"] == "2"
    assert kv["background_3p_exact"] == "3" and kv["max_background_sites"] == "-1"
    rc, kv = parse(host, "-i", "a.fa", "-o", "b.csv", "--background=host.fa", "--background-mismatches", "1",
                   "--background-3p-exact", "0", "--max-background-sites", "40")
    assert rc == 0 and (kv["background_mismatches"], kv["background_3p_exact"], kv["max_background_sites"]) == \
        ("1", "0", "40")
    monkeypatch.setenv("BACKGROUND", "env.fa")
    monkeypatch.setenv("BACKGROUND_MISMATCHES", "3")
    monkeypatch.setenv("BACKGROUND_3P_EXACT", "5")
    monkeypatch.setenv("MAX_BACKGROUND_SITES", "7")
    rc, kv = parse(host, "-i", "a.fa", "-o", "b.csv")
    assert rc == 0 and (kv["background"], kv["background_mismatches"], kv["background_3p_exact"],
                        kv["max_background_sites"]) == ("env.fa", "3", "5", "7")
    rc, kv = parse(host, "-i", "a.fa", "-o", "b.csv", "--background-mismatches", "0")   # the command line wins
    assert rc == 0 and kv["background_mismatches"] == "0"


def test_cli_usage_errors(host, monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for flag in ("--background-mismatches", "--background-3p-exact", "--max-background-sites"):
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", flag, "1")
        assert rc == 2 and f"'{flag}' needs '--background <FASTA>'" in out
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--background", "h.fa", "--background-mismatches", "14")
    assert rc == 2 and "'--background-mismatches 14' is larger than '--kmer-size 13'" in out
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--background", "h.fa", "--background-3p-exact", "9",
                    "--kmer-size", "8")
    assert rc == 2 and "'--background-3p-exact 9' is larger than '--kmer-size 8'" in out
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--background", "h.fa", "--max-background-sites", "-1")
    assert rc == 2 and "invalid value '-1' for '--max-background-sites'" in out
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--help")
    assert rc == 2 and "--background <...>  [env: BACKGROUND=]" in out and "first device" in out
