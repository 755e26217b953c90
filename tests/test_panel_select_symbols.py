"""The selection by coverage's interface without a GPU: the header declares the four msspe_panel_select* calls and
msspe_select_opt and states the rule, the library exports them, the binding's EXPORTS lists them, a NULL context is an
argument error, and the CLI takes --select-by-coverage (env SELECT_BY_COVERAGE, default false) with --thin-panel's
values and refuses the combinations it cannot serve."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
NAMES = ["msspe_panel_select", "msspe_panel_select_bitmap", "msspe_panel_select_dev", "msspe_panel_select_packed_dev"]
ENV = ("SELECT_BY_COVERAGE", "THIN_PANEL", "THIN_MISMATCHES", "THIN_3P_EXACT", "THIN_MIN_GAIN", "THIN_TM", "THIN_THAL",
       "KMER_SIZE", "KEEP_ALL", "MSSPE_DEVICES", "COVER_ON_DEVICE", "TUBES", "EXISTING_PRIMERS", "REPICK_ROUNDS")


@pytest.fixture(scope="module")
def lib():
    import msspe_amd
    return msspe_amd.load_library()


@pytest.fixture(scope="module")
def host(lib):
    return C.CDLL(str(HOST_LIB))


def test_library_exports_the_selection(lib, host):
    for name in NAMES:
        assert hasattr(lib, name), name
    assert hasattr(host, "odm_select_panel")


def test_header_and_binding_list_the_selection():
    import msspe_amd
    from msspe_amd import capi
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    for name in NAMES:
        assert name in capi.EXPORTS, name
        assert f"int {name}(" in header, name
    assert "} msspe_select_opt;" in header
    assert [f[0] for f in msspe_amd.SelectOpt._fields_] == ["min_gain", "max_tubes", "drop_self_pairs"]
    for key in ("panel_select_rounds", "panel_select_tubes", "panel_select_barred", "panel_select_prepare_us",
                "panel_select_incidence_us", "panel_select_rounds_us"):
        assert f'"{key}"' in header, key
    flat = " ".join(header.replace(" *", " ").split())
    for words in ("Ties go to the LOWEST index", "tube(p) = the lowest tube not in mask[p]",
                  "mask[u] |= 1 << tube(p) for every u != p with S[p][u] set",
                  "Every neighbour of a forced primer starts with all T bits set",
                  "No two picks of one tube are neighbours in S", "does NOT promise"):
        assert words in flat, words


def test_null_context_is_an_argument_error(lib):
    from msspe_amd import Chem, KmerOpt, SelectOpt, seed_rule
    g = np.full((2, 600), ord("A"), dtype=np.uint8)
    w = np.array([1, 2], dtype=np.uint64)
    bits = np.zeros(2, dtype=np.uint64)
    keep, tube, barred = np.zeros(2, np.uint8), np.zeros(2, np.uint8), np.zeros(2, np.uint8)
    order, gains = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    n = C.c_int(-1)
    opt, rule, sel, chem = KmerOpt(500, 250, 50, 13, 0, 0), seed_rule(1, 3), SelectOpt(1, 1, 0), Chem.ntthal()
    head = (None, g.ctypes.data, 2, 600, C.byref(opt), C.byref(rule), C.byref(sel), w.ctypes.data, 1,
            w[1:].ctypes.data, 1, None)
    tail = (keep.ctypes.data, order.ctypes.data, gains.ctypes.data, C.byref(n), tube.ctypes.data, barred.ctypes.data,
            None, None, None, None)
    for name in NAMES:
        graph = (C.byref(chem), C.c_float(-9000.0)) if name == "msspe_panel_select" else (bits.ctypes.data,)
        assert getattr(lib, name)(*head, *graph, *tail) == 1, name


def parse(host, *a):
    argv = (C.c_char_p * (len(a) + 1))(b"od-msspe-hip", *[x.encode() for x in a])
    buf = C.create_string_buffer(1 << 16)
    rc = host.odm_parse_args(len(a) + 1, argv, buf, 1 << 16)
    return rc, buf.value.decode()


def values(out):
    kv = dict(l.split("=", 1) for l in out.splitlines())
    return (kv["select_by_coverage"], kv["thin_panel"], kv["thin_mismatches"], kv["thin_3p_exact"], kv["thin_min_gain"],
            kv["thin_tm"], kv["thin_thal"], kv["tubes"])


def test_cli_flag(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv")
    assert rc == 0 and values(out) == ("false", "false", "0", "3", "1", "", "", "0")
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--select-by-coverage", "true", "--thin-mismatches", "2",
                    "--thin-3p-exact=5", "--thin-min-gain", "4", "--tubes", "8", "--thin-tm", "30", "--thin-thal",
                    "end1")
    assert rc == 0 and values(out) == ("true", "false", "2", "5", "4", "30", "end1", "8")
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--select-by-coverage=true", "--thin-tm", "25")
    assert rc == 0 and values(out)[5:7] == ("25", "any")
    # the --thin-* values are read with this switch exactly as with --thin-panel
    for bad in (("--select-by-coverage", "yes"), ("--select-by-coverage", "true", "--thin-mismatches", "14"),
                ("--select-by-coverage", "true", "--thin-3p-exact", "14"),
                ("--select-by-coverage", "true", "--thin-3p-exact", "two"),
                ("--select-by-coverage", "true", "--thin-min-gain", "0"),
                ("--select-by-coverage", "true", "--thin-tm", "warm"),
                ("--select-by-coverage", "true", "--thin-tm", "30", "--thin-thal", "both"),
                ("--select-by-coverage", "true", "--tubes", "65")):
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", *bad)
        assert rc == 2 and ("--thin-" in out or "--select-by-coverage" in out or "--tubes" in out), (bad, out)
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--thin-mismatches", "99", "--thin-min-gain", "0")
    assert rc == 0 and values(out)[0] == "false"
    monkeypatch.setenv("SELECT_BY_COVERAGE", "true")
    monkeypatch.setenv("THIN_MISMATCHES", "1")
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv")
    assert rc == 0 and values(out)[:3] == ("true", "false", "1")
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--select-by-coverage", "false")
    assert rc == 0 and values(out)[0] == "false"
    rc, out = parse(host, "--help")
    assert rc == 2 and "--select-by-coverage <...>  [env: SELECT_BY_COVERAGE=]" in out
    assert "Conflicts may cost segments" in out


def test_flag_combinations_are_usage_errors(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    for extra in (("--thin-panel", "true"), ("--keep-all", "true"), ("--devices", "0,0"),
                  ("--cover-on-device", "true")):
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--select-by-coverage", "true", *extra)
        assert rc == 2 and extra[0] in out and "--select-by-coverage" in out, (extra, out)
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--select-by-coverage", "false", *extra)
        assert rc == 0, extra
    # --tubes with --existing-primers stays the error it is
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--select-by-coverage", "true", "--tubes", "4",
                    "--existing-primers", "panel.csv")
    assert rc == 2 and "--tubes" in out and "--existing-primers" in out
    # the panel, the tubes, the re-pick rounds and the rejected list go with the switch
    for extra in (("--existing-primers", "panel.csv"), ("--tubes", "4"), ("--repick-rounds", "2"),
                  ("--rejected-out", "r.csv"), ("--check-self-dimers", "false"), ("--check-cross-dimers", "false")):
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--select-by-coverage", "true", *extra)
        assert rc == 0, (extra, out)
