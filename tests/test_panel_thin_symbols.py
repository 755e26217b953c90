"""The panel thinning's interface without a GPU: the header declares msspe_panel_thin / _dev / _packed_dev, the library
exports them, the binding's EXPORTS lists them, a NULL context is an argument error, and the CLI takes --thin-panel
(env THIN_PANEL, default false) with --thin-mismatches, --thin-3p-exact and --thin-min-gain."""
import ctypes as C
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
NAMES = ["msspe_panel_thin", "msspe_panel_thin_dev", "msspe_panel_thin_packed_dev"]
ENV = ("THIN_PANEL", "THIN_MISMATCHES", "THIN_3P_EXACT", "THIN_MIN_GAIN", "KMER_SIZE", "KEEP_ALL", "MSSPE_DEVICES")


@pytest.fixture(scope="module")
def lib():
    import msspe_amd
    return msspe_amd.load_library()


@pytest.fixture(scope="module")
def host(lib):
    return C.CDLL(str(HOST_LIB))


def test_library_exports_the_thinning(lib, host):
    for name in NAMES:
        assert hasattr(lib, name), name
    assert hasattr(host, "odm_thin_panel")


def test_header_and_binding_list_the_thinning():
    from msspe_amd import capi
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    for name in NAMES:
        assert name in capi.EXPORTS, name
        assert f"int {name}(" in header, name
    assert "} msspe_thin_opt;" in header
    for key in ("panel_thin_rounds", "panel_thin_groups", "panel_thin_incidence_us", "panel_thin_rounds_us",
                "panel_thin_matrix_max_mb"):
        assert f'"{key}"' in header, key
    assert "does NOT preserve" in header   # the smallest mismatch count per segment


def test_null_context_is_an_argument_error(lib):
    import numpy as np
    from msspe_amd import KmerOpt, MismatchOpt, ThinOpt
    g = np.full((2, 600), ord("A"), dtype=np.uint8)
    w = np.zeros(1, dtype=np.uint64)
    keep, order, gains = np.zeros(2, np.uint8), np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    n = C.c_int(-1)
    opt, mm, thin = KmerOpt(500, 250, 50, 13, 0, 0), MismatchOpt(1, 3), ThinOpt(1)
    for name in NAMES:
        assert getattr(lib, name)(None, g.ctypes.data, 2, 600, C.byref(opt), C.byref(mm), C.byref(thin),
                                  w.ctypes.data, 1, w.ctypes.data, 1, None, keep.ctypes.data, order.ctypes.data,
                                  gains.ctypes.data, C.byref(n), None, None, None) == 1, name


def parse(host, *a):
    argv = (C.c_char_p * (len(a) + 1))(b"od-msspe-hip", *[x.encode() for x in a])
    buf = C.create_string_buffer(1 << 16)
    rc = host.odm_parse_args(len(a) + 1, argv, buf, 1 << 16)
    return rc, buf.value.decode()


def thin_of(out):
    kv = dict(l.split("=", 1) for l in out.splitlines())
    return kv["thin_panel"], kv["thin_mismatches"], kv["thin_3p_exact"], kv["thin_min_gain"]


def test_cli_flags(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv")
    assert rc == 0 and thin_of(out) == ("false", "0", "3", "1")
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--thin-panel", "true", "--thin-mismatches", "2",
                    "--thin-3p-exact=5", "--thin-min-gain", "4")
    assert rc == 0 and thin_of(out) == ("true", "2", "5", "4")
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--thin-panel", "true", "--thin-mismatches", "13",
                    "--thin-3p-exact", "13")
    assert rc == 0 and thin_of(out) == ("true", "13", "13", "1")
    for bad in (("--thin-panel", "yes"), ("--thin-panel", "true", "--thin-mismatches", "14"),
                ("--thin-panel", "true", "--thin-mismatches", "-1"), ("--thin-mismatches", "x"),
                ("--thin-panel", "true", "--thin-3p-exact", "14"), ("--thin-panel", "true", "--thin-3p-exact", "two"),
                ("--thin-panel", "true", "--thin-3p-exact", "-2"), ("--thin-panel", "true", "--thin-min-gain", "0"),
                ("--thin-min-gain", "-3"), ("--kmer-size", "8", "--thin-panel", "true", "--thin-mismatches", "9")):
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", *bad)
        assert rc == 2 and "--thin-" in out, (bad, out)
    # without the switch the values are not read beyond their form
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--thin-mismatches", "99", "--thin-3p-exact", "many",
                    "--thin-min-gain", "0")
    assert rc == 0 and thin_of(out)[0] == "false"
    monkeypatch.setenv("THIN_PANEL", "true")
    monkeypatch.setenv("THIN_MISMATCHES", "1")
    monkeypatch.setenv("THIN_3P_EXACT", "0")
    monkeypatch.setenv("THIN_MIN_GAIN", "2")
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv")
    assert rc == 0 and thin_of(out) == ("true", "1", "0", "2")
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--thin-panel", "false")
    assert rc == 0 and thin_of(out)[0] == "false"
    rc, out = parse(host, "--help")
    assert rc == 2
    for flag, env in (("--thin-panel", "THIN_PANEL"), ("--thin-mismatches", "THIN_MISMATCHES"),
                      ("--thin-3p-exact", "THIN_3P_EXACT"), ("--thin-min-gain", "THIN_MIN_GAIN")):
        assert f"{flag} <...>  [env: {env}=]" in out
    assert "best mismatch\ncount may rise" in out or "best mismatch count may rise" in out.replace("\n", " ")


def test_flag_combinations_are_usage_errors(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    for extra in (("--keep-all", "true"), ("--devices", "0,0")):
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--thin-panel", "true", *extra)
        assert rc == 2 and extra[0] in out and "--thin-panel" in out, extra
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--thin-panel", "false", *extra)
        assert rc == 0, extra
    # the panel of --existing-primers and the tubes go with the switch
    for extra in (("--existing-primers", "panel.csv"), ("--tubes", "4"), ("--cover-on-device", "true")):
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--thin-panel", "true", *extra)
        assert rc == 0, (extra, out)
