"""The layered selection's interface without a GPU: the header declares the five msspe_panel_select_depth* calls, the
library exports them, the binding's EXPORTS lists them, a NULL context is an argument error, and the CLI takes
--select-depth (env SELECT_DEPTH, default 1, 1..255, read only with --select-by-coverage true) while --thin-depth above
1 with --select-by-coverage true stays the usage error it was."""
import ctypes as C
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
CALLS = ["msspe_panel_select_depth_dev", "msspe_panel_select_depth_packed_dev", "msspe_panel_select_depth",
         "msspe_panel_select_depth_bitmap", "msspe_panel_select_depth_rule"]
ENV = ("THIN_PANEL", "THIN_MISMATCHES", "THIN_3P_EXACT", "THIN_MIN_GAIN", "THIN_DEPTH", "THIN_TM", "THIN_THAL",
       "SELECT_BY_COVERAGE", "SELECT_DEPTH", "KMER_SIZE", "KEEP_ALL", "MSSPE_DEVICES", "TUBES")


@pytest.fixture(scope="module")
def lib():
    import msspe_amd
    return msspe_amd.load_library()


@pytest.fixture(scope="module")
def host(lib):
    return C.CDLL(str(HOST_LIB))


def test_library_exports_the_layered_selection(lib, host):
    for name in CALLS:
        assert hasattr(lib, name), name
    assert hasattr(host, "odm_select_panel_depth")


def test_header_and_binding_list_the_layered_selection():
    import msspe_amd
    from msspe_amd import capi
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    for name in CALLS:
        assert name in capi.EXPORTS, name
        assert f"int {name}(" in header, name
    assert "} msspe_select_depth_opt;" in header
    for key in ("panel_select_depth_layers", "panel_select_depth_layer_us"):
        assert f'"{key}"' in header, key
    for text in ("L = min(R, max(1, D))", "cnt[s] < min(r, depth_all[s])", "Rounds reported = picks + L",
                 "R = 1 is msspe_panel_select*", "depth_kept[s] >= min(R, depth_all[s])"):
        assert text in header, text
    opt = msspe_amd.SelectDepthOpt(3, 4, 1, 2)
    assert (opt.min_gain, opt.max_tubes, opt.drop_self_pairs, opt.depth) == (3, 4, 1, 2) and C.sizeof(opt) == 16
    assert callable(msspe_amd.Engine.panel_select_depth)


def test_null_context_is_an_argument_error(lib):
    import numpy as np
    from msspe_amd import Chem, ConflictRule, KmerOpt, SelectDepthOpt, seed_rule
    g = np.full((2, 600), ord("A"), dtype=np.uint8)
    w = np.zeros(1, dtype=np.uint64)
    keep, tube = np.zeros(2, np.uint8), np.zeros(2, np.uint8)
    order, gains, bits = np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros((2, 1), np.uint64)
    n = C.c_int(-1)
    opt, rule, sel, chem = KmerOpt(500, 250, 50, 13, 0, 0), seed_rule(1, 3), SelectDepthOpt(1, 1, 0, 2), Chem.ntthal()
    both = ConflictRule.of(-9000.0, 30.0)
    head = (None, g.ctypes.data, 2, 600, C.byref(opt), C.byref(rule), C.byref(sel), w.ctypes.data, 1, w.ctypes.data, 1,
            None)
    tail = (keep.ctypes.data, order.ctypes.data, gains.ctypes.data, C.byref(n), tube.ctypes.data, None, None, None,
            None, None, None)
    graphs = {"msspe_panel_select_depth": (C.byref(chem), C.c_float(-9000.0)),
              "msspe_panel_select_depth_rule": (C.byref(chem), C.byref(both))}
    for name in CALLS:
        assert getattr(lib, name)(*head, *graphs.get(name, (bits.ctypes.data,)), *tail) == 1, name


def parse(host, *a):
    argv = (C.c_char_p * (len(a) + 1))(b"od-msspe-hip", *[x.encode() for x in a])
    buf = C.create_string_buffer(1 << 16)
    rc = host.odm_parse_args(len(a) + 1, argv, buf, 1 << 16)
    return rc, buf.value.decode()


def kv_of(out):
    return dict(l.split("=", 1) for l in out.splitlines())


BASE = ("-i", "a.fa", "-o", "b.csv")
ON = BASE + ("--select-by-coverage", "true")


def test_cli_flag(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    rc, out = parse(host, *BASE)
    assert rc == 0 and kv_of(out)["select_depth"] == "1"
    rc, out = parse(host, *ON, "--select-depth", "3")
    assert rc == 0 and kv_of(out)["select_depth"] == "3" and kv_of(out)["select_by_coverage"] == "true"
    for ok in ("1", "255"):
        rc, out = parse(host, *ON, f"--select-depth={ok}")
        assert rc == 0 and kv_of(out)["select_depth"] == ok
    for bad in ("0", "256", "-1"):
        rc, out = parse(host, *ON, "--select-depth", bad)
        assert rc == 2 and "--select-depth" in out, (bad, out)     # "-1" already fails the option's form
        assert bad == "-1" or "[1 .. 255]" in out, (bad, out)
    rc, out = parse(host, *BASE, "--select-depth", "two")
    assert rc == 2 and "--select-depth" in out
    # without the switch the value is not read beyond its form
    rc, out = parse(host, *BASE, "--select-depth", "999")
    assert rc == 0 and kv_of(out)["select_by_coverage"] == "false"
    rc, out = parse(host, *BASE, "--thin-panel", "true", "--select-depth", "999")
    assert rc == 0
    monkeypatch.setenv("SELECT_BY_COVERAGE", "true")
    monkeypatch.setenv("SELECT_DEPTH", "4")
    rc, out = parse(host, *BASE)
    assert rc == 0 and kv_of(out)["select_depth"] == "4"
    rc, out = parse(host, *BASE, "--select-depth", "2")           # the command line goes before the environment
    assert rc == 0 and kv_of(out)["select_depth"] == "2"
    monkeypatch.setenv("SELECT_DEPTH", "300")
    rc, out = parse(host, *BASE)
    assert rc == 2 and "--select-depth" in out
    rc, out = parse(host, "--help")
    assert rc == 2 and "--select-depth <...>  [env: SELECT_DEPTH=]" in out
    assert "--select-depth <R>" in out


def test_thin_depth_with_the_selection_is_still_refused(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    for extra in ((), ("--select-depth", "2")):
        rc, out = parse(host, *ON, "--thin-depth", "2", *extra)
        assert rc == 2 and "--thin-depth" in out and "--select-by-coverage" in out and "--select-depth" in out
    rc, out = parse(host, *ON, "--thin-depth", "1", "--select-depth", "2")
    assert rc == 0


def test_depth_one_leaves_the_other_values_untouched(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    args = ON + ("--thin-mismatches", "2", "--thin-3p-exact", "5", "--thin-min-gain", "4", "--thin-tm", "31.5",
                 "--thin-thal", "end1", "--tubes", "3")
    rc, plain = parse(host, *args)
    rc1, one = parse(host, *args, "--select-depth", "1")
    rc2, two = parse(host, *args, "--select-depth", "2")
    assert rc == rc1 == rc2 == 0
    assert one == plain
    a, b = kv_of(plain), kv_of(two)
    assert b.pop("select_depth") == "2" and a.pop("select_depth") == "1" and a == b
    assert plain.count("select_depth=") == 1 and "thin_depth=1\nselect_depth=1\n" in plain
