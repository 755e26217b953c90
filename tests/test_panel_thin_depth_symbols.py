"""The depth thinning's interface without a GPU: the header declares the six msspe_panel_thin_depth* /
msspe_panel_thin_thal_depth* calls, the library exports them, the binding's EXPORTS lists them, a NULL context is an
argument error, and the CLI takes --thin-depth (env THIN_DEPTH, default 1, 1..255, read only with --thin-panel true,
not above 1 with --select-by-coverage true)."""
import ctypes as C
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
MM = ["msspe_panel_thin_depth", "msspe_panel_thin_depth_dev", "msspe_panel_thin_depth_packed_dev"]
THAL = ["msspe_panel_thin_thal_depth", "msspe_panel_thin_thal_depth_dev", "msspe_panel_thin_thal_depth_packed_dev"]
ENV = ("THIN_PANEL", "THIN_MISMATCHES", "THIN_3P_EXACT", "THIN_MIN_GAIN", "THIN_DEPTH", "THIN_TM", "THIN_THAL",
       "SELECT_BY_COVERAGE", "KMER_SIZE", "KEEP_ALL", "MSSPE_DEVICES")


@pytest.fixture(scope="module")
def lib():
    import msspe_amd
    return msspe_amd.load_library()


@pytest.fixture(scope="module")
def host(lib):
    return C.CDLL(str(HOST_LIB))


def test_library_exports_the_depth_thinning(lib, host):
    for name in MM + THAL:
        assert hasattr(lib, name), name
    assert hasattr(host, "odm_thin_panel_depth") and hasattr(host, "odm_thin_shadows")


def test_header_and_binding_list_the_depth_thinning():
    import msspe_amd
    from msspe_amd import capi
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    for name in MM + THAL:
        assert name in capi.EXPORTS, name
        assert f"int {name}(" in header, name
    assert "} msspe_thin_depth_opt;" in header
    for key in ("panel_thin_depth_shadows", "panel_thin_depth_colsum_us"):
        assert f'"{key}"' in header, key
    assert "depth_kept[s] >= min(R, depth_all[s])" in header   # the guarantee at min_gain 1
    opt = msspe_amd.ThinDepthOpt(3, 2)
    assert (opt.min_gain, opt.depth) == (3, 2) and C.sizeof(opt) == 8


def test_null_context_is_an_argument_error(lib):
    import numpy as np
    from msspe_amd import Chem, KmerOpt, MismatchOpt, ThinDepthOpt
    g = np.full((2, 600), ord("A"), dtype=np.uint8)
    w = np.zeros(1, dtype=np.uint64)
    keep, order, gains = np.zeros(2, np.uint8), np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    n = C.c_int(-1)
    opt, mm, thin, chem = KmerOpt(500, 250, 50, 13, 0, 0), MismatchOpt(1, 3), ThinDepthOpt(1, 2), Chem.ntthal()
    tail = (w.ctypes.data, 1, w.ctypes.data, 1, None, keep.ctypes.data, order.ctypes.data, gains.ctypes.data,
            C.byref(n), None, None, None)
    for name in MM:
        assert getattr(lib, name)(None, g.ctypes.data, 2, 600, C.byref(opt), C.byref(mm), C.byref(thin), *tail) == 1, name
    for name in THAL:
        assert getattr(lib, name)(None, g.ctypes.data, 2, 600, C.byref(opt), C.byref(mm), C.byref(thin),
                                  C.byref(chem), 2, 30.0, *tail) == 1, name


def parse(host, *a):
    argv = (C.c_char_p * (len(a) + 1))(b"od-msspe-hip", *[x.encode() for x in a])
    buf = C.create_string_buffer(1 << 16)
    rc = host.odm_parse_args(len(a) + 1, argv, buf, 1 << 16)
    return rc, buf.value.decode()


def kv_of(out):
    return dict(l.split("=", 1) for l in out.splitlines())


def test_cli_flag(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv")
    assert rc == 0 and kv_of(out)["thin_depth"] == "1"
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--thin-panel", "true", "--thin-depth", "3")
    assert rc == 0 and kv_of(out)["thin_depth"] == "3" and kv_of(out)["thin_panel"] == "true"
    for ok in ("1", "255"):
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--thin-panel", "true", f"--thin-depth={ok}")
        assert rc == 0 and kv_of(out)["thin_depth"] == ok
    for bad in ("0", "256", "-1"):
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--thin-panel", "true", "--thin-depth", bad)
        assert rc == 2 and "--thin-depth" in out, (bad, out)
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--thin-depth", "two")
    assert rc == 2 and "--thin-depth" in out
    # without the switch the value is not read beyond its form
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--thin-depth", "999")
    assert rc == 0 and kv_of(out)["thin_panel"] == "false"
    # the selection has no depth: above 1 is refused, 1 is today's run
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--select-by-coverage", "true", "--thin-depth", "2")
    assert rc == 2 and "--thin-depth" in out and "--select-by-coverage" in out
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--select-by-coverage", "true", "--thin-depth", "1")
    assert rc == 0
    monkeypatch.setenv("THIN_PANEL", "true")
    monkeypatch.setenv("THIN_DEPTH", "4")
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv")
    assert rc == 0 and kv_of(out)["thin_depth"] == "4"
    monkeypatch.setenv("THIN_DEPTH", "300")
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv")
    assert rc == 2 and "--thin-depth" in out
    rc, out = parse(host, "--help")
    assert rc == 2 and "--thin-depth <...>  [env: THIN_DEPTH=]" in out
    assert "--thin-depth <R>" in out


def test_depth_one_leaves_the_other_values_untouched(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    args = ("-i", "a.fa", "-o", "b.csv", "--thin-panel", "true", "--thin-mismatches", "2", "--thin-3p-exact", "5",
            "--thin-min-gain", "4", "--thin-tm", "31.5", "--thin-thal", "end1", "--tubes", "3")
    rc, plain = parse(host, *args)
    rc1, one = parse(host, *args, "--thin-depth", "1")
    rc2, two = parse(host, *args, "--thin-depth", "2")
    assert rc == rc1 == rc2 == 0
    assert one == plain
    a, b = kv_of(plain), kv_of(two)
    assert b.pop("thin_depth") == "2" and a.pop("thin_depth") == "1" and a == b
