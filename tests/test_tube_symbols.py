"""The tube split's interface without a GPU: the header declares msspe_conflict_tubes / _dev, the library exports them,
the binding's EXPORTS lists them, a NULL context is an argument error, and the CLI takes --tubes (env TUBES, 0..64,
default 0)."""
import ctypes as C
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
NAMES = ["msspe_conflict_tubes", "msspe_conflict_tubes_dev"]


@pytest.fixture(scope="module")
def lib():
    import msspe_amd
    return msspe_amd.load_library()


@pytest.fixture(scope="module")
def host(lib):
    return C.CDLL(str(HOST_LIB))


def test_library_exports_the_tube_split(lib):
    for name in NAMES:
        assert hasattr(lib, name), name


def test_header_and_binding_list_the_tube_split():
    from msspe_amd import capi
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    for name in NAMES:
        assert name in capi.EXPORTS, name
        assert f"int {name}(" in header, name
    assert "#define MSSPE_TUBE_NONE 255" in header
    for key in ("tube_rounds", "tube_keys_us", "tube_symmetrise_us", "tube_rounds_us"):
        assert f'"{key}"' in header, key


def test_null_context_is_an_argument_error(lib):
    from msspe_amd import Chem
    tube = (C.c_uint8 * 2)()
    used, unplaced = C.c_int(-1), C.c_int(-1)
    assert lib.msspe_conflict_tubes(None, b"ACGTACGTACGTAACGTACGTACGTA", 2, 13, C.byref(Chem.ntthal()),
                                    C.c_float(-9000.0), 0, 4, tube, C.byref(used), C.byref(unplaced)) == 1
    assert lib.msspe_conflict_tubes_dev(None, None, 0, 13, None, 0, 4, None, C.byref(used), C.byref(unplaced)) == 1


def parse(host, *a):
    argv = (C.c_char_p * (len(a) + 1))(b"od-msspe-hip", *[x.encode() for x in a])
    buf = C.create_string_buffer(1 << 16)
    rc = host.odm_parse_args(len(a) + 1, argv, buf, 1 << 16)
    return rc, buf.value.decode()


def tubes_of(out):
    return dict(l.split("=", 1) for l in out.splitlines())["tubes"]


def test_cli_flag(host, monkeypatch):
    monkeypatch.delenv("TUBES", raising=False)
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv")
    assert rc == 0 and tubes_of(out) == "0"
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--tubes", "4")
    assert rc == 0 and tubes_of(out) == "4"
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--tubes=0")
    assert rc == 0 and tubes_of(out) == "0"
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--tubes", "64")
    assert rc == 0 and tubes_of(out) == "64"
    for bad in ("65", "-1", "x"):
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--tubes", bad)
        assert rc == 2 and "--tubes" in out, bad
    monkeypatch.setenv("TUBES", "5")
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv")
    assert rc == 0 and tubes_of(out) == "5"
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--tubes", "2")
    assert rc == 0 and tubes_of(out) == "2"


def test_flag_combinations_are_usage_errors(host, monkeypatch):
    monkeypatch.delenv("TUBES", raising=False)
    for extra in (("--devices", "0,0"), ("--cover-on-device", "true"), ("--existing-primers", "panel.csv")):
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--tubes", "3", *extra)
        assert rc == 2 and extra[0] in out, extra
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--tubes", "0", *extra)
        assert rc == 0, extra
