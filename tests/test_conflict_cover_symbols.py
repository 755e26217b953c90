"""The device vertex cover's interface without a GPU: the library exports msspe_conflict_cover / _dev, the binding's
EXPORTS lists them, a NULL context is an argument error, and the CLI takes --cover-on-device (env COVER_ON_DEVICE,
default false)."""
import ctypes as C
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
NAMES = ["msspe_conflict_cover", "msspe_conflict_cover_dev"]


@pytest.fixture(scope="module")
def lib():
    import msspe_amd
    return msspe_amd.load_library()


@pytest.fixture(scope="module")
def host(lib):
    return C.CDLL(str(HOST_LIB))


def test_library_exports_the_cover(lib):
    for name in NAMES:
        assert hasattr(lib, name), name


def test_binding_lists_the_cover():
    from msspe_amd import capi
    for name in NAMES:
        assert name in capi.EXPORTS, name
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    assert '"cover_rounds"' in header


def test_null_context_is_an_argument_error(lib):
    from msspe_amd import Chem
    deleted = (C.c_uint8 * 2)()
    nd = C.c_int(-1)
    assert lib.msspe_conflict_cover(None, b"ACGTACGTACGTAACGTACGTACGTA", 2, 13, C.byref(Chem.ntthal()),
                                    C.c_float(-9000.0), 0, deleted, C.byref(nd)) == 1
    assert lib.msspe_conflict_cover_dev(None, None, 0, 13, None, 0, None, C.byref(nd)) == 1


def parse(host, *a):
    argv = (C.c_char_p * (len(a) + 1))(b"od-msspe-hip", *[x.encode() for x in a])
    buf = C.create_string_buffer(1 << 16)
    rc = host.odm_parse_args(len(a) + 1, argv, buf, 1 << 16)
    return rc, buf.value.decode()


def test_cli_flag(host, monkeypatch):
    monkeypatch.delenv("COVER_ON_DEVICE", raising=False)
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv")
    assert rc == 0 and dict(l.split("=", 1) for l in out.splitlines())["cover_on_device"] == "false"
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--cover-on-device", "true")
    assert rc == 0 and dict(l.split("=", 1) for l in out.splitlines())["cover_on_device"] == "true"
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--cover-on-device", "yes")
    assert rc == 2 and "possible values: true, false" in out
    monkeypatch.setenv("COVER_ON_DEVICE", "true")
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv")
    assert dict(l.split("=", 1) for l in out.splitlines())["cover_on_device"] == "true"
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--cover-on-device=false")
    assert dict(l.split("=", 1) for l in out.splitlines())["cover_on_device"] == "false"
