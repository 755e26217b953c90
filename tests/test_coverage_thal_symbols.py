"""The thal-scored coverage's interface without a GPU: the header declares msspe_segment_coverage_thal and its _dev /
_packed_dev forms, the library exports them, the binding's EXPORTS lists them, msspe_scored_match is 32 bytes in the
header's layout and in the binding's, and a NULL context is an argument error."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["msspe_segment_coverage_thal", "msspe_segment_coverage_thal_dev", "msspe_segment_coverage_thal_packed_dev"]


@pytest.fixture(scope="module")
def lib():
    import msspe_amd
    return msspe_amd.load_library()


def test_library_exports_the_family(lib):
    for name in NAMES:
        assert hasattr(lib, name), name


def test_header_and_binding_list_the_family():
    from msspe_amd import capi
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    for name in NAMES:
        assert name in capi.EXPORTS, name
        assert f"int {name}(" in header, name
    for key in ("coverage_thal_matches", "coverage_thal_slabs", "coverage_thal_redone", "coverage_thal_list_us",
                "coverage_thal_score_us", "coverage_thal_fold_us"):
        assert f'"{key}"' in header, key


def test_scored_match_is_32_bytes():
    from msspe_amd import capi
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} msspe_scored_match;", header).group(1)
    fields = re.findall(r"(uint32_t|uint16_t|double)\s+([a-z_, ]+);", body)
    ctype = {"uint32_t": C.c_uint32, "uint16_t": C.c_uint16, "double": C.c_double}

    class Rec(C.Structure):
        _fields_ = [(n.strip(), ctype[t]) for t, names in fields for n in names.split(",")]

    assert [f for f, _ in Rec._fields_] == ["primer", "segment", "offset", "mismatches", "stable", "dg", "t"]
    assert C.sizeof(Rec) == 32
    assert capi.SCORED_MATCH_DTYPE.itemsize == 32
    assert list(capi.SCORED_MATCH_DTYPE.names) == [f for f, _ in Rec._fields_]
    for name, _ in Rec._fields_:
        assert capi.SCORED_MATCH_DTYPE.fields[name][1] == getattr(Rec, name).offset, name


def test_null_context_is_an_argument_error(lib):
    for name in NAMES:
        assert getattr(lib, name)(None, None, 0, 0, None, None, None, 0, None, 0, None, 1, C.c_float(30.0), None, None,
                                  None, None, None, 0, None) == 1
