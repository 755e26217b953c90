"""The thal-scored panel thinning's interface without a GPU: the header declares msspe_panel_thin_thal / _dev /
_packed_dev with their sibling's arguments and chem, mode, tm_threshold behind thin, the library exports them, the
binding lists them and has Engine.panel_thin_thal, a NULL context is an argument error, and the host layer has the
block's hook."""
import ctypes as C
import inspect
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
NAMES = ["msspe_panel_thin_thal", "msspe_panel_thin_thal_dev", "msspe_panel_thin_thal_packed_dev"]
INFO = ["matches", "unique_pairs", "slabs", "redone", "list_us", "unique_us", "score_us", "fold_us", "rounds_us"]


@pytest.fixture(scope="module")
def lib():
    import msspe_amd
    return msspe_amd.load_library()


def test_library_and_host_layer_export_the_call(lib):
    for name in NAMES:
        assert hasattr(lib, name), name
    host = C.CDLL(str(HOST_LIB))
    assert hasattr(host, "odm_thin_thal_block") and hasattr(host, "odm_thin_panel")


def declared_args(header, name):
    decl = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
    return [" ".join(a.split()) for a in decl.split(",")]


def test_header_declares_the_siblings_arguments_with_the_scoring_behind_thin():
    from msspe_amd import capi
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    for name in NAMES:
        assert name in capi.EXPORTS, name
        args = declared_args(header, name)
        sibling = declared_args(header, name.replace("_thal", ""))
        assert len(sibling) == 19 and len(args) == 22, name
        assert args[:7] == sibling[:7] and args[10:] == sibling[7:], name
        assert args[7:10] == ["const msspe_chem *chem", "int mode", "float tm_threshold"], name
        assert len(getattr(capi.load_library(), name).argtypes) == 22, name
    for key in INFO:
        assert f'"panel_thin_thal_{key}"' in header, key
    assert '"thin_thal_unique"' in header and "does NOT preserve" in header and "t_best per segment" in header


def test_binding_has_the_method_beside_panel_thin():
    from msspe_amd import Engine
    sig = inspect.signature(Engine.panel_thin_thal)
    base = inspect.signature(Engine.panel_thin)
    names = list(sig.parameters)
    assert names[:7] == list(base.parameters)[:7] and names[7:10] == ["chem", "mode", "tm_threshold"]
    assert names[10:] == list(base.parameters)[7:]


def test_null_context_is_an_argument_error(lib):
    import numpy as np
    from msspe_amd import Chem, KmerOpt, MismatchOpt, ThinOpt
    g = np.full((2, 600), ord("A"), dtype=np.uint8)
    w = np.zeros(1, dtype=np.uint64)
    keep, order, gains = np.zeros(2, np.uint8), np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    n = C.c_int(-1)
    opt, mm, thin, chem = KmerOpt(500, 250, 50, 13, 0, 0), MismatchOpt(1, 3), ThinOpt(1), Chem.ntthal()
    for name in NAMES:
        assert getattr(lib, name)(None, g.ctypes.data, 2, 600, C.byref(opt), C.byref(mm), C.byref(thin),
                                  C.byref(chem), 1, 30.0, w.ctypes.data, 1, w.ctypes.data, 1, None, keep.ctypes.data,
                                  order.ctypes.data, gains.ctypes.data, C.byref(n), None, None, None) == 1, name
