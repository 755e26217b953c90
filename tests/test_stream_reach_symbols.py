"""The reach calls' interface without a GPU: the library exports the two symbols, the header declares them and states
the contract, the binding lists them and lays the record out as the header does (48 bytes), a NULL context is an
argument error, and the CLI names its usage errors before it touches a device."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"
CALLS = ["msspe_stream_reach_packed_dev", "msspe_stream_reach"]
FIELDS = ["sites_plus", "sites_minus", "reached_plus", "reached_minus", "reached_either", "reached_both",
          "gap_plus_len", "gap_plus_pos", "gap_minus_len", "gap_minus_pos", "gap_either_len", "gap_either_pos"]


@pytest.fixture(scope="module")
def lib():
    import msspe_amd
    return msspe_amd.load_library()


def test_library_exports_the_reach_calls(lib):
    for name in CALLS:
        assert hasattr(lib, name), name


def test_header_and_binding_list_the_reach_calls():
    import msspe_amd
    from msspe_amd import capi
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    for name in CALLS:
        assert name in capi.EXPORTS, name
        assert f"int {name}(" in header, name
    assert hasattr(msspe_amd.Engine, "stream_reach_packed") and hasattr(msspe_amd.Engine, "stream_reach")
    flat = " ".join(header.split())
    for words in ("p <= b <= p + D - 1", "q + k - D <= b <= q + k - 1", "Reach never leaves its record",
                  "ties go to the lowest position", "len = 0 gives pos = s_r", "k <= D < 2^31",
                  "every gap is the whole record", "reach_plane_bytes", "reach_grows", "reach_tile_columns"):
        assert words in flat, words


def test_the_record_is_48_bytes_and_laid_out_as_the_header():
    from msspe_amd import capi
    import stream_reach_model as srm
    assert capi.REACH_RECORD_DTYPE.itemsize == 48 == srm.REACH_RECORD_DTYPE.itemsize
    assert list(capi.REACH_RECORD_DTYPE.names) == FIELDS == list(srm.REACH_RECORD_DTYPE.names)
    assert all(capi.REACH_RECORD_DTYPE[f] == np.uint32 for f in FIELDS)
    assert C.sizeof(capi.ReachOpt) == 4
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    body = header[header.index("} msspe_reach_opt;"):header.index("} msspe_reach_record;")]
    declared = [w.strip(" ;") for line in body.splitlines() if line.strip().startswith("uint32_t")
                for w in line.strip()[len("uint32_t"):].split(",")]
    assert declared == FIELDS


def test_null_context_is_an_argument_error(lib):
    from msspe_amd import Chem, MismatchOpt
    from msspe_amd.capi import REACH_RECORD_DTYPE, ReachOpt
    mm, opt, chem = MismatchOpt(0, 0), ReachOpt(100), Chem.ntthal()
    words, out = (C.c_uint64 * 1)(0), (C.c_uint64 * 2)()
    recs = np.zeros(1, dtype=REACH_RECORD_DTYPE)
    assert lib.msspe_stream_reach_packed_dev(None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1, 0.0, 0,
                                             C.byref(opt), None, 0, out, out, recs.ctypes.data) == 1
    assert lib.msspe_stream_reach(None, None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1, 0.0, 0,
                                  C.byref(opt), out, out, recs.ctypes.data, None) == 1


def test_cli_usage_errors(tmp_path):
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n>b\nACGTACGTACGTACGTACGTACGTACGT\n")
    for flags, why in ((("--reach", "12"), "is smaller than '--kmer-size 13'"),
                       (("--reach-mismatches", "1"), "'--reach-mismatches' needs '--reach <D>'"),
                       (("--reach-3p-exact", "1"), "'--reach-3p-exact' needs '--reach <D>'"),
                       (("--reach-tm", "30"), "'--reach-tm' needs '--reach <D>'"),
                       (("--reach-thal", "end1"), "'--reach-thal' needs '--reach <D>'"),
                       (("--reach-out", str(tmp_path / "r.csv")), "'--reach-out' needs '--reach <D>'"),
                       (("--reach", "500", "--reach-thal", "end1"), "'--reach-thal' needs '--reach-tm <C>'"),
                       (("--reach", "500", "--reach-thal", "both", "--reach-tm", "30"), "--reach-thal"),
                       (("--reach", "500", "--kmer-size", "1"), "--kmer-size"),
                       (("--reach", "0"), "--reach"), (("--reach", "2147483648"), "--reach")):
        r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(tmp_path / "x.csv"), "--do-align", "false", *flags],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and why in r.stderr, (flags, r.stderr)
