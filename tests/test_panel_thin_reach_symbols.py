"""The reach-thinning calls' interface without a GPU: the library exports the two symbols, the header declares them and
states the contract, the binding lists them, a NULL context is an argument error, and the CLI names its usage errors
before it touches a device."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"
CALLS = ["msspe_panel_thin_reach_packed_dev", "msspe_panel_thin_reach"]


@pytest.fixture(scope="module")
def lib():
    import msspe_amd
    return msspe_amd.load_library()


def test_library_exports_the_calls(lib):
    for name in CALLS:
        assert hasattr(lib, name), name


def test_header_and_binding_list_the_calls():
    import msspe_amd
    from msspe_amd import capi
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    for name in CALLS:
        assert name in capi.EXPORTS, name
        assert f"int {name}(" in header, name
    assert hasattr(msspe_amd.Engine, "panel_thin_reach_packed") and hasattr(msspe_amd.Engine, "panel_thin_reach")
    flat = " ".join(header.split())
    section = flat[flat.index("a panel thinned on target reach"):flat.index("segment coverage scored with thal")]
    for words in ("[p_pos, min(p_pos + D, e_r) - 1]", "[max(q + k - D, s_r), q + k - 1]",
                  "Reach never leaves the site's record", "A word listed twice has two equal sets",
                  "ties to the LOWEST index", "reached_kept == reached_all", "thinning loses no reached column",
                  "NOT preserved", "Memory depends on the number of stable sites", "amplicon_keys_cap_log2",
                  "thin_reach_sites", "thin_reach_intervals", "thin_reach_rounds", "thin_reach_prepare_us",
                  "thin_reach_gain0_us", "thin_reach_rounds_us", "thin_reach_report_us", "min_gain < 1",
                  "n == 0 or total_len < k"):
        assert words in section, words


def test_null_context_is_an_argument_error(lib):
    from msspe_amd import Chem, MismatchOpt
    from msspe_amd.capi import REACH_RECORD_DTYPE, ReachOpt, ThinOpt
    mm, opt, thin, chem = MismatchOpt(0, 0), ReachOpt(100), ThinOpt(1), Chem.ntthal()
    words, out = (C.c_uint64 * 1)(0), (C.c_uint64 * 2)()
    keep, order, gains = (C.c_uint8 * 1)(), (C.c_uint32 * 1)(), (C.c_uint32 * 1)()
    picked, a, b = C.c_int(0), C.c_longlong(0), C.c_longlong(0)
    recs = np.zeros(1, dtype=REACH_RECORD_DTYPE)
    assert lib.msspe_panel_thin_reach_packed_dev(
        None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1, 0.0, 0, C.byref(opt), C.byref(thin), None, None, 0,
        keep, order, gains, C.byref(picked), None, C.byref(a), C.byref(b), out, out, recs.ctypes.data) == 1
    assert lib.msspe_panel_thin_reach(
        None, None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1, 0.0, 0, C.byref(opt), C.byref(thin), None,
        keep, order, gains, C.byref(picked), None, C.byref(a), C.byref(b), out, out, recs.ctypes.data, None) == 1


def test_cli_usage_errors(tmp_path):
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n>b\nACGTACGTACGTACGTACGTACGTACGT\n")
    for flags, why in ((("--thin-reach", "true"), "'--thin-reach' needs '--reach <D>'"),
                       (("--thin-reach", "true", "--reach-tm", "30"), "needs '--reach <D>'"),
                       (("--reach", "500", "--thin-reach", "true", "--thin-reach-min-gain", "0"),
                        "invalid value '0' for '--thin-reach-min-gain"),
                       (("--reach", "500", "--thin-reach", "true", "--thin-reach-min-gain", "-3"),
                        "--thin-reach-min-gain"),
                       (("--reach", "500", "--thin-reach-min-gain", "2"),
                        "'--thin-reach-min-gain' needs '--thin-reach true'"),
                       (("--reach", "500", "--thin-reach", "maybe"), "--thin-reach")):
        r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(tmp_path / "x.csv"), "--do-align", "false", *flags],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and why in r.stderr, (flags, r.stderr)
