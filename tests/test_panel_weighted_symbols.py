"""The weighted thinning and selection's interface without a GPU: the header declares the six msspe_panel_*_weighted*
calls and states the rule and both guarantees, the library exports them, the binding's EXPORTS lists them, the host
library exports the twins' hooks, a NULL context is an argument error, and the CLI takes --genome-weights and
--default-genome-weight and refuses the combinations it cannot serve."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
THIN = ["msspe_panel_thin_weighted", "msspe_panel_thin_weighted_dev", "msspe_panel_thin_weighted_packed_dev"]
SELECT = ["msspe_panel_select_weighted_dev", "msspe_panel_select_weighted_packed_dev", "msspe_panel_select_weighted_rule"]
ENV = ("GENOME_WEIGHTS", "DEFAULT_GENOME_WEIGHT", "SELECT_BY_COVERAGE", "SELECT_DEPTH", "THIN_PANEL", "THIN_DEPTH",
       "THIN_TM", "THIN_THAL", "THIN_MIN_GAIN", "THIN_MISMATCHES", "KMER_SIZE", "KEEP_ALL", "MSSPE_DEVICES", "TUBES",
       "REPICK_ROUNDS")


@pytest.fixture(scope="module")
def lib():
    import msspe_amd
    return msspe_amd.load_library()


@pytest.fixture(scope="module")
def host(lib):
    return C.CDLL(str(HOST_LIB))


def test_libraries_export_the_weighted_calls(lib, host):
    for name in THIN + SELECT:
        assert hasattr(lib, name), name
    for name in ("odm_thin_panel_weighted", "odm_select_panel_weighted"):
        assert hasattr(host, name), name


def test_header_and_binding_list_the_weighted_calls():
    import msspe_amd
    from msspe_amd import capi
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    for name in THIN + SELECT:
        assert name in capi.EXPORTS, name
        assert f"int {name}(" in header, name
    assert hasattr(msspe_amd.Engine, "panel_thin_weighted") and hasattr(msspe_amd.Engine, "panel_select_weighted")
    flat = " ".join(header.replace(" *", " ").split())
    for words in ("gain(p) = the SUM of weights[s]", "ties to the lowest index", "which is in WEIGHT UNITS here",
                  "A segment of weight 0 never contributes", "must be <= 2^32 - 1", "weights == NULL is MSSPE_ERR_ARG",
                  "With all weights 1 every output equals the unweighted call's", "weight_kept_out == weight_all_out",
                  "The selection does not promise this"):
        assert words in flat, words


def test_null_context_is_an_argument_error(lib):
    from msspe_amd import Chem, ConflictRule, KmerOpt, MismatchOpt, SelectOpt, ThinOpt, seed_rule
    g = np.full((2, 600), ord("A"), dtype=np.uint8)
    w = np.array([1, 2], dtype=np.uint64)
    bits = np.zeros(2, dtype=np.uint64)
    weights = np.ones(2, dtype=np.uint32)
    keep, tube, barred = np.zeros(2, np.uint8), np.zeros(2, np.uint8), np.zeros(2, np.uint8)
    order, gains = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    n = C.c_int(-1)
    opt, mm, thin = KmerOpt(500, 250, 50, 13, 0, 0), MismatchOpt(1, 3), ThinOpt(1)
    rule, sel, chem, cr = seed_rule(1, 3), SelectOpt(1, 1, 0), Chem.ntthal(), ConflictRule.of()
    for name in THIN:
        assert getattr(lib, name)(None, g.ctypes.data, 2, 600, C.byref(opt), C.byref(mm), C.byref(thin), w.ctypes.data, 1,
                                  w[1:].ctypes.data, 1, None, weights.ctypes.data, keep.ctypes.data, order.ctypes.data,
                                  gains.ctypes.data, C.byref(n), None, None, None, None, None) == 1, name
    head = (None, g.ctypes.data, 2, 600, C.byref(opt), C.byref(rule), C.byref(sel), w.ctypes.data, 1, w[1:].ctypes.data,
            1, None)
    tail = (weights.ctypes.data, keep.ctypes.data, order.ctypes.data, gains.ctypes.data, C.byref(n), tube.ctypes.data,
            barred.ctypes.data, None, None, None, None, None, None)
    for name in SELECT:
        graph = (C.byref(chem), C.byref(cr)) if name.endswith("_rule") else (bits.ctypes.data,)
        assert getattr(lib, name)(*head, *graph, *tail) == 1, name


def parse(host, *a):
    argv = (C.c_char_p * (len(a) + 1))(b"od-msspe-hip", *[x.encode() for x in a])
    buf = C.create_string_buffer(1 << 16)
    rc = host.odm_parse_args(len(a) + 1, argv, buf, 1 << 16)
    return rc, buf.value.decode()


def test_cli_flags(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    base = ("-i", "a.fa", "-o", "b.csv")
    rc, out = parse(host, *base)
    kv = dict(l.split("=", 1) for l in out.splitlines())
    assert rc == 0 and (kv["genome_weights"], kv["default_genome_weight"]) == ("", "1")
    for switch in (("--thin-panel", "true"), ("--select-by-coverage", "true"),
                   ("--select-by-coverage", "true", "--thin-tm", "30"),
                   ("--select-by-coverage", "true", "--repick-rounds", "2"),
                   ("--select-by-coverage", "true", "--tubes", "2")):
        rc, out = parse(host, *base, *switch, "--genome-weights", "w.csv", "--default-genome-weight=3")
        kv = dict(l.split("=", 1) for l in out.splitlines())
        assert rc == 0 and (kv["genome_weights"], kv["default_genome_weight"]) == ("w.csv", "3"), (switch, out)
    monkeypatch.setenv("GENOME_WEIGHTS", "env.csv")
    rc, out = parse(host, *base, "--thin-panel", "true")
    assert rc == 0 and "genome_weights=env.csv" in out
    monkeypatch.delenv("GENOME_WEIGHTS")
    rc, out = parse(host, *base, "--thin-panel", "true", "--default-genome-weight", "-1")
    assert rc == 2 and "--default-genome-weight" in out
    rc, out = parse(host, "--help")
    assert rc == 2 and "--genome-weights <...>  [env: GENOME_WEIGHTS=]" in out
    assert "--default-genome-weight <...>  [env: DEFAULT_GENOME_WEIGHT=]" in out and "weight units" in out


def test_combinations_that_are_usage_errors(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    base = ("-i", "a.fa", "-o", "b.csv", "--genome-weights", "w.csv")
    rc, out = parse(host, *base)
    assert rc == 2 and "--genome-weights" in out and "does nothing" in out
    for extra, named in ((("--thin-panel", "true", "--thin-depth", "2"), "--thin-depth"),
                         (("--select-by-coverage", "true", "--select-depth", "2"), "--select-depth"),
                         (("--thin-panel", "true", "--thin-tm", "30"), "--thin-tm")):
        rc, out = parse(host, *base, *extra)
        assert rc == 2 and "--genome-weights" in out and named in out and "not built yet" in out, (extra, out)
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", *extra)       # without the weights they stand
        assert rc == 0, extra
