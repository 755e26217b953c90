"""The thinning and selection by gain per cost's interface without a GPU: the header declares the six msspe_panel_*_cost*
calls and states the rule, the guarantees and the errors, the library exports them, the binding's EXPORTS lists them and
has the two methods, the host library exports the twins' hooks, a NULL context is an argument error, and the CLI takes
--primer-costs, --default-primer-cost and --background-site-cost, refuses the combinations it cannot serve, and leaves
the --genome-weights errors as they were."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
THIN = ["msspe_panel_thin_cost", "msspe_panel_thin_cost_dev", "msspe_panel_thin_cost_packed_dev"]
SELECT = ["msspe_panel_select_cost_dev", "msspe_panel_select_cost_packed_dev", "msspe_panel_select_cost_rule"]
ENV = ("PRIMER_COSTS", "DEFAULT_PRIMER_COST", "BACKGROUND_SITE_COST", "BACKGROUND", "GENOME_WEIGHTS",
       "DEFAULT_GENOME_WEIGHT", "SELECT_BY_COVERAGE", "SELECT_DEPTH", "THIN_PANEL", "THIN_DEPTH", "THIN_TM", "THIN_THAL",
       "THIN_MIN_GAIN", "THIN_MISMATCHES", "KMER_SIZE", "KEEP_ALL", "MSSPE_DEVICES", "TUBES", "REPICK_ROUNDS",
       "EXISTING_PRIMERS", "BACKGROUND_TM", "MAX_BACKGROUND_SITES")


@pytest.fixture(scope="module")
def lib():
    import msspe_amd
    return msspe_amd.load_library()


@pytest.fixture(scope="module")
def host(lib):
    return C.CDLL(str(HOST_LIB))


def test_libraries_export_the_cost_calls(lib, host):
    for name in THIN + SELECT:
        assert hasattr(lib, name), name
    for name in ("odm_thin_panel_cost", "odm_select_panel_cost"):
        assert hasattr(host, name), name


def test_header_and_binding_list_the_cost_calls():
    import msspe_amd
    from msspe_amd import capi
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    for name in THIN + SELECT:
        assert name in capi.EXPORTS, name
        assert f"int {name}(" in header, name
    assert hasattr(msspe_amd.Engine, "panel_thin_cost") and hasattr(msspe_amd.Engine, "panel_select_cost")
    flat = " ".join(header.replace(" *", " ").split())
    for words in ("gain(p) * cost(q) > gain(q) * cost(p) in 64-bit unsigned arithmetic",
                  "on equal products the greater gain wins, then the lowest index",
                  "A primer whose gain is below min_gain is no candidate", "gain_out holds gains, not ratios",
                  "NULL means every segment counts 1", "costs == NULL or a cost of 0 is MSSPE_ERR_ARG",
                  "names the first offending index", "With all costs equal to any constant c >= 1",
                  "covered_kept_out == covered_all_out", "The selection promises neither", "Depth 1 only"):
        assert " ".join(words.replace(" *", " ").split()) in flat, words


def test_null_context_is_an_argument_error(lib):
    from msspe_amd import Chem, ConflictRule, KmerOpt, MismatchOpt, SelectOpt, ThinOpt, seed_rule
    g = np.full((2, 600), ord("A"), dtype=np.uint8)
    w = np.array([1, 2], dtype=np.uint64)
    bits = np.zeros(2, dtype=np.uint64)
    weights, costs = np.ones(2, dtype=np.uint32), np.ones(2, dtype=np.uint32)
    keep, tube, barred = np.zeros(2, np.uint8), np.zeros(2, np.uint8), np.zeros(2, np.uint8)
    order, gains = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    n = C.c_int(-1)
    opt, mm, thin = KmerOpt(500, 250, 50, 13, 0, 0), MismatchOpt(1, 3), ThinOpt(1)
    rule, sel, chem, cr = seed_rule(1, 3), SelectOpt(1, 1, 0), Chem.ntthal(), ConflictRule.of()
    for name in THIN:
        assert getattr(lib, name)(None, g.ctypes.data, 2, 600, C.byref(opt), C.byref(mm), C.byref(thin), w.ctypes.data, 1,
                                  w[1:].ctypes.data, 1, None, weights.ctypes.data, costs.ctypes.data, keep.ctypes.data,
                                  order.ctypes.data, gains.ctypes.data, C.byref(n), None, None, None, None, None, None,
                                  None) == 1, name
    head = (None, g.ctypes.data, 2, 600, C.byref(opt), C.byref(rule), C.byref(sel), w.ctypes.data, 1, w[1:].ctypes.data,
            1, None)
    tail = (weights.ctypes.data, costs.ctypes.data, keep.ctypes.data, order.ctypes.data, gains.ctypes.data, C.byref(n),
            tube.ctypes.data, barred.ctypes.data, None, None, None, None, None, None, None, None)
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
    assert rc == 0 and (kv["primer_costs"], kv["default_primer_cost"], kv["background_site_cost"]) == ("", "1", "0")
    for switch in (("--thin-panel", "true"), ("--select-by-coverage", "true"),
                   ("--select-by-coverage", "true", "--thin-tm", "30"),
                   ("--select-by-coverage", "true", "--thin-tm", "30", "--thin-thal", "end1"),
                   ("--select-by-coverage", "true", "--repick-rounds", "2"),
                   ("--select-by-coverage", "true", "--existing-primers", "p.csv"),
                   ("--select-by-coverage", "true", "--tubes", "2"),
                   ("--thin-panel", "true", "--genome-weights", "w.csv")):
        rc, out = parse(host, *base, *switch, "--primer-costs", "c.csv", "--default-primer-cost=4294967295",
                        "--background", "bg.fa", "--background-site-cost", "5")
        kv = dict(l.split("=", 1) for l in out.splitlines())
        assert rc == 0, (switch, out)
        assert (kv["primer_costs"], kv["default_primer_cost"], kv["background_site_cost"]) == ("c.csv", "4294967295", "5")
    rc, out = parse(host, *base, "--thin-panel", "true", "--background=bg.fa", "--background-site-cost=2")
    assert rc == 0 and "background_site_cost=2" in out and "primer_costs=\n" in out   # either option alone
    monkeypatch.setenv("PRIMER_COSTS", "env.csv")
    monkeypatch.setenv("BACKGROUND_SITE_COST", "9")
    monkeypatch.setenv("DEFAULT_PRIMER_COST", "6")
    rc, out = parse(host, *base, "--thin-panel", "true", "--background", "bg.fa")
    assert rc == 0 and "primer_costs=env.csv" in out and "background_site_cost=9" in out and "default_primer_cost=6" in out
    for v in ("PRIMER_COSTS", "BACKGROUND_SITE_COST", "DEFAULT_PRIMER_COST"):
        monkeypatch.delenv(v)
    for flag in ("--default-primer-cost", "--background-site-cost"):
        for bad in ("0", "-1", "4294967296", "x", "1.5"):
            rc, out = parse(host, *base, "--thin-panel", "true", "--background", "bg.fa", "--primer-costs", "c.csv",
                            flag, bad)
            assert rc == 2 and flag in out and "4294967295" in out, (flag, bad, out)
    rc, out = parse(host, "--help")
    assert rc == 2
    for line in ("--primer-costs <...>  [env: PRIMER_COSTS=]", "--default-primer-cost <...>  [env: DEFAULT_PRIMER_COST=]",
                 "--background-site-cost <...>  [env: BACKGROUND_SITE_COST=]", "coverage per cost"):
        assert line in out, line


def test_combinations_that_are_usage_errors(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    plain = ("-i", "a.fa", "-o", "b.csv")
    for cost in (("--primer-costs", "c.csv"), ("--background", "bg.fa", "--background-site-cost", "3")):
        base = plain + cost
        rc, out = parse(host, *base)                     # neither switch
        assert rc == 2 and "--primer-costs" in out and "--background-site-cost" in out and "nothing without" in out
        assert "--thin-panel true" in out and "--select-by-coverage true" in out
        for extra, named, why in ((("--thin-panel", "true", "--thin-depth", "2"), "--thin-depth", "depth 1"),
                                  (("--select-by-coverage", "true", "--select-depth", "2"), "--select-depth", "depth 1"),
                                  (("--thin-panel", "true", "--thin-tm", "30"), "--thin-tm", "no cost form")):
            rc, out = parse(host, *base, *extra)
            assert rc == 2 and "--primer-costs" in out and "--background-site-cost" in out, (extra, out)
            assert named in out and why in out and "not built yet" in out, (extra, out)
            rc, out = parse(host, *plain, *extra)        # without the costs they stand
            assert rc == 0, extra
        rc, out = parse(host, *base, "--devices", "0,1")
        assert rc == 2 and "--primer-costs" in out and "--background-site-cost" in out and "--devices" in out, out
    rc, out = parse(host, *plain, "--thin-panel", "true", "--background-site-cost", "3")
    assert rc == 2 and out.strip() == "error: '--background-site-cost' needs '--background <FASTA>'"
    rc, out = parse(host, *plain, "--thin-panel", "true", "--default-primer-cost", "3")   # a default alone prices nothing
    assert rc == 0


def test_the_genome_weights_errors_are_unchanged(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    base = ("-i", "a.fa", "-o", "b.csv", "--genome-weights", "w.csv")
    texts = {
        ("--thin-panel", "true", "--thin-depth", "2"):
            "error: '--genome-weights' with '--thin-depth' above 1 is not built yet: weights run at depth 1",
        ("--select-by-coverage", "true", "--select-depth", "2"):
            "error: '--genome-weights' with '--select-depth' above 1 is not built yet: weights run at depth 1",
        ("--thin-panel", "true", "--thin-tm", "30"):
            "error: '--genome-weights' with '--thin-panel true --thin-tm' is not built yet: the weighted thinning runs "
            "on the string rule"}
    for extra, text in texts.items():
        for cost in ((), ("--primer-costs", "c.csv")):   # with a cost option too they come first, as they are
            rc, out = parse(host, *base, *extra, *cost)
            assert rc == 2 and out.strip() == text, (extra, cost, out)
