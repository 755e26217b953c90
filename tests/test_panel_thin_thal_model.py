"""The model of msspe_panel_thin_thal* (tests/panel_thin_thal_model.py: the scored matches of coverage_thal_model, the
greedy loop of panel_thin_model) against the host layer's sequential rule (odm_thin_panel over the held rows), the
block's host text (odm_thin_thal_block), the CLI's --thin-tm / --thin-thal through the parse hook, hand-built
one-segment cases and the grid's pinned picks -- every comparison on integers, exactly.  No GPU needed."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import coverage_thal_model as ctm
import panel_thin_model as tm
import panel_thin_thal_model as ttm
from test_coverage_mm_model import draw_primers, one_segment, parse, rc
from test_panel_thin_model import host_thin

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
P_FWD = "ACGTTGCAGGATC"
TAIL = "GATTACAGGCTCA"
ENV = ("THIN_PANEL", "THIN_MISMATCHES", "THIN_3P_EXACT", "THIN_MIN_GAIN", "THIN_TM", "THIN_THAL", "KMER_SIZE",
       "KEEP_ALL", "MSSPE_DEVICES", "COVERAGE_TM")
# chemistry, threshold -> segments held by the whole set, picks, (order, gains) where pinned
GRID = {("ntthal", 30.0): (69, 10, [25, 105, 115, 4, 20, 89, 109, 19, 121, 98], [10, 10, 10, 9, 8, 8, 7, 4, 2, 1]),
        ("ntthal", 40.0): (44, 7, [105, 115, 4, 25, 89, 20, 98], [10, 10, 9, 9, 4, 1, 1]),
        ("primer3", 30.0): (62, 8, None, None),
        ("primer3", 40.0): (40, 6, None, None)}
STRING_RULE_ORDER = [19, 25, 105, 115, 121, 4, 89, 109, 45, 98]


@pytest.fixture(scope="module")
def host():
    import msspe_amd
    msspe_amd.load_library()
    return C.CDLL(str(LIB))


def grid_input():
    """The alignment and the 65 + 65 primers of test_gpu_coverage_thal.py::grid_input."""
    import msspe_amd
    g = msspe_amd.synth.aligned_genomes(10, 2600, seed=53)
    rng = np.random.default_rng(1302)
    fwd = draw_primers(rng, g, 60, 13)
    rev = [rc(w) for w in draw_primers(rng, g, 60, 13)]
    return g, fwd, rev


def same(host, H, min_gain=1, forced=None):
    """The host's sequential rule over the rows of H equals the model's loop; returns the model's result."""
    want = tm.greedy(H, min_gain, forced)
    keep, order, gains, covered, c_all, c_kept, rounds = want
    h_keep, h_order, h_gains, h_all, h_kept = host_thin(host, H, min_gain, forced)
    np.testing.assert_array_equal(h_order, order)
    np.testing.assert_array_equal(h_gains, gains)
    np.testing.assert_array_equal(h_keep, keep)
    assert (h_all, h_kept) == (c_all, c_kept)
    if min_gain == 1:
        assert c_all == c_kept
    return want


@pytest.fixture(scope="module")
def grid_results(oracle, oracle_tables):
    g, fwd, rev = grid_input()
    assert (len(fwd), len(rev)) == (65, 65)
    args = {"ntthal": oracle.ntthal_args(), "primer3": oracle.p3_args()}
    out = {}
    for chem in ("ntthal", "primer3"):
        for mode in ("any", "end1"):
            base = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, 13, fwd, rev, 2, 3, mode, 30.0, args[chem])
            for thr in (30.0, 40.0):
                out[chem, mode, thr] = ctm.rethreshold(base, thr)
    return g, fwd, rev, out


@pytest.mark.parametrize("chem,thr", sorted(GRID))
def test_grid_picks_are_pinned(host, grid_results, chem, thr):
    g, fwd, rev, results = grid_results
    held, picks, order, gains = GRID[chem, thr]
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    string_rule = tm.greedy(I)
    assert string_rule[1].tolist() == STRING_RULE_ORDER
    per_mode = []
    for mode in ("any", "end1"):
        res = results[chem, mode, thr]
        assert res["count"] == 130 and ttm.distinct_pairs(res) == 36
        H = ttm.held_incidence(res)
        np.testing.assert_array_equal(H.sum(axis=1), res["primer_held"])
        np.testing.assert_array_equal(H.any(axis=0), res["held"].reshape(-1) == 2)
        assert not (H & ~I).any()                       # a held cell is a matched cell
        keep, got_order, got_gains, covered, c_all, c_kept, rounds = same(host, H)
        assert c_all == c_kept == held and len(got_order) == picks and rounds == picks + 1
        if order is not None:
            assert got_order.tolist() == order and got_gains.tolist() == gains
        # the guarantee at min_gain 1: the kept rows hold what all rows hold
        np.testing.assert_array_equal(H[keep != 0].any(axis=0), res["held"].reshape(-1) == 2)
        np.testing.assert_array_equal(covered, res["held"].reshape(-1) == 2)
        # tied top gains occur, so the lowest-index rule decides picks here
        live = np.ones(len(H), dtype=bool)
        cov = np.zeros(H.shape[1], dtype=bool)
        tied = 0
        for p in got_order:
            gain = np.where(live, (H & ~cov).sum(axis=1), -1)
            tied += int((gain == gain.max()).sum() > 1)
            assert int(np.argmax(gain)) == p
            live[p] = False
            cov |= H[p]
        assert tied >= 2
        # thinning on I instead of H is another answer
        assert got_order.tolist() != STRING_RULE_ORDER[:len(got_order)]
        assert set(got_order.tolist()) != set(STRING_RULE_ORDER)
        for G in (2, 5):
            same(host, H, G)
        forced = np.zeros(len(H), dtype=np.uint8)
        forced[got_order[:2]] = 1
        forced[int(np.flatnonzero(H.sum(axis=1) == 0)[0])] = 1      # a primer that holds nothing, forced
        same(host, H, 1, forced)
        per_mode.append((got_order.tolist(), got_gains.tolist(), keep.tolist()))
    assert per_mode[0] == per_mode[1]                   # ANY and END1 agree on this input


@pytest.fixture(scope="module")
def run(oracle, oracle_tables):
    def go(seg, fwd, rev, M, E, thr=30.0, mode="any", W=13, k=13):
        L = seg.shape[1]
        return ctm.coverage_thal(oracle_tables, seg, L, L, W, k, fwd, rev, M, E, mode, thr, oracle.ntthal_args())
    return go


def test_a_stable_and_an_unstable_match_in_one_segment(host, run):
    seg = one_segment(P_FWD, TAIL)
    weak = "TG" + P_FWD[2:]
    base = run(seg, [weak, P_FWD], [], 2, 3)
    t = {int(m["primer"]): float(m["t"]) for m in base["matches"]}
    assert t[0] < t[1]
    res = ctm.rethreshold(base, (t[0] + t[1]) / 2)
    H = ttm.held_incidence(res)
    assert H.tolist() == [[False], [True]]
    keep, order, gains, covered, c_all, c_kept, _ = same(host, H)
    # the string rule would keep primer 0 (the lowest index of two equal rows); the held rule keeps the one that holds
    I = tm.incidence(seg, seg.shape[1], seg.shape[1], 13, 13, [weak, P_FWD], [], 2, 3)
    assert I.tolist() == [[True], [True]] and tm.greedy(I)[1].tolist() == [0]
    assert order.tolist() == [1] and gains.tolist() == [1] and keep.tolist() == [0, 1] and (c_all, c_kept) == (1, 1)


def test_a_primer_with_only_unstable_matches_is_never_picked(host, run):
    seg = one_segment(P_FWD, TAIL)
    weak = "TG" + P_FWD[2:]
    base = run(seg, [weak], [rc(TAIL)], 2, 3)
    t = {int(m["primer"]): float(m["t"]) for m in base["matches"]}
    res = ctm.rethreshold(base, (t[0] + t[1]) / 2)
    assert t[0] < t[1] and res["held"].tolist() == [[2]]
    H = ttm.held_incidence(res)
    keep, order, gains, covered, c_all, c_kept, _ = same(host, H)
    assert H[0].sum() == 0 and order.tolist() == [1] and keep.tolist() == [0, 1]
    above = ttm.held_incidence(ctm.rethreshold(base, t[1] + 5.0))     # nothing stable: nothing picked, nothing held
    keep, order, gains, covered, c_all, c_kept, _ = same(host, above)
    assert order.size == 0 and not keep.any() and (c_all, c_kept) == (0, 0)
    keep, order, _, _, c_all, c_kept, _ = same(host, above, 1, [1, 0])  # forced all the same, and it holds nothing
    assert keep.tolist() == [1, 0] and order.size == 0 and (c_all, c_kept) == (0, 0)


@pytest.mark.parametrize("thr", [0.0, -5.0])
def test_a_threshold_of_zero_or_less_gives_the_string_rules_incidence(host, grid_results, thr):
    g, fwd, rev, results = grid_results
    H = ttm.held_incidence(ctm.rethreshold(results["ntthal", "any", 30.0], thr))
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    np.testing.assert_array_equal(H, I)
    assert same(host, H)[1].tolist() == STRING_RULE_ORDER


def kv(out):
    return dict(l.split("=", 1) for l in out.splitlines())


def test_cli_flags(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    got = kv(parse(host, "-i", "a", "-o", "b")[1])
    assert got["thin_tm"] == "" and got["thin_thal"] == ""
    rc_, out = parse(host, "-i", "a", "-o", "b", "--thin-panel", "true", "--thin-tm", "30")
    assert rc_ == 0 and kv(out)["thin_tm"] == "30" and kv(out)["thin_thal"] == "any"
    rc_, out = parse(host, "-i", "a", "-o", "b", "--thin-panel", "true", "--thin-tm", "-2.5", "--thin-thal", "end1",
                     "--thin-mismatches", "2")
    assert rc_ == 0 and kv(out)["thin_tm"] == "-2.5" and kv(out)["thin_thal"] == "end1"
    for bad in (("--thin-tm", "warm"), ("--thin-tm", "30C"), ("--thin-tm", "nan"),
                ("--thin-tm", "30", "--thin-thal", "end2"), ("--thin-tm", "30", "--kmer-size", "1"),
                ("--thin-tm", "30", "--keep-all", "true"), ("--thin-tm", "30", "--devices", "0,1")):
        rc_, out = parse(host, "-i", "a", "-o", "b", "--thin-panel", "true", *bad)
        assert rc_ == 2 and "--thin-" in out, (bad, out)
    # without --thin-panel true the values are not read, whatever they say
    rc_, out = parse(host, "-i", "a", "-o", "b", "--thin-tm", "warm", "--thin-thal", "end2")
    assert rc_ == 0 and kv(out)["thin_panel"] == "false"
    # ... and without --thin-tm the mode is not read
    rc_, out = parse(host, "-i", "a", "-o", "b", "--thin-panel", "true", "--thin-thal", "end2")
    assert rc_ == 0 and kv(out)["thin_tm"] == ""
    monkeypatch.setenv("THIN_PANEL", "true")
    monkeypatch.setenv("THIN_TM", "41.5")
    monkeypatch.setenv("THIN_THAL", "end1")
    got = kv(parse(host, "-i", "a", "-o", "b")[1])
    assert got["thin_tm"] == "41.5" and got["thin_thal"] == "end1"
    rc_, out = parse(host, "--help")
    assert rc_ == 2 and "--thin-tm <...>  [env: THIN_TM=]" in out and "--thin-thal <...>  [env: THIN_THAL=]" in out


def test_the_host_text_is_the_models_render(host):
    host.odm_thin_thal_block.argtypes = [C.c_int, C.c_float] + [C.c_int] * 3 + [C.c_longlong] * 8 + [C.c_char_p,
                                                                                                     C.c_size_t]
    for mode, thr, M, E, G, rest in ((1, 30.0, 2, 3, 1, (4, 60, 5, 65, 7, 69, 69, 130)),
                                     (2, 41.256, 0, 13, 3, (0, 0, 1, 2, 0, 5, 4, 1000000)),
                                     (1, -5.0, 1, 0, 1, (10, 10, 0, 0, 0, 0, 0, 0))):
        buf = C.create_string_buffer(1 << 12)
        n = host.odm_thin_thal_block(mode, thr, M, E, G, *rest, buf, 1 << 12)
        assert n > 0 and buf.value.decode() == ttm.render_block(mode, thr, M, E, G, *rest)
    assert ttm.render_block("end1", 30.0, 2, 3, 1, 4, 60, 5, 65, 7, 69, 69, 130) == (
        "\nPanel thinning (thal END1, t >= 30.00 C; matches within 2 mismatches, last 3 bases exact, gain >= 1):\n"
        "  Primers:  kept 9 of 125 (forward 4 of 60, reverse 5 of 65), 7 forced\n"
        "  Segments: held 69/130 by all 125, 69/130 by the kept 9\n")
