"""The model of msspe_segment_coverage_thal* (tests/coverage_thal_model.py) on hand-built one-segment alignments, the
CLI's --coverage-tm / --coverage-thal through the host hooks, and the block's host text against the model's render --
no GPU needed."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import coverage_thal_model as ctm
from test_coverage_mm_model import one_segment, parse, rc

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
P_FWD = "ACGTTGCAGGATC"      # 13 bases, no reverse-complement symmetry
TAIL = "GATTACAGGCTCA"


@pytest.fixture(scope="module")
def host():
    import msspe_amd
    msspe_amd.load_library()
    return C.CDLL(str(LIB))


@pytest.fixture(scope="module")
def run(oracle, oracle_tables):
    def go(seg, fwd, rev, M, E, thr=30.0, mode="any", W=13, k=13):
        L = seg.shape[1]
        return ctm.coverage_thal(oracle_tables, seg, L, L, W, k, fwd, rev, M, E, mode, thr, oracle.ntthal_args())
    return go


def thal(oracle, tables, a, b, mode="any"):
    res = oracle.thal(tables, a, b, ctm.MODES[mode], oracle.ntthal_args())
    return (np.inf, 0.0) if res.no_structure else (res.dG, res.t)


def test_a_forward_exact_match_scores_the_primer_against_its_reverse_complement(run, oracle, oracle_tables):
    r = run(one_segment(P_FWD, TAIL), [P_FWD], [], 0, 3)
    assert r["count"] == 1 and r["templates"] == [rc(P_FWD)]
    m = r["matches"][0]
    assert (int(m["primer"]), int(m["segment"]), int(m["offset"]), int(m["mismatches"])) == (0, 0, 0, 0)
    dg, t = thal(oracle, oracle_tables, P_FWD, rc(P_FWD))
    assert t > 30.0 and (m["dg"], m["t"]) == (dg, t) and m["stable"] == 1
    assert r["held"].tolist() == [[2]] and r["t_best"].tolist() == [[t]]
    assert r["primer_segments"].tolist() == [1] and r["primer_held"].tolist() == [1]


def test_a_reverse_primers_template_is_the_tail_as_written(run, oracle, oracle_tables):
    rp = rc(TAIL)
    r = run(one_segment(P_FWD, TAIL), [], [rp], 0, 3)
    assert r["count"] == 1 and r["templates"] == [TAIL] and TAIL != rc(TAIL)
    dg, t = thal(oracle, oracle_tables, rp, TAIL)
    assert (r["matches"][0]["dg"], r["matches"][0]["t"]) == (dg, t)
    # the other orientation is another number, so a swapped template cannot pass
    assert thal(oracle, oracle_tables, rp, rc(TAIL)) != (dg, t)
    # with one mismatch the template stays the alignment's own columns, not the primer's complement
    sub = "A" + rp[1:] if rp[0] != "A" else "C" + rp[1:]
    r1 = run(one_segment(P_FWD, TAIL), [P_FWD], [sub], 1, 3)
    assert [int(x) for x in r1["matches"]["primer"]] == [0, 1] and r1["templates"] == [rc(P_FWD), TAIL]
    assert (r1["matches"][1]["dg"], r1["matches"][1]["t"]) == thal(oracle, oracle_tables, sub, TAIL)


def test_a_5p_substitution_lowers_t_and_a_3p_one_is_no_match(run):
    seg = one_segment(P_FWD, TAIL)
    exact = run(seg, [P_FWD], [], 1, 3)["matches"][0]
    five = "T" + P_FWD[1:]
    got = run(seg, [five], [], 1, 3)
    assert got["count"] == 1 and got["matches"][0]["mismatches"] == 1 and got["templates"] == [rc(P_FWD)]
    assert 0.0 < got["matches"][0]["t"] < exact["t"]
    three = P_FWD[:-2] + "A" + P_FWD[-1]
    none = run(seg, [three], [], 1, 3)
    assert none["count"] == 0 and none["held"].tolist() == [[0]] and none["t_best"].tolist() == [[0.0]]
    assert none["primer_segments"].tolist() == [0] and none["primer_held"].tolist() == [0]
    assert run(seg, [three], [], 1, 1)["count"] == 1   # outside the exact 3' bases it is a mismatch like any other


@pytest.mark.parametrize("bad", ["N", "-", "R"])
def test_a_window_with_an_invalid_column_is_never_a_match(run, bad):
    seg = one_segment(P_FWD[:4] + bad + P_FWD[5:], TAIL[:7] + bad + TAIL[8:])
    r = run(seg, [P_FWD], [rc(TAIL)], 13, 0, thr=0.0)
    assert r["count"] == 0 and not r["held"].any()


def test_a_repeat_counts_once_per_segment(run):
    k, W = 6, 20
    rep = "ACGTAC"
    g = np.frombuffer(("ACGTACGTACGTACGTACGT" + "C" * 30 + "ACGTACGTACGTACGTACGT").encode(), dtype=np.uint8)[None]
    r = run(g, [rep, rep, "TTTTTT"], [], 0, 0, thr=0.0, W=W, k=k)
    per_primer = np.bincount(r["matches"]["primer"], minlength=3)
    assert per_primer.tolist() == [4, 4, 0]   # positions 0, 4, 8, 12 of the head window
    assert r["primer_segments"].tolist() == [1, 1, 0] and r["primer_held"].tolist() == [1, 1, 0]
    assert r["matches"]["offset"].tolist() == [0, 4, 8, 12, 0, 4, 8, 12]


def test_thresholds_and_the_tri_state(run):
    seg = one_segment(P_FWD, TAIL)
    weak = "TG" + P_FWD[2:]
    base = run(seg, [P_FWD, weak], [], 2, 3, thr=30.0)
    t = {int(m["primer"]): float(m["t"]) for m in base["matches"]}
    assert t[1] < t[0]
    between = (t[0] + t[1]) / 2
    r = ctm.rethreshold(base, between)
    assert r["held"].tolist() == [[2]] and r["primer_held"].tolist() == [1, 0] and r["primer_segments"].tolist() == [1, 1]
    assert r["t_best"].tolist() == [[t[0]]]
    above = ctm.rethreshold(base, t[0] + 5.0)
    assert above["held"].tolist() == [[1]] and above["primer_held"].tolist() == [0, 0] and above["t_best"].tolist() == [[t[0]]]
    for thr in (0.0, -3.0):   # a threshold <= 0: held = matched
        z = ctm.rethreshold(base, thr)
        assert z["held"].tolist() == [[2]] and z["primer_held"].tolist() == z["primer_segments"].tolist()
    # the rule rounds t to two decimals in f32 first: a threshold equal to the rounded t still holds
    import pyoracle
    assert ctm.is_stable(t[0], pyoracle.round_fixed_f32(t[0], 2))
    assert run(seg, ["TTTTTTTTTTTTT"], [], 0, 0)["held"].tolist() == [[0]]


def kv(out):
    return dict(l.split("=", 1) for l in out.splitlines())


def test_cli_flags_and_usage_errors(host, monkeypatch):
    for v in ("COVERAGE_TM", "COVERAGE_THAL", "COVERAGE_MISMATCHES", "COVERAGE_3P_EXACT", "KMER_SIZE", "MSSPE_DEVICES"):
        monkeypatch.delenv(v, raising=False)
    rc_, out = parse(host, "-i", "a", "-o", "b")
    assert rc_ == 0 and kv(out)["coverage_tm"] == "" and kv(out)["coverage_thal"] == ""
    rc_, out = parse(host, "-i", "a", "-o", "b", "--coverage-tm", "30")
    assert rc_ == 0 and kv(out)["coverage_tm"] == "30" and kv(out)["coverage_thal"] == "any"
    rc_, out = parse(host, "-i", "a", "-o", "b", "--coverage-tm", "-2.5", "--coverage-thal", "end1",
                     "--coverage-mismatches", "2", "--coverage-3p-exact", "4")
    assert rc_ == 0 and kv(out)["coverage_tm"] == "-2.5" and kv(out)["coverage_thal"] == "end1"
    assert kv(out)["coverage_mismatches"] == "2" and kv(out)["coverage_3p_exact"] == "4"
    for bad in (("--coverage-tm", "warm"), ("--coverage-tm", "30C"), ("--coverage-tm", "nan"),
                ("--coverage-tm", "30", "--coverage-thal", "end2"), ("--coverage-tm", "30", "--devices", "0,1"),
                ("--coverage-tm", "30", "--coverage-3p-exact", "14"), ("--coverage-tm", "30", "--kmer-size", "1")):
        rc_, out = parse(host, "-i", "a", "-o", "b", *bad)
        assert rc_ == 2 and "--coverage-" in out, (bad, out)
    # the prefilter's 3' length is read with --coverage-tm too (at 0 mismatches it only shows in the heading)
    assert kv(parse(host, "-i", "a", "-o", "b", "--coverage-tm", "30", "--coverage-3p-exact", "5")[1])[
        "coverage_3p_exact"] == "5"
    # --coverage-thal alone is ignored, whatever it says
    rc_, out = parse(host, "-i", "a", "-o", "b", "--coverage-thal", "end2", "--devices", "0,1")
    assert rc_ == 0
    monkeypatch.setenv("COVERAGE_TM", "41.5")
    monkeypatch.setenv("COVERAGE_THAL", "end1")
    got = kv(parse(host, "-i", "a", "-o", "b")[1])
    assert got["coverage_tm"] == "41.5" and got["coverage_thal"] == "end1"
    rc_, out = parse(host, "--help")
    assert rc_ == 2 and "--coverage-tm <...>  [env: COVERAGE_TM=]" in out
    assert "--coverage-thal <...>  [env: COVERAGE_THAL=]" in out


def test_the_host_text_is_the_models_render(host):
    rng = np.random.default_rng(4)
    names = [f"g{i}" for i in range(7)]
    L, seg, stride = 2000, 500, 250
    lengths = [L, L, 1200, L, 700, L, L]                 # a short record's missing segments are not counted
    seqs = ["A" * n for n in lengths]
    P = (L - seg) // stride + 1
    held = rng.integers(0, 3, size=(7, P)).astype(np.uint8)
    held[3] = 2
    primer_held = np.array([3, 0, 7, 0, 0, 1], dtype=np.uint32)
    recs = "".join(f"{n}\t{s}\n" for n, s in zip(names, seqs)).encode()
    host.odm_coverage_thal_block.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.c_int, C.c_int, C.c_float, C.c_char_p, C.c_size_t]
    for mode, thr, M, E in ((1, 30.0, 2, 3), (2, 41.256, 0, 13), (1, -5.0, 1, 0)):
        buf = C.create_string_buffer(1 << 16)
        n = host.odm_coverage_thal_block(recs, seg, stride, held.ctypes.data, primer_held.ctypes.data, 6, M, E, mode,
                                         thr, buf, 1 << 16)
        want = ctm.render(names, lengths, held, primer_held, seg, stride, M, E, mode, thr)
        assert n > 0 and buf.value.decode() == want
    assert "  Primers:   3 of 6 hold no segment\n" in want and "(thal ANY, t >= -5.00 C; matches within 1 mism" in want
