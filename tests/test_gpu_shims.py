"""The protocol shims (bin/ntthal-hip, bin/primer3_core-hip): an unmodified od-msspe selects its
executables with --ntthal / --primer3 (config.rs:142-147); these speak the same pipes."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BIN = Path(__file__).resolve().parent.parent / "open-msspe-design_amd" / "bin"


def parse_ntthal_output(input_text: str, output: str, threshold: float):
    """delta_g.rs:27-59 restated: zip input lines with 5-line blocks, token 13 = dG."""
    edges = {}
    out_lines = iter(output.splitlines())
    for line in input_text.splitlines():
        first = next(out_lines, None)
        if first is not None:
            toks = first.split()
            if len(toks) > 13:
                dg = np.float32(toks[13])
                if dg < np.float32(threshold):
                    a, b = line.split(",")
                    edges[(a, b)] = "%.2f" % dg
        for _ in range(4):
            next(out_lines, None)
    return edges


def test_ntthal_shim_reproduces_the_reference_transcript(golden_dir):
    """The exact argv of delta_g.rs:93-110 and the transcript of delta_g.rs:206-230."""
    g = json.loads((golden_dir / "ntthal_dimer.json").read_text())
    for temp in (37.0, 25.0):
        vecs = [v for v in g["vectors"] if v["temp_c"] == temp]
        stdin = "\n".join(f'{v["oligo1"]},{v["oligo2"]}' for v in vecs)
        res = subprocess.run([str(BIN / "ntthal-hip"), "-a", "ANY", "-mv", "50.00", "-dv", "3.00", "-n", "0.00",
                              "-d", "250.00", "-t", "%.2f" % temp, "-path", "/nonexistent/primer3_config/", "-i"],
                             input=stdin, capture_output=True, text=True)
        # a missing -path directory is an error for ntthal as well
        assert res.returncode != 0
        res = subprocess.run([str(BIN / "ntthal-hip"), "-a", "ANY", "-mv", "50.00", "-dv", "3.00", "-n", "0.00",
                              "-d", "250.00", "-t", "%.2f" % temp, "-i"],
                             input=stdin, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        lines = res.stdout.splitlines()
        assert len(lines) == 5 * len(vecs)
        for q, v in enumerate(vecs):
            head = lines[5 * q].split()
            assert head[:5] == ["Calculated", "thermodynamical", "parameters", "for", "dimer:"]
            assert (head[7], head[10], head[13], head[16]) == (v["dS"], v["dH"], v["dG"], v["t"])
            rows = [r.replace("\t", " " * v["tab_spaces"]).rstrip() for r in lines[5 * q + 1: 5 * q + 5]]
            assert rows == [d.rstrip() for d in v["drawing"]]
        edges = parse_ntthal_output(stdin, res.stdout, 100000.0)
        assert len(edges) == len(vecs)


def test_ntthal_shim_prints_nothing_for_a_pair_without_structure():
    res = subprocess.run([str(BIN / "ntthal-hip"), "-a", "ANY", "-t", "25", "-i"],
                         input="AAAAAAAAAAAAA,AAAAAAAAAAAAA\nAGGCCTATATCCA,GAAGCAGTATTTT",
                         capture_output=True, text=True)
    assert res.returncode == 0 and len(res.stdout.splitlines()) == 5


def test_primer3_shim_golden(golden_dir):
    """primer.rs:218-250: od-msspe's exact Boulder-IO record in, the five values it reads back out."""
    g = json.loads((golden_dir / "primer3_check_primers.json").read_text())
    res = subprocess.run([str(BIN / "primer3_core-hip")], input=g["format_input"]["expected"],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    kv = dict(l.split("=", 1) for l in res.stdout.splitlines() if "=" in l and l != "=")
    want = g["check_primers"][0]
    assert kv["SEQUENCE_ID"] == want["primer"]
    assert np.float32(kv["PRIMER_LEFT_0_TM"]) == np.float32(want["tm"])
    assert np.float32(kv["PRIMER_LEFT_0_GC_PERCENT"]) == np.float32(want["gc"])
    assert (kv["PRIMER_LEFT_0_SELF_ANY_TH"], kv["PRIMER_LEFT_0_SELF_END_TH"], kv["PRIMER_LEFT_0_HAIRPIN_TH"]) == \
        ("0.00", "0.00", "0.00")
    assert res.stdout.rstrip().endswith("=")


def test_ntthal_shim_answers_the_reference_input_text_in_order(golden_dir):
    """The text of delta_g.rs:162-193 (four ordered pairs, no trailing newline) piped into the shim with
    the reference's argv: one 5-line block per input line, in input order, so that parse_ntthal_output's
    zip (delta_g.rs:31-56) attributes every dG to the right pair."""
    import pyoracle
    g = json.loads((golden_dir / "ntthal_format.json").read_text())
    stdin = g["expected"]
    res = subprocess.run([str(BIN / "ntthal-hip"), "-a", "ANY", "-mv", "50.00", "-dv", "3.00", "-n", "0.00",
                          "-d", "250.00", "-t", "25.00", "-i"], input=stdin, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    pairs = [l.split(",") for l in stdin.split("\n")]
    assert len(lines) == 5 * len(pairs)
    tables = pyoracle.Tables()
    for q, (a, b) in enumerate(pairs):
        want = pyoracle.thal(tables, a, b, pyoracle.ANY, pyoracle.ntthal_args())
        assert lines[5 * q].split()[13] == "%g" % want.dG


# ---- both transcripts against the oracle -------------------------------------------------------------------------------

# a shim that hangs fails its test: a healthy run takes well under a second
SHIM_TIMEOUT = 60
NTTHAL_HEADER = "Calculated thermodynamical parameters for dimer:\tdS = %g\tdH = %g\tdG = %g\tt = %g"
# (argv after "-a MODE", pyoracle.ntthal_args keywords): the reference's argv (delta_g.rs:93-110 at its defaults) and one
# that sets temperature, divalent salt, dNTP, DNA concentration and the loop limit
NTTHAL_RUNS = {
    "reference_argv": (["-mv", "50.00", "-dv", "3.00", "-n", "0.00", "-d", "250.00", "-t", "25.00"], {}),
    "t37_dv1.5_n0.6_d50_maxloop3": (["-t", "37.00", "-dv", "1.50", "-n", "0.60", "-d", "50.00", "-maxloop", "3"],
                                    dict(temp_c=37.0, dv=1.5, dntp=0.6, dna_conc=50.0, max_loop=3)),
}


def mixed_length_pairs(seed, n=200):
    """n pairs of lengths 6, 13 and 20 in random order (the shim groups them by length and scatters the records back
    into input order), three of them without any structure."""
    import random
    rng = random.Random(seed)
    rand = lambda k: "".join(rng.choice("ACGT") for _ in range(k))
    pairs = []
    for _ in range(n - 3):
        k = rng.choice((6, 13, 20))
        pairs.append((rand(k), rand(k)))
    for q, k in zip((17, 90, 151), (13, 6, 20)):
        pairs.insert(q, ("A" * k, "A" * k))
    return pairs


def expected_ntthal_blocks(oracle, tables, pairs, mode, args):
    """Per pair None (no structure: ntthal prints nothing) or (header line, four drawing rows), from the oracle alone."""
    from helpers import draw_dimer
    blocks = []
    for a, b in pairs:
        r = oracle.thal(tables, a, b, {"ANY": oracle.ANY, "END1": oracle.END1}[mode], args)
        if r.no_structure:
            blocks.append(None)
            continue
        rows = draw_dimer(a, b, list(r.ps1[:len(a)]), list(r.ps2[:len(b)]))
        blocks.append((NTTHAL_HEADER % (r.dS, r.dH, r.dG, r.t), [x.replace("\t", " ").rstrip() for x in rows], r.dG))
    return blocks


@pytest.mark.parametrize("run", list(NTTHAL_RUNS))
@pytest.mark.parametrize("mode", ["ANY", "END1"])
def test_ntthal_shim_transcript_against_the_oracle(oracle, oracle_tables, mode, run):
    argv, okw = NTTHAL_RUNS[run]
    pairs = mixed_length_pairs(8100)
    assert {len(a) for a, _ in pairs} == {6, 13, 20}
    blocks = expected_ntthal_blocks(oracle, oracle_tables, pairs, mode, oracle.ntthal_args(**okw))
    assert sum(b is None for b in blocks) >= 3
    res = subprocess.run([str(BIN / "ntthal-hip"), "-a", mode] + argv + ["-i"],
                         input="\n".join(f"{a},{b}" for a, b in pairs), capture_output=True, text=True, timeout=SHIM_TIMEOUT)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    shown = [(p, b) for p, b in zip(pairs, blocks) if b is not None]
    assert len(lines) == 5 * len(shown)
    for q, (p, (head, rows, _)) in enumerate(shown):
        assert lines[5 * q] == head, (q, p)
        assert [r.replace("\t", " ").rstrip() for r in lines[5 * q + 1:5 * q + 5]] == rows, (q, p)
    # the reference's parser (one 5-line block per line it sent) attributes every dG to its own pair
    edges = parse_ntthal_output("\n".join(f"{a},{b}" for (a, b), _ in shown), res.stdout, 100000.0)
    want = {p: "%.2f" % np.float32("%g" % b[2]) for p, b in shown}
    assert len(want) == len(shown) and edges == want


@pytest.mark.parametrize("mode", ["ANY", "END1"])
def test_ntthal_shim_s1_s2_prints_the_block_of_the_one_line_run(oracle, oracle_tables, mode):
    """No chemistry on the command line: ntthal's own defaults (50 / 3 / 0 / 250 nM, 37 C)."""
    a, b = "AGTCCTGCGTGAT", "TGGCCTACATCAG"
    one = subprocess.run([str(BIN / "ntthal-hip"), "-a", mode, "-i"], input=f"{a},{b}\n", capture_output=True, text=True, timeout=SHIM_TIMEOUT)
    two = subprocess.run([str(BIN / "ntthal-hip"), "-a", mode, "-s1", a, "-s2", b], capture_output=True, text=True, timeout=SHIM_TIMEOUT)
    assert one.returncode == 0 and two.returncode == 0, (one.stderr, two.stderr)
    assert two.stdout == one.stdout
    (block,) = expected_ntthal_blocks(oracle, oracle_tables, [(a, b)], mode, oracle.ntthal_args(temp_c=37.0))
    lines = two.stdout.splitlines()
    assert len(lines) == 5 and lines[0] == block[0]
    assert [r.replace("\t", " ").rstrip() for r in lines[1:]] == block[1]


def test_primer3_shim_forty_records_against_the_oracle(oracle, oracle_tables):
    """od-msspe sends all its candidates in one stdin (primer.rs:143-166): 40 records, designed stem-loops and a dimer
    among random 13- and 20-mers, two records with a chemistry of their own; every record answered in order with the
    five values the reference reads back."""
    import random
    rng = random.Random(8200)
    rand = lambda k: "".join(rng.choice("ACGT") for _ in range(k))
    oligos = [rand(13) if q % 2 == 0 else rand(20) for q in range(36)]
    for q, o in zip((0, 9, 22, 31), ("ACGTGAAAACGTA", "GCGCTTTTGCGCA", "GGGCCCTTTGGGC", "AGCCCGTGTAAAC")):
        oligos.insert(q, o)
    assert len(oligos) == 40 and len(set(oligos)) == 40
    own = {9: dict(dv=3.0, dntp=0.2, dna_conc=250.0), 20: dict(dv=0.5, dntp=0.8, dna_conc=20.0)}
    stdin, want = "", []
    for q, p in enumerate(oligos):
        stdin += (f"SEQUENCE_ID={p}\nSEQUENCE_PRIMER={p}\nPRIMER_TASK=check_primers\nPRIMER_MIN_SIZE={len(p)}\n"
                  "PRIMER_MIN_TM=29.00\nPRIMER_MAX_TM=59.00\nPRIMER_OPT_TM=59.00\nPRIMER_PICK_ANYWAY=1\n")
        if q in own:
            c = own[q]
            stdin += (f"PRIMER_SALT_DIVALENT={c['dv']:.2f}\nPRIMER_DNTP_CONC={c['dntp']:.2f}\n"
                      f"PRIMER_DNA_CONC={c['dna_conc']:.2f}\n")
        stdin += "=\n"
        want.append(oracle.check_primers(oracle_tables, [p], oracle.p3_args(**own.get(q, {})))[0])
    assert any(w["hairpin_th"] != 0.0 for w in want) and any(w["self_any_th"] != 0.0 for w in want)
    for q in own:          # the chemistry of such a record moves its Tm
        assert want[q]["tm"] != oracle.check_primers(oracle_tables, [oligos[q]])[0]["tm"]
    res = subprocess.run([str(BIN / "primer3_core-hip")], input=stdin, capture_output=True, text=True, timeout=SHIM_TIMEOUT)
    assert res.returncode == 0, res.stderr
    assert res.stdout.endswith("=\n")
    records = res.stdout.split("\n=\n")          # each record ends with a line holding only "="
    assert records[-1] == "" and len(records) == 41
    for q, (p, w) in enumerate(zip(oligos, want)):
        kv = dict(l.split("=", 1) for l in records[q].splitlines())
        assert kv["SEQUENCE_ID"] == p and kv["SEQUENCE_PRIMER"] == p and kv["PRIMER_LEFT_0_SEQUENCE"] == p, q
        got = tuple(kv["PRIMER_LEFT_0_" + t] for t in ("TM", "GC_PERCENT", "SELF_ANY_TH", "SELF_END_TH", "HAIRPIN_TH"))
        assert got == ("%.3f" % w["tm"], "%.3f" % w["gc"], "%.2f" % w["self_any_th"], "%.2f" % w["self_end_th"],
                       "%.2f" % w["hairpin_th"]), (q, p)
