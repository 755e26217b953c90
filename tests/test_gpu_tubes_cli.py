"""od-msspe-hip --tubes N: the primers are split into tubes (msspe_conflict_tubes) instead of covered.  The CSV gains a
1-based tube column and loses exactly the primers that fit no tube, no two primers of one tube conflict, the report's
block counts the CSV's rows, --keep-all true keeps the unplaced rows with an empty field, the flag refuses --devices,
--cover-on-device true and --existing-primers, and a later run reads the CSV back as a panel."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
HEADER = "direction,name,primers,gc,avg,std,tm"
# the filters --keep-all true bypasses, switched off where they can be (homopolymer runs are taken out by the test), so
# that the run with --keep-all true lists the primers the tube split sees
NO_FILTER = ["--check-hairpin", "false", "--disable-tm-stddev", "true", "--disable-min-max-tm", "true",
             "--max-self-dimer-any-tm", "1000", "--max-self-dimer-end-tm", "1000"]
T = 3


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def alignment(m, tmp_path_factory):
    g = np.concatenate([m.synth.aligned_genomes(40, 12000, seed=310 + j) for j in range(3)])
    fa = tmp_path_factory.mktemp("tubes") / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    return fa


def cli(fa, csv, *extra):
    return subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                          capture_output=True, text=True, timeout=600)


def run(fa, csv, *extra):
    r = cli(fa, csv, *extra)
    assert r.returncode == 0, r.stderr
    lines = Path(csv).read_text().splitlines()
    return r.stdout, lines[0], [l.split(",") for l in lines[1:] if l]


@pytest.fixture(scope="module")
def runs(alignment):
    d = alignment.parent
    return {"all": run(alignment, d / "all.csv", "--keep-all", "true", *NO_FILTER),
            "tubes": run(alignment, d / "tubes.csv", "--tubes", str(T), *NO_FILTER),
            "tubes_all": run(alignment, d / "tubes_all.csv", "--tubes", str(T), "--keep-all", "true", *NO_FILTER)}


@pytest.fixture(scope="module")
def assignment(m, runs):
    """The tube of every primer the split sees, recomputed with Engine.conflict_tubes over the distinct primers in the
    CLI's order (forward rows, then reverse rows), and the conflicting pairs of those primers."""
    host = C.CDLL(str(HOST_LIB))
    _, header, rows = runs["all"]
    assert header == HEADER
    rows = [r for r in rows if not host.odm_is_run(r[2].encode())]
    assert [r[0] for r in rows] == sorted((r[0] for r in rows), key="FR".index)
    words = list(dict.fromkeys(r[2] for r in rows))
    eng = m.Engine(0)
    try:
        tube, used, unplaced = eng.conflict_tubes(words, m.Chem.ntthal(), -9000.0, T)
        e, _ = eng.cross_dimer_edges(words, m.Chem.ntthal(), -9000.0, capacity=1 << 22)
    finally:
        eng.close()
    pairs = {(words[a], words[b]) for a, b in zip(e["a"].tolist(), e["b"].tolist())}
    return rows, dict(zip(words, tube.tolist())), pairs


def block(stdout):
    at = stdout.index(f"Tube assignment (up to {T} tubes):")
    text = stdout[at:]
    used = int(re.search(r"Tubes used: (\d+)", text).group(1))
    per = {int(a): int(b) for a, b in re.findall(r"Tube (\d+): (\d+) primers", text)}
    return used, per, int(re.search(r"Unplaced: (\d+) primers", text).group(1))


def test_tubes_csv_is_the_keep_all_csv_minus_the_unplaced(runs, assignment):
    rows, tube, pairs = assignment
    stdout, header, got = runs["tubes"]
    assert header == HEADER + ",tube"
    want = [r for r in rows if tube[r[2]] != 255]
    assert len(want) < len(rows) or all(t != 255 for t in tube.values())
    assert [g[0:1] + g[2:7] for g in got] == [w[0:1] + w[2:7] for w in want]       # the names are renumbered
    assert [g[7] for g in got] == [str(tube[w[2]] + 1) for w in want]
    assert {g[7] for g in got} <= {str(t) for t in range(1, T + 1)} and len(got) > 0
    for d in "FR":
        assert [g[1] for g in got if g[0] == d] == [f"Primer_{i}_{d}" for i in range(sum(g[0] == d for g in got))]
    by_tube = {}
    for g in got:
        by_tube.setdefault(g[7], []).append(g[2])
    for members in by_tube.values():                     # no two primers of one tube conflict, in either order
        for a in members:
            for b in members:
                assert a == b or (a, b) not in pairs, (a, b)
    used, per, unplaced = block(stdout)
    assert used == len(by_tube) and per == {int(t): len(v) for t, v in by_tube.items()}
    assert unplaced == 0                                 # the unplaced rows are gone from the CSV and the report
    assert stdout.index("Tube assignment") > stdout.index("Coverage")


def test_tubes_with_keep_all_keeps_the_unplaced_rows(runs, assignment):
    rows, tube, _ = assignment
    stdout, header, got = runs["tubes_all"]
    _, _, everything = runs["all"]
    assert header == HEADER + ",tube"
    assert [g[:7] for g in got] == everything
    assert {g[7] for g in got} <= {""} | {str(t) for t in range(1, T + 1)}
    if len(rows) == len(everything):     # no homopolymer runs: --keep-all true splits the primers --tubes alone does
        assert [g[7] for g in got] == ["" if tube[g[2]] == 255 else str(tube[g[2]] + 1) for g in got]
    used, per, unplaced = block(stdout)
    assert unplaced == sum(g[7] == "" for g in got)
    assert per == {t: sum(g[7] == str(t) for g in got) for t in range(1, used + 1)}
    assert sum(per.values()) + unplaced == len(got)


@pytest.mark.parametrize("extra,flag", [(("--devices", "0,0"), "--devices"),
                                        (("--cover-on-device", "true"), "--cover-on-device"),
                                        (("--existing-primers", "PANEL"), "--existing-primers")])
def test_flag_combinations_are_usage_errors(alignment, runs, tmp_path, extra, flag):
    extra = tuple(str(alignment.parent / "tubes.csv") if x == "PANEL" else x for x in extra)
    r = cli(alignment, tmp_path / "x.csv", "--tubes", str(T), *extra)
    assert r.returncode == 2 and flag in (r.stderr + r.stdout) and "--tubes" in (r.stderr + r.stdout)
    assert not (tmp_path / "x.csv").exists()


def test_a_tubes_csv_reads_back_as_a_panel(alignment, runs, tmp_path):
    stdout, header, rows = run(alignment, tmp_path / "next.csv", "--existing-primers",
                               str(alignment.parent / "tubes.csv"))
    assert header == HEADER and "Tube assignment" not in stdout
