"""od-msspe-hip --seed-mismatches / --seed-3p-exact / --seed-tm / --seed-thal: extending a panel on what it covers.

On the 40 x 6,000 alignment of stage_a_excluding_model.cases, with a panel of the unseeded winners' 5' variants (words
that occur nowhere in the alignment): without the flags the panel changes nothing stage A picks and the output is the
recorded one of the commit before the flags existed (tests/golden/tolerant_cli_parent.json); with --seed-mismatches 1
the CSV holds the tolerant model's winners, the report opens with the model's seeding block and covers panel and new
primers together; --seed-tm is held against the model the same way.  --keep-all true keeps every stage A winner, so
the CSV is stage A's answer.  On the 180 x 12,000 alignment of test_gpu_repick_cli.py a re-pick round with the flag is
the extension run with the flag.  The usage errors are reported."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import coverage_thal_model as ctm
from stage_a_excluding_model import CachedSegments
from stage_a_seeded_model import SeededModel
from stage_a_tolerant_model import TolerantModel, first_base_changed, render_block
from test_seeded_cli import HEADER, report_of

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"
GOLDEN = ROOT / "tests" / "golden" / "tolerant_cli_parent.json"
FIELDS = (500, 250, 50, 13, 1000, 1)   # the CLI's defaults; 40 records: max_mismatch_segments 1


def run(fa, csv, *extra):
    return subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                          capture_output=True, text=True, timeout=600)


def rows(path):
    return [line.split(",") for line in Path(path).read_text().splitlines()[1:] if line]


def words(path, direction):
    return [r[2] for r in rows(path) if r[0] == direction]


def inputs(m, oracle, directory):
    """The alignment as FASTA, the panel CSV (three 5' variants of the first winners per direction, absent from the
    alignment) and what the models need."""
    g = m.synth.aligned_genomes(40, 6000)
    fa = Path(directory) / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    segs = CachedSegments(oracle.Segments([bytes(x).decode() for x in g], *FIELDS[:4]))
    plain = [SeededModel(segs, d) for d in (0, 1)]
    winners = [p.candidates(FIELDS[4], FIELDS[5]) for p in plain]
    panel = [first_base_changed([w for w, _ in winners[d][:3]], plain[d].vocab, 13) for d in (0, 1)]
    assert all(len(p) == 3 for p in panel)
    csv = Path(directory) / "panel.csv"
    csv.write_text(HEADER + "".join(f"{'FR'[d]},Primer_{i}_{'FR'[d]},{w},0.5,50,1,50\n"
                                    for d in (0, 1) for i, w in enumerate(panel[d])))
    return g, fa, csv, segs, winners, panel


@pytest.fixture(scope="module")
def case(oracle, tmp_path_factory):
    import msspe_amd as m
    return (m,) + inputs(m, oracle, tmp_path_factory.mktemp("tolerant"))


def coverage_text(m, g, fwd, rev):
    eng = m.Engine(0)
    try:
        return report_of(eng.segment_coverage(g, m.KmerOpt(500, 250, 50, 13, 0, 0), fwd, rev))
    finally:
        eng.close()


def test_without_the_flags_the_output_is_the_recorded_one(case, tmp_path):
    m, g, fa, panel_csv, segs, winners, panel = case
    want = json.loads(GOLDEN.read_text())
    for name, extra in (("extend", ("--existing-primers", str(panel_csv), "--keep-all", "true")),
                        ("extend_filtered", ("--existing-primers", str(panel_csv))),
                        ("repick", ("--repick-rounds", "2"))):
        got = run(fa, tmp_path / f"{name}.csv", *extra)
        assert got.returncode == 0, got.stderr
        assert (tmp_path / f"{name}.csv").read_text() == want[name]["csv"], name
        assert got.stdout == want[name]["stdout"], name
    # the absent panel words seed nothing: stage A's winners are the unseeded ones
    for d in (0, 1):
        assert words(tmp_path / "extend.csv", "FR"[d]) == [w for w, _ in winners[d]]
    assert "Seeding" not in want["extend"]["stdout"] + want["repick"]["stdout"]


def test_seed_mismatches_gives_the_models_winners_and_block(case, tmp_path):
    m, g, fa, panel_csv, segs, winners, panel = case
    got = run(fa, tmp_path / "t.csv", "--existing-primers", str(panel_csv), "--keep-all", "true",
              "--seed-mismatches", "1")
    assert got.returncode == 0, got.stderr
    want = [TolerantModel(segs, d, g, FIELDS).candidates_tolerant(FIELDS[4], FIELDS[5], panel[d], 1, 3) for d in (0, 1)]
    new = [words(tmp_path / "t.csv", "F"), words(tmp_path / "t.csv", "R")]
    for d in (0, 1):
        assert new[d] == [w for w, _ in want[d][0]] != [w for w, _ in winners[d]]
        assert not set(new[d]) & {w for w, _ in winners[d][:3]}
    names = [r[1] for r in rows(tmp_path / "t.csv") if r[0] == "F"]
    assert names == [f"Primer_{3 + i}_F" for i in range(len(names))]       # numbered on from the panel
    n_seg = want[0][1].size
    block = render_block(1, 3, (int(want[0][1].sum()), n_seg, 3), (int(want[1][1].sum()), n_seg, 3))
    assert int(want[0][1].sum()) > 0 and got.stdout == block + coverage_text(m, g, new[0] + panel[0], new[1] + panel[1])
    # --seed-3p-exact is read with it; the environment is read like the flag
    wide = run(fa, tmp_path / "e0.csv", "--existing-primers", str(panel_csv), "--keep-all", "true",
               "--seed-mismatches", "2", "--seed-3p-exact", "0")
    assert wide.returncode == 0, wide.stderr
    want2 = [TolerantModel(segs, d, g, FIELDS).candidates_tolerant(FIELDS[4], FIELDS[5], panel[d], 2, 0) for d in (0, 1)]
    assert words(tmp_path / "e0.csv", "F") == [w for w, _ in want2[0][0]]
    assert words(tmp_path / "e0.csv", "R") == [w for w, _ in want2[1][0]]
    assert wide.stdout.startswith(render_block(2, 0, (int(want2[0][1].sum()), n_seg, 3), (int(want2[1][1].sum()), n_seg, 3)))


def test_seed_tm_gives_the_models_winners_and_block(case, oracle, oracle_tables, tmp_path):
    m, g, fa, panel_csv, segs, winners, panel = case
    models = [TolerantModel(segs, d, g, FIELDS) for d in (0, 1)]
    cache = {}
    # a threshold between the seeds' scores, so that some matches hold and some do not
    ts = []
    for d in (0, 1):
        f, r = ([], sorted(panel[d])) if d else (sorted(panel[d]), [])
        res = ctm.coverage_thal(oracle_tables, g, 500, 250, 50, 13, f, r, 1, 3, "end1", 0.0, oracle.ntthal_args(), cache=cache)
        ts += [max(0.0, float(t)) for t in res["matches"]["t"]]
    thr = round(float(np.median(ts)), 1) + 0.05
    want = [models[d].candidates_tolerant(FIELDS[4], FIELDS[5], panel[d], 1, 3, "end1", thr, oracle_tables,
                                          oracle.ntthal_args(), cache) for d in (0, 1)]
    mode0 = [models[d].candidates_tolerant(FIELDS[4], FIELDS[5], panel[d], 1, 3) for d in (0, 1)]
    assert any(0 < int(want[d][1].sum()) < int(mode0[d][1].sum()) for d in (0, 1)), (thr, sorted(ts)[:5], sorted(ts)[-5:])
    got = run(fa, tmp_path / "tm.csv", "--existing-primers", str(panel_csv), "--keep-all", "true", "--seed-mismatches", "1",
              "--seed-tm", f"{thr:.2f}", "--seed-thal", "end1")
    assert got.returncode == 0, got.stderr
    for d in (0, 1):
        assert words(tmp_path / "tm.csv", "FR"[d]) == [w for w, _ in want[d][0]]
    n_seg = want[0][1].size
    assert got.stdout.startswith(render_block(1, 3, (int(want[0][1].sum()), n_seg, 3), (int(want[1][1].sum()), n_seg, 3),
                                              "end1", thr))


@pytest.fixture(scope="module")
def big_fa(tmp_path_factory):
    import msspe_amd as m
    g = np.concatenate([m.synth.aligned_genomes(60, 12000, seed=70 + c) for c in range(3)])
    path = tmp_path_factory.mktemp("repick_tolerant") / "in.fa"
    path.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    return path


def test_a_repick_round_seeds_tolerantly_like_the_extension_run(big_fa, tmp_path):
    d = tmp_path
    r1 = run(big_fa, d / "run1.csv", "--rejected-out", str(d / "r.csv"), "--seed-mismatches", "1")
    assert r1.returncode == 0, r1.stderr
    assert "Seeding" not in r1.stdout                      # round 0 has no panel: nothing seeds
    r2 = run(big_fa, d / "run2.csv", "--existing-primers", str(d / "run1.csv"), "--exclude-primers", str(d / "r.csv"),
             "--seed-mismatches", "1")
    assert r2.returncode == 0, r2.stderr
    r2x = run(big_fa, d / "run2x.csv", "--existing-primers", str(d / "run1.csv"), "--exclude-primers", str(d / "r.csv"))
    assert r2x.returncode == 0, r2x.stderr
    r3 = run(big_fa, d / "run3.csv", "--repick-rounds", "2", "--seed-mismatches", "1")
    assert r3.returncode == 0, r3.stderr
    one, two, three = [(d / f"run{i}.csv").read_text() for i in (1, 2, 3)]
    assert len(rows(d / "r.csv")) >= 3 and three.startswith(one + two[two.index("\n") + 1:])
    assert r2.stdout.count("\nSeeding (up to 1 mismatches, last 3 bases exact):\n") == 1
    blocks = r3.stdout.count("\nSeeding (up to 1 mismatches, last 3 bases exact):\n")
    assert blocks == r3.stdout.count("Re-pick round") - 1 >= 1      # every round but round 0 seeds
    assert r3.stdout.index("Re-pick round 0") < r3.stdout.index("Seeding") < r3.stdout.index("Re-pick round 1")
    # the first seeding block of the re-pick run is the extension run's
    assert r2.stdout[:r2.stdout.index("\nCoverage report")] in r3.stdout
    # the tolerant extension never adds more primers than the exact one: the panel covers at least as much
    assert len(rows(d / "run2.csv")) <= len(rows(d / "run2x.csv"))


@pytest.mark.parametrize("extra,what", [
    (("--seed-thal", "any"), "'--seed-thal' needs '--seed-tm <C>'"),
    (("--seed-mismatches", "1", "--devices", "0"), "--devices"),
    (("--seed-tm", "30", "--devices", "0,1"), "--devices"),
    (("--repick-rounds", "1", "--seed-mismatches", "14"), "--kmer-size"),
    (("--repick-rounds", "1", "--seed-mismatches", "1", "--seed-3p-exact", "x"), "--seed-3p-exact"),
    (("--repick-rounds", "1", "--seed-tm", "warm"), "--seed-tm"),
    (("--repick-rounds", "1", "--seed-tm", "30", "--seed-thal", "end2"), "[possible values: any, end1]")])
def test_usage_errors(case, tmp_path, extra, what):
    fa = case[2]
    csv = tmp_path / "out.csv"
    got = run(fa, csv, *extra)
    assert got.returncode == 2
    assert "--seed-" in got.stderr and what in got.stderr
    assert not csv.exists()
