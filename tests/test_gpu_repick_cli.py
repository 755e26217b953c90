"""od-msspe-hip --exclude-primers / --rejected-out / --repick-rounds: re-picking the primers the filters drop.

On the 180 x 12,000 alignment of test_seeded_cli.py: --repick-rounds 0 and a header-only --exclude-primers change
nothing; a re-pick round is exactly an --existing-primers run on the first run's CSV that excludes the first run's
rejected candidates (run 3 = run 1 followed by run 2, and run 2's coverage report); nothing in the final CSV was
rejected; covered segments never go down from round to round; the usage errors are reported."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"
REASONS = {"stage_b", "background", "panel_dimer", "cover"}


@pytest.fixture(scope="module")
def fa(tmp_path_factory):
    import msspe_amd as m
    g = np.concatenate([m.synth.aligned_genomes(60, 12000, seed=70 + c) for c in range(3)])
    path = tmp_path_factory.mktemp("repick") / "in.fa"
    path.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    return path


def run(fa, csv, *extra):
    return subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                          capture_output=True, text=True, timeout=600)


def rows(path):
    return [line.split(",") for line in Path(path).read_text().splitlines()[1:] if line]


def report(stdout):
    """stdout without the per-round lines"""
    return "".join(line for line in stdout.splitlines(keepends=True) if not line.startswith("Re-pick round"))


def covered(stdout):
    return int(re.search(r"Segments:\s+(\d+)/\d+ covered", stdout).group(1))


@pytest.fixture(scope="module")
def runs(fa, tmp_path_factory):
    """Run 1: plain, with --rejected-out.  Run 2: extends run 1's CSV, excluding run 1's rejected candidates.
    Run 3: --repick-rounds 1."""
    d = tmp_path_factory.mktemp("runs")
    r1 = run(fa, d / "run1.csv", "--rejected-out", str(d / "r.csv"))
    assert r1.returncode == 0, r1.stderr
    r2 = run(fa, d / "run2.csv", "--existing-primers", str(d / "run1.csv"), "--exclude-primers", str(d / "r.csv"))
    assert r2.returncode == 0, r2.stderr
    r3 = run(fa, d / "run3.csv", "--repick-rounds", "1", "--rejected-out", str(d / "r3.csv"))
    assert r3.returncode == 0, r3.stderr
    return d, r1, r2, r3


def test_round_0_rejects_and_round_1_finds_new_primers(runs):
    """What the other tests stand on: at least 3 rejected candidates per direction in round 0, a new primer in round 1."""
    d, _, _, r3 = runs
    rej = rows(d / "r.csv")
    assert (d / "r.csv").read_text().splitlines()[0] == "direction,name,primers,round,reason"
    for direction in "FR":
        assert sum(1 for r in rej if r[0] == direction) >= 3, direction
    assert {r[4] for r in rej} <= REASONS and {r[3] for r in rej} == {"0"}
    assert len(rows(d / "run2.csv")) >= 1
    lines = [line for line in r3.stdout.splitlines() if line.startswith("Re-pick round")]
    assert len(lines) == 2, r3.stdout
    n1, n2 = len(rows(d / "run1.csv")), len(rows(d / "run2.csv"))
    assert lines[0] == f"Re-pick round 0: {n1} new, {len(rej)} rejected, {n1} kept so far"
    assert lines[1].startswith(f"Re-pick round 1: {n2} new, ") and lines[1].endswith(f" rejected, {n1 + n2} kept so far")


def test_zero_rounds_and_an_empty_exclusion_file_change_nothing(fa, runs, tmp_path):
    d, r1, _, _ = runs
    empty = tmp_path / "none.csv"
    empty.write_text("direction,name,primers,round,reason\n")
    got = run(fa, tmp_path / "same.csv", "--repick-rounds", "0", "--exclude-primers", str(empty))
    assert got.returncode == 0, got.stderr
    assert (tmp_path / "same.csv").read_bytes() == (d / "run1.csv").read_bytes()
    assert got.stdout == r1.stdout


def test_a_repick_round_is_an_extension_run_that_excludes_the_rejected(runs):
    d, r1, r2, r3 = runs
    one, two, three = [(d / f"run{i}.csv").read_text() for i in (1, 2, 3)]
    assert three == one + two[two.index("\n") + 1:]
    assert report(r3.stdout) == r2.stdout
    # run 2 picked none of what run 1 rejected, and nothing of run 1's panel
    banned = {(r[0], r[2]) for r in rows(d / "r.csv")}
    assert not {(r[0], r[2]) for r in rows(d / "run2.csv")} & banned
    assert not {(r[0], r[2]) for r in rows(d / "run2.csv")} & {(r[0], r[2]) for r in rows(d / "run1.csv")}
    # rows are numbered on, per direction
    for direction in "FR":
        names = [r[1] for r in rows(d / "run3.csv") if r[0] == direction]
        assert names == [f"Primer_{i}_{direction}" for i in range(len(names))]


def test_nothing_in_the_final_csv_was_rejected_and_coverage_never_goes_down(fa, runs, tmp_path):
    d, r1, _, r3 = runs
    rej3 = rows(d / "r3.csv")
    assert {r[3] for r in rej3} <= {"0", "1"} and {r[4] for r in rej3} <= REASONS
    assert [r for r in rej3 if r[3] == "0"] == rows(d / "r.csv")
    assert not {(r[0], r[2]) for r in rows(d / "run3.csv")} & {(r[0], r[2]) for r in rej3}
    more = run(fa, tmp_path / "more.csv", "--repick-rounds", "2", "--rejected-out", str(tmp_path / "rm.csv"))
    assert more.returncode == 0, more.stderr
    assert not {(r[0], r[2]) for r in rows(tmp_path / "more.csv")} & {(r[0], r[2]) for r in rows(tmp_path / "rm.csv")}
    # kept primers are never removed: each run's CSV starts with the one before it
    assert (tmp_path / "more.csv").read_text().startswith((d / "run3.csv").read_text())
    assert covered(r1.stdout) <= covered(r3.stdout) <= covered(more.stdout)


@pytest.mark.parametrize("extra,what", [(("--repick-rounds", "1", "--tubes", "2"), "--tubes"),
                                        (("--repick-rounds", "1", "--devices", "0"), "--devices"),
                                        (("--repick-rounds", "17"), "[0 .. 16]")])
def test_usage_errors(fa, tmp_path, extra, what):
    csv = tmp_path / "out.csv"
    got = run(fa, csv, *extra)
    assert got.returncode == 2
    assert "--repick-rounds" in got.stderr and what in got.stderr
    assert not csv.exists()


def test_malformed_exclusion_file_is_a_usage_error(fa, tmp_path):
    bad = tmp_path / "bad.csv"
    bad.write_text("direction,name,primers,round,reason\nF,Rejected_0_F,ACGTACGTACGT,0,cover\n")
    csv = tmp_path / "out.csv"
    got = run(fa, csv, "--exclude-primers", str(bad))
    assert got.returncode == 2
    assert "--exclude-primers" in got.stderr and "line 2" in got.stderr and "12 bases" in got.stderr
    assert not csv.exists()
