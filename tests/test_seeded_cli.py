"""od-msspe-hip --existing-primers: extending a panel.  A header-only panel changes nothing; a panel taken from an
earlier run gives new primers only, none equal to or dimerising with a panel primer, numbered on from the panel,
and a coverage report over panel and new primers together; a malformed panel is a usage error."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"
HEADER = "direction,name,primers,gc,avg,std,tm\n"


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def aln(m, tmp_path_factory):
    g = np.concatenate([m.synth.aligned_genomes(60, 12000, seed=70 + c) for c in range(3)])
    fa = tmp_path_factory.mktemp("panel") / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    return g, fa


def run(fa, csv, *extra):
    return subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                          capture_output=True, text=True, timeout=600)


def rows(csv_text):
    return [line.split(",") for line in csv_text.splitlines()[1:] if line]


def report_of(hit):
    """coverage_report()'s text (main.rs:518-594) from a hit matrix (n_seq, P), f32 arithmetic as there."""
    f32 = np.float32
    covered, total = int(hit.sum()), int(hit.size)
    per = [f32(int(r.sum())) / f32(hit.shape[1]) * f32(100.0) for r in hit]
    well = sum(1 for c in per if c >= f32(80.0))
    out = "\nCoverage report:\n"
    out += f"  Segments:  {covered}/{total} covered ({float(f32(100.0) * f32(covered) / f32(total)):.1f}%)\n"
    out += (f"  Sequences: {well}/{hit.shape[0]} at ≥" f"80% coverage (min {float(min(per)):.1f}%, "
            f"max {float(max(per)):.1f}%)\n")
    unc = [str(p) for p in range(hit.shape[1]) if not hit[:, p].any()]
    out += "  All partitions have primer coverage\n" if not unc else f"  Uncovered partitions: [{', '.join(unc)}]\n"
    return out


def test_header_only_panel_changes_nothing(aln, tmp_path):
    _, fa = aln
    base = run(fa, tmp_path / "a.csv")
    assert base.returncode == 0, base.stderr
    panel = tmp_path / "panel.csv"
    panel.write_text(HEADER)
    got = run(fa, tmp_path / "b.csv", "--existing-primers", str(panel))
    assert got.returncode == 0, got.stderr
    assert (tmp_path / "b.csv").read_bytes() == (tmp_path / "a.csv").read_bytes()
    assert got.stdout == base.stdout


def test_panel_from_an_earlier_run_is_extended(m, oracle, oracle_tables, aln, tmp_path):
    g, fa = aln
    first = run(fa, tmp_path / "first.csv")
    assert first.returncode == 0, first.stderr
    old = rows((tmp_path / "first.csv").read_text())
    panel_f = [r for r in old if r[0] == "F"][:6]
    panel_r = [r for r in old if r[0] == "R"][:4]
    assert len(panel_f) == 6 and len(panel_r) == 4
    panel = tmp_path / "panel.csv"
    panel.write_text(HEADER + "".join(",".join(r) + "\n" for r in panel_f + panel_r))
    got = run(fa, tmp_path / "new.csv", "--existing-primers", str(panel))
    assert got.returncode == 0, got.stderr
    new = rows((tmp_path / "new.csv").read_text())
    new_f = [r for r in new if r[0] == "F"]
    new_r = [r for r in new if r[0] == "R"]
    assert new_f and new_r
    pf, pr = [r[2] for r in panel_f], [r[2] for r in panel_r]
    words = [r[2] for r in new]
    # new primers only, numbered on from the panel per direction
    assert not set(words) & set(pf + pr)
    assert [r[1] for r in new_f] == [f"Primer_{6 + i}_F" for i in range(len(new_f))]
    assert [r[1] for r in new_r] == [f"Primer_{4 + i}_R" for i in range(len(new_r))]
    # no ANY conflict with a panel primer, in either order (the oracle's dG rule at the CLI's defaults)
    pool = words + pf + pr
    _, _, cf, _ = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(), -9000.0)
    n = len(words)
    assert not cf[:n, n:].any() and not cf[n:, :n].any()
    # the report is the coverage of panel and new primers together
    eng = m.Engine(0)
    try:
        hit = eng.segment_coverage(g, m.KmerOpt(500, 250, 50, 13, 0, 0), pf + [r[2] for r in new_f],
                                   pr + [r[2] for r in new_r])
    finally:
        eng.close()
    assert got.stdout == report_of(hit)


@pytest.mark.parametrize("bad,what", [("F,Primer_0_F,ACGTACGTACGT,0.5,50,1,50", "12 bases"),
                                      ("R,Primer_0_R,ACGTACGTACGNA,0.5,50,1,50", "other than A, C, G and T")])
def test_malformed_panel_is_a_usage_error(aln, tmp_path, bad, what):
    _, fa = aln
    panel = tmp_path / "panel.csv"
    panel.write_text(HEADER + "F,Primer_0_F,ACGTACGTACGTA,0.5,50,1,50\n" + bad + "\n")
    csv = tmp_path / "out.csv"
    got = run(fa, csv, "--existing-primers", str(panel))
    assert got.returncode == 2
    assert "line 3" in got.stderr and what in got.stderr
    assert not csv.exists()
