"""od-msspe-hip --max-cross-dimer-end-tm <C>: the pipeline's conflict graph is the union of the dG rule and the 3'-end
rule (msspe_conflict_graph*).  The default host path, --cover-on-device true and the CLI's own outputs agree byte for
byte; the removed set is checked independently (the union edges of the filtered candidates through
oracle/ref_pipeline.vertex_cover); --tubes 1 against the host's sequential rule fed the same edges; a panel primer
built on a candidate's 3' tail drops that candidate; a threshold nothing reaches changes nothing.

Thresholds: --delta-g-threshold -12000 --max-cross-dimer-end-tm 25.  On the 364 stage-A winners of the alignment used
here that pass stage B, the CPU oracle counts 26 pairs under the dG rule only, 38 under the 3'-end rule only and 10
under both; one of the 38 is (CATAAAGGCAGAT, GATCTGCCATGCG)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import conflict_graph_model as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
HEADER = "direction,name,primers,gc,avg,std,tm\n"
DG, TM = -12000.0, 25.0
RULE = ("--delta-g-threshold", "-12000", "--max-cross-dimer-end-tm", "25")


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fasta(m, tmp_path_factory):
    """The first synthetic alignment of tests/test_gpu_cover_cli.py."""
    g = np.concatenate([m.synth.aligned_genomes(40, 12000, seed=310 + j) for j in range(3)])
    fa = tmp_path_factory.mktemp("graph_cli") / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    return fa


def run(fa, csv, *extra):
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout, Path(csv).read_bytes()


def primers_of(csv):
    return [line.split(",")[2] for line in csv.decode().splitlines()[1:] if line]


@pytest.fixture(scope="module")
def host_run(fasta, tmp_path_factory):
    return run(fasta, tmp_path_factory.mktemp("host") / "host.csv", *RULE)


@pytest.fixture(scope="module")
def candidates(fasta, tmp_path_factory):
    """The filtered candidates: what a run without the cross-dimer stage keeps."""
    _, csv = run(fasta, tmp_path_factory.mktemp("cands") / "all.csv", "--check-cross-dimers", "false", *RULE)
    return primers_of(csv)


@pytest.fixture(scope="module")
def union_edges(m, eng, candidates):
    uniq = list(dict.fromkeys(candidates))
    edges, _ = eng.conflict_graph_edges(uniq, m.Chem.ntthal(), m.ConflictRule.of(DG, TM))
    return uniq, edges


def test_device_cover_gives_the_host_paths_output(fasta, host_run, tmp_path):
    dev = run(fasta, tmp_path / "dev.csv", "--cover-on-device", "true", *RULE)
    assert dev[1] == host_run[1]
    assert dev[0] == host_run[0]
    assert "Cross-dimer conflicts among" in host_run[0] and "3'-end only" in host_run[0]


def test_removed_set_is_the_cover_of_the_union_edges(m, host_run, candidates, union_edges):
    import ref_pipeline
    uniq, edges = union_edges
    kinds = np.bincount(edges["kinds"], minlength=4)
    assert kinds[m.KIND_END] > 0 and kinds[m.KIND_ANY] > 0          # an END-only edge exists at these thresholds
    ab = list(zip(edges["a"].tolist(), edges["b"].tolist()))
    pairs = {(uniq[a], uniq[b]) for a, b in ab}
    deleted = ref_pipeline.vertex_cover(candidates, pairs)
    assert primers_of(host_run[1]) == [w for w in candidates if w not in deleted]
    any_pairs = {(uniq[a], uniq[b]) for (a, b), kd in zip(ab, edges["kinds"].tolist()) if kd & m.KIND_ANY}
    assert ref_pipeline.vertex_cover(candidates, any_pairs) != deleted     # the 3'-end rule changes what is removed
    line = [l for l in host_run[0].splitlines() if l.startswith("Cross-dimer conflicts among")]
    assert line == [f"Cross-dimer conflicts among {len(uniq)} primers (dG < -12000.00 or 3'-end Tm >= 25.00): "
                    f"{kinds[1]} dG only, {kinds[2]} 3'-end only, {kinds[3]} both"]


def test_union_edges_equal_the_oracle(oracle, oracle_tables, union_edges):
    uniq, edges = union_edges
    a, e = M.random_planes(oracle, oracle_tables, uniq, DG, TM)
    np.testing.assert_array_equal(edges, M.kind_edges(a, e))


def test_one_tube_against_the_hosts_rule(fasta, candidates, union_edges, tmp_path):
    uniq, edges = union_edges
    _, csv = run(fasta, tmp_path / "tubes.csv", "--tubes", "1", *RULE)
    host = C.CDLL(str(HOST_LIB))
    text = "\n".join(f"{uniq[a]},{uniq[b]}" for a, b in zip(edges["a"].tolist(), edges["b"].tolist())).encode()
    cap = 32 * len(uniq) + 64
    buf = C.create_string_buffer(cap)
    assert host.odm_assign_tubes("\n".join(uniq).encode(), text, 1, buf, cap) >= 0
    placed = {l.split("\t")[0] for l in buf.value.decode().splitlines() if l.split("\t")[1] != "-"}
    assert primers_of(csv) == [w for w in candidates if w in placed]


def test_select_by_coverage_sees_the_union(m, eng, fasta, tmp_path):
    """One tube: no two kept primers conflict under either rule, and none conflicts with itself."""
    out, csv = run(fasta, tmp_path / "sel_end.csv", "--select-by-coverage", "true", *RULE)
    assert "Cross-dimer conflicts among" in out
    kept = primers_of(csv)
    assert len(kept) > 10 and len(set(kept)) == len(kept)
    _, count = eng.conflict_graph_edges(kept, m.Chem.ntthal(), m.ConflictRule.of(DG, TM))
    assert count == 0


def test_a_threshold_nothing_reaches_changes_nothing(fasta, tmp_path):
    plain = run(fasta, tmp_path / "plain.csv", "--delta-g-threshold", "-12000")
    far = run(fasta, tmp_path / "far.csv", "--delta-g-threshold", "-12000", "--max-cross-dimer-end-tm", "200")
    assert far[1] == plain[1]
    assert "Cross-dimer conflicts among" not in plain[0]
    assert [l for l in far[0].splitlines() if not l.startswith("Cross-dimer conflicts among")] == plain[0].splitlines()


def test_panel_primer_on_a_candidates_3p_tail_drops_the_candidate(oracle, oracle_tables, fasta, candidates, tmp_path):
    uniq = list(dict.fromkeys(candidates))
    pick = None
    for cand in uniq:                              # the panel primer: the reverse complement of the 3' tail, then filler
        panel = (M.rc(cand[-9:]) + "ACAC")[:13]
        if panel in uniq:
            continue
        a1, e1 = M.ab_planes(oracle, oracle_tables, [cand], [panel], DG, TM)
        a2, e2 = M.ab_planes(oracle, oracle_tables, [panel], [cand], DG, TM)
        if (e1[0, 0] or e2[0, 0]) and not a1[0, 0] and not a2[0, 0]:      # an END-only conflict in either role
            pick = (cand, panel)
            break
    assert pick is not None
    cand, panel = pick
    pf = tmp_path / "panel.csv"
    pf.write_text(HEADER + f"F,Primer_0_F,{panel},0.5,40.0,1.0,40.0\n")

    def rejected(*extra):
        rej = tmp_path / "rej.csv"
        _, csv = run(fasta, tmp_path / "out.csv", "--existing-primers", str(pf), "--rejected-out", str(rej), *extra)
        rows = [l.split(",") for l in rej.read_text().splitlines()[1:]]
        return {(r[2], r[4]) for r in rows}, primers_of(csv)

    with_end, kept = rejected(*RULE)
    assert (cand, "panel_dimer") in with_end and cand not in kept
    without, _ = rejected("--delta-g-threshold", "-12000")
    assert (cand, "panel_dimer") not in without


def test_a_value_that_does_not_parse_is_a_usage_error(fasta, tmp_path):
    r = subprocess.run([str(CLI), "-i", str(fasta), "-o", str(tmp_path / "x.csv"), "--do-align", "false",
                        "--max-cross-dimer-end-tm", "warm"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--max-cross-dimer-end-tm" in (r.stderr + r.stdout)
