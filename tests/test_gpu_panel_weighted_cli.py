"""od-msspe-hip --genome-weights on a 10-genome alignment: the CSV and the text block, with its "Weight:" line, of
--thin-panel true and of --select-by-coverage true --tubes 2 against the numpy model (tests/panel_weighted_model.py) fed
what the CLI fed the device; a weights file of all ones changes nothing but that line; and every usage error."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import panel_select_model as sm
import panel_thin_model as tm
import panel_weighted_model as wm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"
LISTED = {"g0": 5, "g1": 0, "g4": 3, "g8": 0, "g9": 7}      # the others weigh --default-genome-weight 2
DEFAULT = 2


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
def case(m, tmp_path_factory):
    g = np.concatenate([m.synth.aligned_genomes(5, 6000, seed=700 + j) for j in range(2)])
    d = tmp_path_factory.mktemp("weighted_cli")
    fa, wf, ones = d / "in.fa", d / "weights.csv", d / "ones.csv"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    wf.write_text("".join(f"{k},{v}\n" for k, v in LISTED.items()))
    ones.write_text("".join(f"g{i},1\n" for i in range(10)))
    P = tm.n_partitions(6000, 500, 250)
    w = np.repeat([LISTED.get(f"g{i}", DEFAULT) for i in range(10)], P)
    return fa, g, wf, ones, w, P


def run_cli(fa, csv, *extra, ok=True):
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                       capture_output=True, text=True, timeout=600)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr
    rows = [l.split(",") for l in Path(csv).read_text().splitlines()[1:] if l]
    return r.stdout, rows


def block_of(out, title, lines):
    at = out.index("\n" + title)
    got = out[at:].split("\n")
    end = lines
    while end < len(got) and got[end].startswith("  Tube "):
        end += 1
    return "".join(l + "\n" for l in got[:end])


def test_thin_panel_with_genome_weights(case, tmp_path):
    fa, g, wf, ones, w, P = case
    _, base = run_cli(fa, tmp_path / "a.csv")
    weighted = ("--thin-panel", "true", "--thin-mismatches", "2", "--genome-weights", str(wf),
                "--default-genome-weight", str(DEFAULT))
    out, rows = run_cli(fa, tmp_path / "b.csv", *weighted)
    fwd = [r[2] for r in base if r[0] == "F"]
    rev = [r[2] for r in base if r[0] == "R"]
    I = tm.incidence(g, 500, 250, 50, 13, fwd, rev, 2, 3)
    want = wm.greedy_weighted(I, w)
    keep = want["keep"]
    kf = [x for x, q in zip(fwd, keep[:len(fwd)]) if q]
    kr = [x for x, q in zip(rev, keep[len(fwd):]) if q]
    assert [r[2] for r in rows if r[0] == "F"] == kf and [r[2] for r in rows if r[0] == "R"] == kr and kf + kr
    block = tm.render_block(2, 3, 1, len(kf), len(fwd), len(kr), len(rev), 0, want["covered_all"],
                            want["covered_kept"], 10 * P)
    line = wm.weight_line(want["weight_all"], want["weight_kept"], int(w.sum()), len(fwd) + len(rev), len(kf) + len(kr))
    assert block_of(out, "Panel thinning", 5) == wm.with_weight_line(block, line)
    assert want["weight_kept"] == want["weight_all"]
    # min_gain is in weight units
    out5, rows5 = run_cli(fa, tmp_path / "c.csv", *weighted, "--thin-min-gain", "5")
    want5 = wm.greedy_weighted(I, w, 5)
    assert len(rows5) == int(want5["keep"].sum()) and "gain >= 5" in out5
    assert wm.weight_line(want5["weight_all"], want5["weight_kept"], int(w.sum()), len(fwd) + len(rev), len(rows5)) in out5


def test_all_ones_change_nothing_but_the_weight_line(case, tmp_path):
    fa, g, wf, ones, w, P = case
    for switch in (("--thin-panel", "true"), ("--select-by-coverage", "true", "--tubes", "2")):
        plain, rows = run_cli(fa, tmp_path / "p.csv", *switch, "--thin-mismatches", "2")
        csv = (tmp_path / "p.csv").read_bytes()
        got, rows1 = run_cli(fa, tmp_path / "q.csv", *switch, "--thin-mismatches", "2", "--genome-weights", str(ones))
        assert (tmp_path / "q.csv").read_bytes() == csv
        assert "  Weight:" not in plain
        kept = [l for l in got.splitlines(keepends=True) if not l.startswith("  Weight:")]
        assert "".join(kept) == plain and len(kept) + 1 == len(got.splitlines())
        lines = got.splitlines()
        at = next(i for i, l in enumerate(lines) if l.startswith("  Weight:"))
        seg, wl = lines[at - 1], lines[at]              # the block's own "Segments:" line stands right before it
        assert seg.startswith("  Segments:")
        assert wl.split("covered ", 1)[1] == seg.split("covered ", 1)[1]   # at weight 1 the weights are the counts


def test_select_by_coverage_with_genome_weights_and_tubes(m, eng, case, tmp_path):
    fa, g, wf, ones, w, P = case
    rej = tmp_path / "rej.csv"
    extra = ("--tubes", "2")
    out, rows = run_cli(fa, tmp_path / "b.csv", *extra, "--select-by-coverage", "true", "--thin-mismatches", "2",
                        "--rejected-out", str(rej), "--genome-weights", str(wf), "--default-genome-weight", str(DEFAULT))
    dropped = [l.split(",") for l in rej.read_text().splitlines()[1:] if l]
    sel_drop = {r[2]: r[4] for r in dropped if r[4].startswith("select_")}
    _, every = run_cli(fa, tmp_path / "all.csv", *extra, "--keep-all", "true")   # the offered lists in stage B's order
    kept_words = {r[2] for r in rows}
    fwd = [r[2] for r in every if r[0] == "F" and (r[2] in kept_words or r[2] in sel_drop)]
    rev = [r[2] for r in every if r[0] == "R" and (r[2] in kept_words or r[2] in sel_drop)]
    assert len(fwd) + len(rev) == len(rows) + len(sel_drop)
    pool = fwd + rev
    B = sm.unpack_bitmap(eng.cross_dimer(pool, m.Chem.ntthal(), -9000.0, want_dg=False)["bitmap"], len(pool))
    I = tm.incidence(g, 500, 250, 50, 13, fwd, rev, 2, 3)
    want = wm.select_weighted(I, B, w, 2)
    keep, tube = want["keep"], want["tube"]
    kf = [x for x, q in zip(fwd, keep[:len(fwd)]) if q]
    kr = [x for x, q in zip(rev, keep[len(fwd):]) if q]
    assert [r[2] for r in rows if r[0] == "F"] == kf and [r[2] for r in rows if r[0] == "R"] == kr and kf + kr
    of = {x: int(t) for x, t in zip(pool, tube)}
    assert [int(r[7]) for r in rows] == [of[r[2]] + 1 for r in rows]
    for x, q, b in zip(pool, keep, want["barred"]):
        assert (x in sel_drop) == (not q)
        if not q:
            assert sel_drop[x] == ("select_conflict" if b else "select_unneeded"), x
    per_tube = [int((tube[keep != 0] == t).sum()) for t in range(want["tubes_used"])]
    block = sm.render_block(0, 0.0, 2, 3, 1, 2, len(kf), len(fwd), len(kr), len(rev), 0, int(want["barred"].sum()),
                            want["covered_all"], want["covered_kept"], 10 * P, per_tube)
    line = wm.weight_line(want["weight_all"], want["weight_kept"], int(w.sum()), len(pool), len(kf) + len(kr))
    assert block_of(out, "Panel selection by coverage", 7) == wm.with_weight_line(block, line)


def test_usage_errors(case, tmp_path):
    fa, g, wf, ones, w, P = case

    def fails(text, *extra, switch=("--thin-panel", "true"), words=()):
        bad = tmp_path / "bad.csv"
        if text is not None:
            bad.write_text(text)
        r = run_cli(fa, tmp_path / "x.csv", *switch, "--genome-weights", str(bad), *extra, ok=False)
        assert r.returncode == 2 and "--genome-weights" in r.stderr, r.stderr
        for word in words:
            assert word in r.stderr, (word, r.stderr)

    fails("g0,1\nnobody,2\n", words=("line 2", "nobody"))                     # a name no record carries
    fails("g0,1\ng1\n", words=("line 2",))                                     # malformed lines
    fails("g0,1\n\ng1,-3\n", words=("line 3",))
    fails("g0,1.5\n", words=("line 1",))
    fails("g0,4294967296\n", words=("line 1",))
    fails("g0,1\ng1,4294967295\n", words=("line 2", "4294967295"))           # the total: P segments per record
    fails("g0,1\n", "--default-genome-weight", "300000000", words=("--default-genome-weight",))
    (tmp_path / "bad.csv").unlink()
    fails(None, words=("cannot read",))
    for switch in (("--select-by-coverage", "true"),):
        fails("g0,1\nnobody,2\n", switch=switch, words=("line 2",))
    # the combinations
    r = run_cli(fa, tmp_path / "x.csv", "--genome-weights", str(wf), ok=False)
    assert r.returncode == 2 and "does nothing" in r.stderr
    for extra in (("--thin-panel", "true", "--thin-depth", "2"), ("--select-by-coverage", "true", "--select-depth", "2"),
                  ("--thin-panel", "true", "--thin-tm", "30")):
        r = run_cli(fa, tmp_path / "x.csv", "--genome-weights", str(wf), *extra, ok=False)
        assert r.returncode == 2 and "not built yet" in r.stderr, extra
    # a name that several records carry applies to all of them; a name listed twice: the later line holds
    twin = tmp_path / "twin.fa"
    twin.write_text("".join(f">{'same' if i < 2 else 'g%d' % i} x\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    lst = tmp_path / "twin.csv"
    lst.write_text("same,4\ng5,9\ng5,0\n")
    out, _ = run_cli(twin, tmp_path / "t.csv", "--thin-panel", "true", "--genome-weights", str(lst))
    total = (2 * 4 + 0 + 7 * 1) * P
    assert any(l.startswith("  Weight:") and l.count(f"/{total} ") == 2 for l in out.splitlines()), out
