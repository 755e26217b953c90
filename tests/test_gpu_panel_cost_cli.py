"""od-msspe-hip --primer-costs / --background-site-cost on a 10-genome alignment: the CSV and the text block, with its
"Cost:" line, of --thin-panel true and of --select-by-coverage true --tubes 2 --genome-weights against the model
(tests/panel_cost_model.py) fed what the CLI fed the device; a planted background that makes one of two interchangeable
candidates expensive; a cost file of all ones changes nothing but that line; and every usage error."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import panel_cost_model as cm
import panel_select_model as sm
import panel_thin_model as tm
import panel_weighted_model as wm
from test_coverage_mm_model import rc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"
LISTED = {"g0": 5, "g1": 0, "g4": 3, "g8": 0, "g9": 7}      # genome weights; the others weigh 2
DEFAULT_WEIGHT = 2
DEFAULT_COST = 3


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


def run_cli(fa, csv, *extra, ok=True):
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                       capture_output=True, text=True, timeout=600)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr
    rows = [l.split(",") for l in Path(csv).read_text().splitlines()[1:] if l]
    return r.stdout, rows


def listed_cost(i):
    return 1 + (7 * i) % 5


@pytest.fixture(scope="module")
def case(m, tmp_path_factory):
    """The alignment, its files, the final lists of a plain run and every candidate of a --keep-all run with --tubes 2
    (the selection's offered lists), and a cost file that lists every second word of both."""
    g = np.concatenate([m.synth.aligned_genomes(5, 6000, seed=700 + j) for j in range(2)])
    d = tmp_path_factory.mktemp("cost_cli")
    fa, wf, cf, ones = d / "in.fa", d / "weights.csv", d / "costs.csv", d / "ones.csv"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    wf.write_text("".join(f"{k},{v}\n" for k, v in LISTED.items()))
    _, base = run_cli(fa, d / "base.csv")
    _, every = run_cli(fa, d / "all.csv", "--tubes", "2", "--keep-all", "true")
    words = list(dict.fromkeys([r[2] for r in base] + [r[2] for r in every]))
    costs = {x: listed_cost(i) for i, x in enumerate(words) if i % 2 == 0}
    first = next(iter(costs))
    cf.write_text(f"{first},4000000000\n\n" + "".join(f"{x},{c}\r\n" for x, c in costs.items()))   # the later line holds
    ones.write_text("".join(f"{x},1\n" for x in words))
    P = tm.n_partitions(6000, 500, 250)
    w = np.repeat([LISTED.get(f"g{i}", DEFAULT_WEIGHT) for i in range(10)], P)
    return {"fa": fa, "g": g, "wf": wf, "cf": cf, "ones": ones, "w": w, "P": P, "base": base, "every": every,
            "costs": costs}


def block_of(out, title, lines):
    at = out.index("\n" + title)
    got = out[at:].split("\n")
    end = lines
    while end < len(got) and got[end].startswith("  Tube "):
        end += 1
    return "".join(l + "\n" for l in got[:end])


def test_thin_panel_with_primer_costs(case, tmp_path):
    fa, g, P = case["fa"], case["g"], case["P"]
    out, rows = run_cli(fa, tmp_path / "b.csv", "--thin-panel", "true", "--thin-mismatches", "2", "--primer-costs",
                        str(case["cf"]), "--default-primer-cost", str(DEFAULT_COST))
    fwd = [r[2] for r in case["base"] if r[0] == "F"]
    rev = [r[2] for r in case["base"] if r[0] == "R"]
    I = tm.incidence(g, 500, 250, 50, 13, fwd, rev, 2, 3)
    costs = [case["costs"].get(x, DEFAULT_COST) for x in fwd + rev]
    want = cm.greedy_cost(I, costs)
    keep = want["keep"]
    kf = [x for x, q in zip(fwd, keep[:len(fwd)]) if q]
    kr = [x for x, q in zip(rev, keep[len(fwd):]) if q]
    assert [r[2] for r in rows if r[0] == "F"] == kf and [r[2] for r in rows if r[0] == "R"] == kr and kf + kr
    assert keep.tolist() != tm.greedy(I)[0].tolist()                     # the costs change the kept set here
    block = tm.render_block(2, 3, 1, len(kf), len(fwd), len(kr), len(rev), 0, want["covered_all"],
                            want["covered_kept"], 10 * P)
    line = cm.cost_line(want["cost_kept"], want["cost_all"], len(kf) + len(kr), len(fwd) + len(rev))
    assert block_of(out, "Panel thinning", 5) == cm.with_cost_line(block, line)
    assert want["covered_kept"] == want["covered_all"]


def test_select_by_coverage_with_costs_weights_and_tubes(m, eng, case, tmp_path):
    fa, g, P, w = case["fa"], case["g"], case["P"], case["w"]
    rej = tmp_path / "rej.csv"
    out, rows = run_cli(fa, tmp_path / "b.csv", "--tubes", "2", "--select-by-coverage", "true", "--thin-mismatches", "2",
                        "--rejected-out", str(rej), "--genome-weights", str(case["wf"]), "--default-genome-weight",
                        str(DEFAULT_WEIGHT), "--primer-costs", str(case["cf"]), "--default-primer-cost",
                        str(DEFAULT_COST))
    dropped = [l.split(",") for l in rej.read_text().splitlines()[1:] if l]
    sel_drop = {r[2]: r[4] for r in dropped if r[4].startswith("select_")}
    kept_words = {r[2] for r in rows}
    fwd = [r[2] for r in case["every"] if r[0] == "F" and (r[2] in kept_words or r[2] in sel_drop)]
    rev = [r[2] for r in case["every"] if r[0] == "R" and (r[2] in kept_words or r[2] in sel_drop)]
    assert len(fwd) + len(rev) == len(rows) + len(sel_drop)
    pool = fwd + rev
    B = sm.unpack_bitmap(eng.cross_dimer(pool, m.Chem.ntthal(), -9000.0, want_dg=False)["bitmap"], len(pool))
    I = tm.incidence(g, 500, 250, 50, 13, fwd, rev, 2, 3)
    costs = [case["costs"].get(x, DEFAULT_COST) for x in pool]
    want = cm.select_cost(I, B, costs, w, 2)
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
    weight = wm.weight_line(want["weight_all"], want["weight_kept"], int(w.sum()), len(pool), len(kf) + len(kr))
    line = cm.cost_line(want["cost_kept"], want["cost_all"], len(kf) + len(kr), len(pool))
    assert block_of(out, "Panel selection by coverage", 8) == cm.with_cost_line(block, line, weight)


def test_background_sites_make_a_candidate_expensive(case, tmp_path):
    """Of two interchangeable candidates the one with background sites goes and the clean one is kept.  The background
    holds exact copies of one primer (three on the forward strand, two on the reverse) between random bases, and is
    searched without mismatches, so the counts are what a text search gives."""
    fa, g, P = case["fa"], case["g"], case["P"]
    fwd = [r[2] for r in case["base"] if r[0] == "F"]
    rev = [r[2] for r in case["base"] if r[0] == "R"]
    pool = fwd + rev
    I = tm.incidence(g, 500, 250, 50, 13, fwd, rev, 2, 3)
    plain = tm.greedy(I)[0]
    site_cost, sites = 1000, 5
    q = None
    for p in np.flatnonzero(plain):                     # a kept primer that the others can stand in for
        costs = [1] * len(pool)
        costs[p] = 1 + site_cost * sites
        want = cm.greedy_cost(I, costs)
        if not want["keep"][p]:
            q = int(p)
            break
    assert q is not None, "no kept primer of this case has a stand-in"
    rng = np.random.default_rng(11)
    junk = lambda n: bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)]).decode()
    word = pool[q]
    bg_seq = junk(40) + word + junk(31) + word + junk(17) + rc(word) + junk(23) + word + junk(9) + rc(word) + junk(40)
    count = lambda x: sum(bg_seq.startswith(y, i) for y in {x, rc(x)} for i in range(len(bg_seq)))
    assert [count(x) for x in pool] == [sites if i == q else 0 for i in range(len(pool))]
    bg = tmp_path / "bg.fa"
    bg.write_text(f">host\n{bg_seq}\n")
    out, rows = run_cli(fa, tmp_path / "b.csv", "--thin-panel", "true", "--thin-mismatches", "2", "--background", str(bg),
                        "--background-mismatches", "0", "--background-site-cost", str(site_cost))
    kept = [r[2] for r in rows]
    assert kept == [x for x, k in zip(pool, want["keep"]) if k]
    assert word not in kept and set(kept) - {x for x, k in zip(pool, plain) if k}    # the clean stand-in is kept
    assert cm.cost_line(want["cost_kept"], want["cost_all"], len(kept), len(pool)) in out
    assert want["cost_kept"] == len(kept) and want["cost_all"] == len(pool) + site_cost * sites
    assert want["covered_kept"] == want["covered_all"]


def test_all_ones_change_nothing_but_the_cost_line(case, tmp_path):
    fa = case["fa"]
    for switch in (("--thin-panel", "true"), ("--select-by-coverage", "true", "--tubes", "2")):
        plain, _ = run_cli(fa, tmp_path / "p.csv", *switch, "--thin-mismatches", "2")
        csv = (tmp_path / "p.csv").read_bytes()
        got, _ = run_cli(fa, tmp_path / "q.csv", *switch, "--thin-mismatches", "2", "--primer-costs", str(case["ones"]))
        assert (tmp_path / "q.csv").read_bytes() == csv
        assert "  Cost:" not in plain
        kept = [l for l in got.splitlines(keepends=True) if not l.startswith("  Cost:")]
        assert "".join(kept) == plain and len(kept) + 1 == len(got.splitlines())
        lines = got.splitlines()
        at = next(i for i, l in enumerate(lines) if l.startswith("  Cost:"))
        assert lines[at - 1].startswith("  Segments:")
        k, n = lines[at].split()[1].split("/")
        assert lines[at] == f"  Cost:     {k}/{n} by the kept {k} of {n}"   # at cost 1 the costs are the numbers


def test_usage_errors(case, tmp_path):
    fa = case["fa"]
    word = case["base"][0][2]

    def fails(text, *extra, switch=("--thin-panel", "true"), words=()):
        bad = tmp_path / "bad.csv"
        if text is not None:
            bad.write_text(text)
        r = run_cli(fa, tmp_path / "x.csv", *switch, "--primer-costs", str(bad), *extra, ok=False)
        assert r.returncode == 2 and "--primer-costs" in r.stderr, r.stderr
        for w in words:
            assert w in r.stderr, (w, r.stderr)

    fails(f"{word},1\n{word}\n", words=("line 2",))                            # malformed lines
    fails(f"{word},1\n\n{word},0\n", words=("line 3",))
    fails(f"{word},-3\n", words=("line 1",))
    fails(f"{word},1.5\n", words=("line 1",))
    fails(f"{word},4294967296\n", words=("line 1", "4294967295"))
    fails(f"{word},2\n{word[:-1]},2\n", words=("line 2", "--kmer-size"))       # not kmer_size bases
    fails(f"{word[:-1]}N,2\n", words=("line 1",))
    fails(f"{word},2,3\n", words=("line 1",))
    fails(f"{word},2\nACGT\n", switch=("--select-by-coverage", "true"), words=("line 2",))
    (tmp_path / "bad.csv").unlink()
    fails(None, words=("cannot read",))
    # the combinations
    good = tmp_path / "good.csv"
    good.write_text(f"{word},2\n")
    bg = tmp_path / "bg.fa"
    bg.write_text(">host\nACGTACGTACGTACGTACGTACGTACGT\n")
    for cost in (("--primer-costs", str(good)), ("--background", str(bg), "--background-site-cost", "2")):
        r = run_cli(fa, tmp_path / "x.csv", *cost, ok=False)
        assert r.returncode == 2 and "nothing without" in r.stderr
        for extra in (("--thin-panel", "true", "--thin-depth", "2"),
                      ("--select-by-coverage", "true", "--select-depth", "2"),
                      ("--thin-panel", "true", "--thin-tm", "30")):
            r = run_cli(fa, tmp_path / "x.csv", *cost, *extra, ok=False)
            assert r.returncode == 2 and "not built yet" in r.stderr and "--primer-costs" in r.stderr, extra
        r = run_cli(fa, tmp_path / "x.csv", *cost, "--devices", "0", ok=False)
        assert r.returncode == 2 and "--devices" in r.stderr and "--background-site-cost" in r.stderr
    r = run_cli(fa, tmp_path / "x.csv", "--thin-panel", "true", "--background-site-cost", "2", ok=False)
    assert r.returncode == 2 and "needs '--background <FASTA>'" in r.stderr
    r = run_cli(fa, tmp_path / "x.csv", "--thin-panel", "true", "--primer-costs", str(good), "--default-primer-cost", "0",
                ok=False)
    assert r.returncode == 2 and "--default-primer-cost" in r.stderr
