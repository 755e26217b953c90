"""msspe_panel_thin_depth* and msspe_panel_thin_thal_depth* on the device against the numpy model
(tests/panel_thin_depth_model.py): keep, order, gains, both depth planes, the four counts and the rounds, exactly.  The
grid in the three forms at R = 2 and 3 with the guarantee through the existing coverage call, R = 1 against
Engine.panel_thin / panel_thin_thal, every group boundary and n_pad edge, saturation over 17 batches of rounds, forced
representatives and shadows, min_gain above 1, the empty inputs, the matrix cap, the depth's range, the thal forms
against the held incidence, the context's shared buffers, and the CLI's --thin-depth."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import coverage_thal_model as ctm
import panel_thin_depth_model as dm
import panel_thin_model as tm
import panel_thin_thal_model as ttm
from test_coverage_mm_model import draw_primers, rc
from test_panel_thin_model import GRID, grid_case

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


def primer_sets(rng, g, n, k):
    return draw_primers(rng, g, n, k), [rc(w) for w in draw_primers(rng, g, n, k)]


def equal(got, want, what=""):
    """An Engine.panel_thin_depth tuple against panel_thin_depth_model.greedy_depth's."""
    keep, order, gains, d_all, d_kept, counts = want[:6]
    np.testing.assert_array_equal(got[1], order, what)
    np.testing.assert_array_equal(got[2], gains, what)
    np.testing.assert_array_equal(got[0], keep, what)
    np.testing.assert_array_equal(got[3].reshape(-1), d_all, what)
    np.testing.assert_array_equal(got[4].reshape(-1), d_kept, what)
    np.testing.assert_array_equal(got[5], counts, what)


def check(eng, g, opt, fwd, rev, M, E, depth, min_gain=1, forced=None, forms=("host",), I=None):
    """The device result of every form against the model; returns (I, the model's result)."""
    if I is None:
        I = tm.incidence(g, opt.segment_size, opt.overlap_size, opt.search_window_size, opt.kmer_size, fwd, rev, M, E)
    sh = dm.shadows(fwd, rev, forced)
    want = dm.greedy_depth(I, depth, min_gain, forced, sh)
    for form in forms:
        equal(eng.panel_thin_depth(g, opt, fwd, rev, M, E, depth, min_gain, forced, form), want, form)
        if I.size:
            assert eng.info("panel_thin_rounds") == want[6]
            assert eng.info("panel_thin_depth_shadows") == int(sh.sum())
    if min_gain == 1:
        assert (want[4].astype(int) >= np.minimum(depth, want[3].astype(int))).all()
        assert want[5][1] == want[5][0] and want[5][3] == want[5][2]
    return I, want


@pytest.fixture(scope="module")
def grid_incidence():
    """The grid's inputs and incidence, computed once and shared."""
    out = {}
    for k, M, _ in GRID:
        g, fwd, rev = grid_case(k, M)
        out[k, M] = (g, fwd, rev, tm.incidence(g, 400, 170, 50, k, fwd, rev, M, 3))
    return out


@pytest.mark.parametrize("k,M,picks", GRID)
def test_grid_in_the_three_forms_and_the_guarantee(m, eng, grid_incidence, k, M, picks):
    g, fwd, rev, I = grid_incidence[k, M]
    opt = m.KmerOpt(400, 170, 50, k, 0, 0)
    _, counts = eng.segment_coverage_mm(g, opt, fwd, rev, M, 3, per_primer=True)
    np.testing.assert_array_equal(counts, I.sum(axis=1))          # the row sums of the matrix the rounds read
    assert not dm.shadows(fwd, rev).any()
    for R in (2, 3):
        _, want = check(eng, g, opt, fwd, rev, M, 3, R, forms=("host", "dev", "packed"), I=I)
        keep = want[0]
        assert len(want[1]) >= picks
        # the guarantee through the existing call: per segment, the kept primers that match it, one call per primer
        # would be the direct way; the kept subset's row sums tie the call to I, and I's columns give the depths
        kf = [w for w, q in zip(fwd, keep[:len(fwd)]) if q]
        kr = [w for w, q in zip(rev, keep[len(fwd):]) if q]
        best, kept_counts = eng.segment_coverage_mm(g, opt, kf, kr, M, 3, per_primer=True)
        np.testing.assert_array_equal(kept_counts, I[keep != 0].sum(axis=1))
        d_kept, d_all = I[keep != 0].sum(axis=0), I.sum(axis=0)
        assert (d_kept >= np.minimum(R, d_all)).all()
        np.testing.assert_array_equal(best.reshape(-1) != 255, d_kept >= 1)
    assert eng.info("panel_thin_groups") == -(-130 // 53)


NF = 69   # forward primers of duplicate_pool


def duplicate_pool(fwd, rev):
    """The (13, 2) grid pool (65 + 65) with words listed twice and three times in a direction -- of primers that do
    match segments --, a word in both directions, and forced flags on a later duplicate, on two duplicates, and on an
    unrelated primer."""
    fwd = fwd + [fwd[19], fwd[25], fwd[19], rev[40]]    # 65, 66, 67 repeat 19, 25, 19; 68 is a reverse word
    rev = rev + [rev[50], rev[24], rev[50]]             # NF + 65, 66, 67 repeat reverse 50, 24, 50
    assert len(fwd) == NF and len(rev) == 68
    forced = np.zeros(NF + 68, dtype=np.uint8)
    forced[[66, 4]] = 1                                 # a forced duplicate of the lower unforced 25
    forced[[NF + 65, NF + 67]] = 1                      # two forced duplicates of the unforced reverse 50
    return fwd, rev, forced


def test_depth_one_is_the_plain_thinning(m, eng, grid_incidence):
    for k, M, _ in GRID:
        g, fwd, rev, _ = grid_incidence[k, M]
        opt = m.KmerOpt(400, 170, 50, k, 0, 0)
        a = eng.panel_thin(g, opt, fwd, rev, M, 3)
        rounds = eng.info("panel_thin_rounds")
        b = eng.panel_thin_depth(g, opt, fwd, rev, M, 3, 1)
        for i in range(3):
            np.testing.assert_array_equal(a[i], b[i])
        assert eng.info("panel_thin_rounds") == rounds and (b[5][0], b[5][1]) == (a[4], a[5])
        np.testing.assert_array_equal(b[4] >= 1, a[3] == 1)
    g, fwd, rev, _ = grid_incidence[13, 2]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    fwd, rev, forced = duplicate_pool(fwd, rev)
    for f in (None, forced):
        for G in (1, 2):
            for form in ("host", "packed"):
                a = eng.panel_thin(g, opt, fwd, rev, 2, 3, G, f, form)
                rounds = eng.info("panel_thin_rounds")
                b = eng.panel_thin_depth(g, opt, fwd, rev, 2, 3, 1, G, f, form)
                for i in range(3):
                    np.testing.assert_array_equal(a[i], b[i])
                assert eng.info("panel_thin_rounds") == rounds and (b[5][0], b[5][1]) == (a[4], a[5])
        assert eng.info("panel_thin_depth_shadows") == int(dm.shadows(fwd, rev, f).sum()) == 6


def test_shadows_and_forced_representatives(m, eng, grid_incidence):
    g, fwd, rev, _ = grid_incidence[13, 2]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    fwd, rev, forced = duplicate_pool(fwd, rev)
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    n = len(fwd) + len(rev)
    assert I[65].sum() == I[19].sum() == 10 and I[NF + 65].sum() == I[NF + 50].sum() == 10
    for R in (2, 3):
        _, free = check(eng, g, opt, fwd, rev, 2, 3, R, forms=("host", "packed"), I=I)
        sh = dm.shadows(fwd, rev)
        assert sh.sum() == 6 and not sh[68] and not free[0][sh != 0].any()          # never picked
        _, want = check(eng, g, opt, fwd, rev, 2, 3, R, forced=forced, forms=("host", "dev"), I=I)
        shf = dm.shadows(fwd, rev, forced)
        assert shf[25] == 1 and shf[66] == 0 and shf[NF + 50] == 1 and shf[NF + 65] == 0 and shf[NF + 67] == 1
        np.testing.assert_array_equal(want[0][shf != 0], forced[shf != 0])          # a shadow's keep: its forced flag
        assert want[0][NF + 67] == 1 and want[0][25] == 0 and want[7].sum() > 0     # forced representatives count
        # forced representatives count first: the first picks forced, the rest goes on from there
        some = np.zeros(n, dtype=np.uint8)
        some[free[1][:3]] = 1
        _, after = check(eng, g, opt, fwd, rev, 2, 3, R, forced=some, I=I)
        assert after[7].sum() > 0 and not set(after[1].tolist()) & set(free[1][:3].tolist())
        every = np.ones(n, dtype=np.uint8)                                          # everything forced
        _, want = check(eng, g, opt, fwd, rev, 2, 3, R, forced=every, I=I)
        assert want[1].size == 0 and want[0].all() and (want[3] == want[4]).all()
    # the duplicates do not pass for redundancy: depth_all is the distinct words' column sum
    got = eng.panel_thin_depth(g, opt, fwd, rev, 2, 3, 2)
    np.testing.assert_array_equal(got[3].reshape(-1), I[dm.shadows(fwd, rev) == 0].sum(axis=0))


@pytest.mark.parametrize("n_seq,L,n_seg", [(1, 400, 1), (4, 2440, 52), (53, 450, 53), (6, 1760, 54), (107, 500, 107),
                                           (10, 2950, 160)])
def test_group_boundaries(m, eng, n_seq, L, n_seg):
    """The six shapes of test_gpu_panel_thin.py::test_group_boundaries at R = 2: 53 segments per group."""
    g = m.synth.aligned_genomes(n_seq, L, seed=n_seg)
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    assert n_seq * tm.n_partitions(L, 400, 170) == n_seg
    fwd, rev = primer_sets(np.random.default_rng(n_seg), g, 30, 13)
    check(eng, g, opt, fwd, rev, 2, 3, 2, forms=("host", "packed"))
    assert eng.info("panel_thin_groups") == -(-n_seg // 53)


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_primer_counts_around_the_row_padding(m, eng, n):
    g = m.synth.aligned_genomes(6, 1760, seed=n)
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    rng = np.random.default_rng(n)
    fwd = draw_primers(rng, g, n // 2, 13, random_extra=0)
    rev = [rc(w) for w in draw_primers(rng, g, n - n // 2, 13, random_extra=0)]
    assert len(fwd) + len(rev) == n
    forced = np.zeros(n, dtype=np.uint8)
    forced[[0, n - 1]] = 1
    check(eng, g, opt, fwd, rev, 2, 3, 2)
    check(eng, g, opt, fwd, rev, 2, 3, 3, forced=forced, forms=("packed",))


def test_saturation_and_many_rounds(m, eng):
    """300 distinct 5-mers at M = 5, E = 0: every primer matches every window, so every count is 300."""
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(1).integers(0, 4, size=(2, 600))].copy()
    words = ["".join("ACGT"[(i >> (2 * j)) & 3] for j in range(5)) for i in range(300)]
    opt = m.KmerOpt(300, 150, 40, 5, 0, 0)
    n_seg = 2 * tm.n_partitions(600, 300, 150)
    keep, order, gains, d_all, d_kept, counts = eng.panel_thin_depth(g, opt, words[:150], words[150:], 5, 0, 255)
    assert order.tolist() == list(range(255)) and gains.tolist() == [n_seg] * 255
    assert (d_all == 255).all() and (d_kept == 255).all() and d_all.size == n_seg   # 300 saturates, 255 kept
    assert counts.tolist() == [n_seg] * 4 and keep.tolist() == [1] * 255 + [0] * 45
    assert eng.info("panel_thin_rounds") == 256                                      # 16 batches of 16 and a 17th
    I = np.ones((300, n_seg), dtype=bool)
    equal((keep, order, gains, d_all, d_kept, counts), dm.greedy_depth(I, 255))


@pytest.mark.parametrize("min_gain", [2, 5])
def test_min_gain(m, eng, grid_incidence, min_gain):
    g, fwd, rev, I = grid_incidence[13, 2]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    _, want = check(eng, g, opt, fwd, rev, 2, 3, 2, min_gain, forms=("host", "packed"), I=I)
    assert (want[2] >= min_gain).all() and len(want[1]) < 16
    rng = np.random.default_rng(min_gain)
    check(eng, g, opt, fwd, rev, 2, 3, 3, min_gain, rng.random(I.shape[0]) < 0.06, I=I)


def test_empty_inputs(m, eng):
    g = m.synth.aligned_genomes(5, 1500, seed=3)
    fwd, rev = primer_sets(np.random.default_rng(3), g, 20, 13)
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    for f, r in (([], []), (fwd, []), ([], rev)):
        check(eng, g, opt, f, r, 2, 3, 2, forms=("host", "dev", "packed"))
    n = len(fwd) + len(rev)
    forced = np.zeros(n, dtype=np.uint8)
    forced[[1, n - 1]] = 1
    got = eng.panel_thin_depth(g, m.KmerOpt(2000, 170, 50, 13, 0, 0), fwd, rev, 2, 3, 2, forced=forced)   # no segment
    assert got[0].tolist() == forced.tolist() and got[1].size == 0 and got[3].shape == (5, 0) == got[4].shape
    assert got[5].tolist() == [0, 0, 0, 0]
    gaps = np.full((4, 1500), ord("-"), dtype=np.uint8)
    _, want = check(eng, gaps, opt, fwd, rev, 2, 3, 2, forced=forced)
    assert want[1].size == 0 and want[5].tolist() == [0, 0, 0, 0]


def test_matrix_cap_and_the_depth_range(m, eng):
    g = m.synth.aligned_genomes(40, 6000, seed=9)
    opt = m.KmerOpt(400, 60, 50, 13, 0, 0)
    fwd, rev = primer_sets(np.random.default_rng(9), g, 995, 13)   # 71 groups x 2,048 words, 1.16 MB
    default = eng.info("panel_thin_matrix_max_mb")
    eng.set_option("panel_thin_matrix_max_mb", 1)
    try:
        with pytest.raises(m.MsspeError) as e:
            eng.panel_thin_depth(g, opt, fwd, rev, 1, 3, 2)
        assert e.value.code == 5 and "needs 2 MB" in str(e.value) and "panel_thin_matrix_max_mb is 1" in str(e.value)
    finally:
        eng.set_option("panel_thin_matrix_max_mb", default)
    small = m.synth.aligned_genomes(2, 1200, seed=1)
    w = ["ACGTACGTACGTA"]
    ok = m.KmerOpt(500, 250, 50, 13, 0, 0)
    chem = m.Chem.ntthal()
    for bad in (0, 256, -1):
        for form in ("host", "dev", "packed"):
            with pytest.raises(m.MsspeError) as e:
                eng.panel_thin_depth(small, ok, w, w, 1, 3, bad, form=form)
            assert e.value.code == 1 and "depth" in str(e.value)
            with pytest.raises(m.MsspeError) as e:
                eng.panel_thin_thal_depth(small, ok, w, w, 1, 3, chem, "end1", 30.0, bad, form=form)
            assert e.value.code == 1 and "depth" in str(e.value)
    with pytest.raises(m.MsspeError) as e:
        eng.panel_thin_depth(small, ok, w, w, 1, 3, 2, min_gain=0)
    assert e.value.code == 1
    for R in (1, 255):                                             # the ends of the range are taken
        assert eng.panel_thin_depth(small, ok, w, w, 1, 3, R)[0].shape == (2,)


@pytest.mark.parametrize("thr", [30.0, -5.0])
def test_thal_forms_on_the_held_incidence(m, eng, oracle, oracle_tables, thr):
    """END1 on the grid of test_gpu_panel_thin_thal.py; at a threshold <= 0 the held incidence is the string rule's."""
    g = m.synth.aligned_genomes(10, 2600, seed=53)
    fwd, rev = primer_sets(np.random.default_rng(1302), g, 60, 13)
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    chem = m.Chem.ntthal()
    I = tm.incidence(g, 400, 170, 50, 13, fwd, rev, 2, 3)
    if thr > 0:
        res = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, 13, fwd, rev, 2, 3, "end1", thr, oracle.ntthal_args())
        H = ttm.held_incidence(res)
        assert H.sum() < I.sum() and not (H & ~I).any()
    else:
        H = I
    n = len(fwd) + len(rev)
    forced = np.zeros(n, dtype=np.uint8)
    forced[[4, n - 3]] = 1
    a = eng.panel_thin_thal(g, opt, fwd, rev, 2, 3, chem, "end1", thr)
    rounds = eng.info("panel_thin_rounds")
    b = eng.panel_thin_thal_depth(g, opt, fwd, rev, 2, 3, chem, "end1", thr, 1)
    for i in range(3):
        np.testing.assert_array_equal(a[i], b[i])
    assert eng.info("panel_thin_rounds") == rounds
    for R in (2, 3):
        for f in (None, forced):
            want = dm.greedy_depth(H, R, 1, f, dm.shadows(fwd, rev, f))
            for form in ("host", "dev", "packed"):
                equal(eng.panel_thin_thal_depth(g, opt, fwd, rev, 2, 3, chem, "end1", thr, R, forced=f, form=form),
                      want, form)
            assert eng.info("panel_thin_rounds") == want[6]
            assert (want[4].astype(int) >= np.minimum(R, want[3].astype(int))).all()
    equal(eng.panel_thin_thal_depth(g, opt, fwd, rev, 2, 3, chem, "end1", thr, 2, min_gain=2),
          dm.greedy_depth(H, 2, 2))


def test_shared_buffers_with_the_other_calls(m, eng, grid_incidence):
    """A larger depth call, a smaller one on the same context, then the plain thinning with its usual result."""
    g, fwd, rev, I = grid_incidence[13, 2]
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    before = eng.panel_thin(g, opt, fwd, rev, 2, 3)
    check(eng, g, opt, fwd, rev, 2, 3, 3, I=I)
    small = m.synth.aligned_genomes(3, 900, seed=2)
    f2, r2 = primer_sets(np.random.default_rng(2), small, 9, 13)
    check(eng, small, opt, f2, r2, 2, 3, 2, forms=("host", "packed"))
    assert eng.info("panel_thin_groups") == 1 and eng.info("panel_thin_depth_colsum_us") >= 0
    after = eng.panel_thin(g, opt, fwd, rev, 2, 3)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    assert len(after[1]) == 10 and eng.info("panel_thin_rounds") == 11


# ---- the CLI ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_fasta(m, tmp_path_factory):
    """The inputs of test_gpu_panel_thin.py's CLI tests."""
    g = np.concatenate([m.synth.aligned_genomes(20, 6000, seed=700 + j) for j in range(2)])
    fa = tmp_path_factory.mktemp("thin_depth_cli") / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    return fa, g


def run_cli(fa, csv, *extra):
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    text = Path(csv).read_text()
    return r.stdout, [l.split(",") for l in text.splitlines()[1:] if l], text


def block_of(out, lines=5):
    at = out.index("\nPanel thinning")
    return "".join(l + "\n" for l in out[at:].split("\n")[:lines])


@pytest.fixture(scope="module")
def cli_base(small_fasta, tmp_path_factory):
    """The run without thinning (its CSV is the pool the thinning is offered) and the plain thinning's run."""
    fa, g = small_fasta
    d = tmp_path_factory.mktemp("thin_depth_base")
    _, base, _ = run_cli(fa, d / "a.csv")
    plain = run_cli(fa, d / "b.csv", "--thin-panel", "true", "--thin-mismatches", "2")
    return base, plain


def depth_case(fa, g, tmp_path, base, extra, I_of, render, panel=((), ()), R=2):
    out, rows, _ = run_cli(fa, tmp_path / "deep.csv", *extra, "--thin-panel", "true", "--thin-mismatches", "2",
                           "--thin-depth", str(R))
    fwd = [r[2] for r in base if r[0] == "F"]
    rev = [r[2] for r in base if r[0] == "R"]
    all_f, all_r = fwd + list(panel[0]), rev + list(panel[1])
    forced = np.array([0] * len(fwd) + [1] * len(panel[0]) + [0] * len(rev) + [1] * len(panel[1]), dtype=np.uint8)
    keep, order, gains, d_all, d_kept, counts, _, _, _ = dm.greedy_depth(I_of(all_f, all_r), R, 1, forced,
                                                                         dm.shadows(all_f, all_r, forced))
    kf = [w for w, q in zip(fwd, keep[:len(fwd)]) if q]
    kr = [w for w, q in zip(rev, keep[len(all_f):len(all_f) + len(rev)]) if q]
    assert [r[2] for r in rows if r[0] == "F"] == kf and [r[2] for r in rows if r[0] == "R"] == kr
    assert 0 < len(kf) + len(kr) < len(fwd) + len(rev)
    segments = g.shape[0] * tm.n_partitions(g.shape[1], 500, 250)
    first = render(len(kf), len(fwd), len(kr), len(rev), int(forced.sum()), int(counts[0]), int(counts[1]), segments)
    head, rest = first.split("):\n", 1)
    want = head + ", depth %d):\n" % R + rest + dm.render_depth_line(R, int(counts[2]), int(counts[3]), segments,
                                                                    len(fwd) + len(rev), len(kf) + len(kr))
    assert block_of(out) == want
    assert counts[3] == counts[2] > 0
    return rows, out


def test_cli_depth_one_prints_todays_bytes(small_fasta, cli_base, tmp_path):
    fa, g = small_fasta
    _, plain = cli_base
    one = run_cli(fa, tmp_path / "one.csv", "--thin-panel", "true", "--thin-mismatches", "2", "--thin-depth", "1")
    assert one[0] == plain[0] and one[2] == plain[2]
    assert "Depth:" not in one[0] and ", depth" not in one[0]


def test_cli_thins_to_a_depth(small_fasta, cli_base, tmp_path):
    fa, g = small_fasta
    base, plain = cli_base
    rows, out = depth_case(fa, g, tmp_path, base, (), lambda f, r: tm.incidence(g, 500, 250, 50, 13, f, r, 2, 3),
                           lambda *a: tm.render_block(2, 3, 1, *a))
    assert len(rows) >= len(plain[1])                     # depth 2 keeps no fewer than depth 1


def test_cli_with_existing_primers(small_fasta, cli_base, tmp_path):
    fa, g = small_fasta
    first, _ = cli_base
    panel_rows = [r for r in first if r[0] == "F"][:4] + [r for r in first if r[0] == "R"][:4]
    panel = tmp_path / "panel.csv"
    panel.write_text("direction,name,primers,gc,avg,std,tm\n" + "".join(",".join(r) + "\n" for r in panel_rows))
    pf = [r[2] for r in panel_rows if r[0] == "F"]
    pr = [r[2] for r in panel_rows if r[0] == "R"]
    extra = ("--existing-primers", str(panel))
    _, base, _ = run_cli(fa, tmp_path / "a.csv", *extra)
    rows, out = depth_case(fa, g, tmp_path, base, extra, lambda f, r: tm.incidence(g, 500, 250, 50, 13, f, r, 2, 3),
                           lambda *a: tm.render_block(2, 3, 1, *a), (pf, pr))
    assert not {r[2] for r in rows} & set(pf + pr) and ", 8 forced\n" in out


def test_cli_with_thin_tm(oracle, oracle_tables, small_fasta, cli_base, tmp_path):
    fa, g = small_fasta
    base, _ = cli_base

    def held(f, r):
        return ttm.held_incidence(ctm.coverage_thal(oracle_tables, g, 500, 250, 50, 13, f, r, 2, 3, "any", 30.0,
                                                    oracle.ntthal_args()))

    depth_case(fa, g, tmp_path, base, ("--thin-tm", "30"), held,
               lambda *a: ttm.render_block("any", 30.0, 2, 3, 1, *a))
