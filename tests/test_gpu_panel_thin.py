"""msspe_panel_thin* on the device against the numpy model (tests/panel_thin_model.py): order, gains, keep, covered
and both counts, exactly.  The grid inputs in the three entry-point forms and the guarantee through the existing
coverage call, every group boundary, both word widths, short and long windows, more primers than one LDS tile, ties,
forced primers, min_gain above 1, the empty inputs, more than two batches of rounds, the matrix cap, the argument
errors, and the CLI's --thin-panel on its own, with --existing-primers and with --tubes."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import panel_thin_model as tm
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


def check(eng, g, opt, fwd, rev, M, E, min_gain=1, forced=None, forms=("host",), chunk=64):
    """The device result of every form against the model; returns (I, the model's result)."""
    I = tm.incidence(g, opt.segment_size, opt.overlap_size, opt.search_window_size, opt.kmer_size, fwd, rev, M, E, chunk)
    want = tm.greedy(I, min_gain, forced)
    keep, order, gains, covered, c_all, c_kept, rounds = want
    for form in forms:
        got = eng.panel_thin(g, opt, fwd, rev, M, E, min_gain, forced, form)
        np.testing.assert_array_equal(got[1], order, form)
        np.testing.assert_array_equal(got[2], gains, form)
        np.testing.assert_array_equal(got[0], keep, form)
        np.testing.assert_array_equal(got[3].reshape(-1), covered.astype(np.uint8), form)
        assert (got[4], got[5]) == (c_all, c_kept), form
        if I.size:
            assert eng.info("panel_thin_rounds") == rounds
    return I, want


@pytest.mark.parametrize("k,M,picks", GRID)
def test_grid_in_the_three_forms_and_the_guarantee(m, eng, k, M, picks):
    g, fwd, rev = grid_case(k, M)
    opt = m.KmerOpt(400, 170, 50, k, 0, 0)
    I, want = check(eng, g, opt, fwd, rev, M, 3, forms=("host", "dev", "packed"))
    keep, order = want[0], want[1]
    assert len(order) == picks
    # the guarantee, through the existing call: the kept subset covers what the whole set covers
    whole, counts = eng.segment_coverage_mm(g, opt, fwd, rev, M, 3, per_primer=True)
    np.testing.assert_array_equal(counts, I.sum(axis=1))
    kf = [w for w, q in zip(fwd, keep[:len(fwd)]) if q]
    kr = [w for w, q in zip(rev, keep[len(fwd):]) if q]
    np.testing.assert_array_equal(eng.segment_coverage_mm(g, opt, kf, kr, M, 3) != 255, whole != 255)
    assert eng.info("panel_thin_groups") == -(-130 // 53)


@pytest.mark.parametrize("n_seq,L,n_seg", [(1, 400, 1), (4, 2440, 52), (53, 450, 53), (6, 1760, 54), (107, 500, 107),
                                           (10, 2950, 160)])
def test_group_boundaries(m, eng, n_seq, L, n_seg):
    """53 segments per group at W = 50, k = 13: one segment, one short of a group, a full group, groups whose last
    holds one segment (54, 107 and 160)."""
    g = m.synth.aligned_genomes(n_seq, L, seed=n_seg)
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    assert n_seq * tm.n_partitions(L, 400, 170) == n_seg
    fwd, rev = primer_sets(np.random.default_rng(n_seg), g, 30, 13)
    check(eng, g, opt, fwd, rev, 2, 3, forms=("host", "packed"))
    assert eng.info("panel_thin_groups") == -(-n_seg // 53)


@pytest.mark.parametrize("k,W", [(13, 50), (16, 40), (17, 50), (31, 70), (13, 13), (20, 20), (5, 2100)])
def test_word_widths_and_windows(m, eng, k, W):
    """Both word widths, W == k (one position per window), and W - k + 1 above one round of positions per block."""
    g = m.synth.aligned_genomes(6, 3000, seed=7)
    rng = np.random.default_rng(k + W)
    fwd, rev = primer_sets(rng, g, 25, k)
    opt = m.KmerOpt(max(W, 300), 150, W, k, 0, 0)
    check(eng, g, opt, fwd, rev, 2, 1, forms=("host", "packed"), chunk=4)


def test_more_primers_than_one_tile(m, eng):
    g = m.synth.aligned_genomes(3, 1500, seed=11)
    rng = np.random.default_rng(13)
    fwd = draw_primers(rng, g, 30000, 13, random_extra=100)
    rev = [rc(w) for w in draw_primers(rng, g, 20000, 13)]
    assert (len(fwd) + len(rev)) % 64
    opt = m.KmerOpt(300, 150, 40, 13, 0, 0)
    check(eng, g, opt, fwd, rev, 2, 3, chunk=1)


def test_ties_across_directions_and_a_word_listed_twice(m, eng):
    rng = np.random.default_rng(77)
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(8, 1400))].copy()
    seg, stride, W, k = 400, 200, 50, 13
    word = lambda: "".join("ACGT"[x] for x in rng.integers(0, 4, k))
    A, B, Cw, D = word(), word(), word(), word()

    def plant(rows, part, w, tail):
        col = part * stride + (seg - W + 9 if tail else 7)
        for r in rows:
            g[r, col:col + k] = np.frombuffer((rc(w) if tail else w).encode(), dtype=np.uint8)

    plant(range(0, 5), 2, A, False)    # forward A and reverse B cover the same five segments
    plant(range(0, 5), 2, B, True)
    plant(range(0, 5), 1, Cw, False)   # forward C and reverse D cover five each, other segments
    plant(range(3, 8), 3, D, True)
    fwd, rev = [word(), A, Cw, A], [D, B, word(), D]
    opt = m.KmerOpt(seg, stride, W, k, 0, 0)
    I, want = check(eng, g, opt, fwd, rev, 0, 3, forms=("host", "packed"))
    assert I.sum(axis=1).tolist() == [0, 5, 5, 5, 5, 5, 0, 5]
    assert want[1].tolist() == [1, 2, 4] and want[2].tolist() == [5, 5, 5]


@pytest.mark.parametrize("min_gain", [1, 2, 5])
def test_forced_primers_and_min_gain(m, eng, min_gain):
    g, fwd, rev = grid_case(13, 2)
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    n = len(fwd) + len(rev)
    check(eng, g, opt, fwd, rev, 2, 3, min_gain)
    rng = np.random.default_rng(min_gain)
    I, want = check(eng, g, opt, fwd, rev, 2, 3, min_gain, rng.random(n) < 0.06, forms=("host", "packed"))
    every = np.ones(n, dtype=np.uint8)                      # everything forced: nothing picked
    _, want = check(eng, g, opt, fwd, rev, 2, 3, min_gain, every)
    assert want[1].size == 0 and want[5] == want[4]
    best = tm.greedy(I)[1][:3]                              # the first picks forced: the rest goes on from there
    some = np.zeros(n, dtype=np.uint8)
    some[best] = 1
    check(eng, g, opt, fwd, rev, 2, 3, min_gain, some)


def test_empty_inputs(m, eng):
    g = m.synth.aligned_genomes(5, 1500, seed=3)
    fwd, rev = primer_sets(np.random.default_rng(3), g, 20, 13)
    opt = m.KmerOpt(400, 170, 50, 13, 0, 0)
    for f, r in (([], []), (fwd, []), ([], rev)):
        check(eng, g, opt, f, r, 2, 3, forms=("host", "dev", "packed"))
    n = len(fwd) + len(rev)
    forced = np.zeros(n, dtype=np.uint8)
    forced[[1, n - 1]] = 1
    got = eng.panel_thin(g, m.KmerOpt(2000, 170, 50, 13, 0, 0), fwd, rev, 2, 3, forced=forced)   # seq_len < segment
    assert got[0].tolist() == forced.tolist() and got[1].size == 0 and got[3].shape == (5, 0) and got[4:] == (0, 0)
    gaps = np.full((4, 1500), ord("-"), dtype=np.uint8)
    _, want = check(eng, gaps, opt, fwd, rev, 2, 3, forced=forced)
    assert want[1].size == 0 and want[4] == 0


def test_more_than_two_batches_of_rounds(m, eng):
    rng = np.random.default_rng(5)
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(6, 2000))].copy()   # unrelated rows
    opt = m.KmerOpt(400, 200, 50, 13, 0, 0)
    fwd = [bytes(g[r, j * 200 + 5:j * 200 + 18]).decode() for r in range(6) for j in range(9)]   # one per segment
    _, want = check(eng, g, opt, fwd, [], 0, 3)
    assert len(want[1]) >= 40
    assert eng.info("panel_thin_rounds") == len(want[1]) + 1 > 32


def test_matrix_cap(m, eng):
    g = m.synth.aligned_genomes(40, 6000, seed=9)
    opt = m.KmerOpt(400, 60, 50, 13, 0, 0)
    rng = np.random.default_rng(9)
    fwd, rev = primer_sets(rng, g, 995, 13)                 # 2,000 primers: 71 groups x 2,048 words, 1.16 MB
    default = eng.info("panel_thin_matrix_max_mb")
    assert default == 8192
    eng.set_option("panel_thin_matrix_max_mb", 1)
    try:
        with pytest.raises(m.MsspeError) as e:
            eng.panel_thin(g, opt, fwd, rev, 1, 3)
        assert e.value.code == 5 and "needs 2 MB" in str(e.value) and "panel_thin_matrix_max_mb is 1" in str(e.value)
    finally:
        eng.set_option("panel_thin_matrix_max_mb", default)
    keep, order, gains, covered, c_all, c_kept = eng.panel_thin(g, opt, fwd, rev, 1, 3)
    whole = eng.segment_coverage_mm(g, opt, fwd, rev, 1, 3)
    np.testing.assert_array_equal(covered == 1, whole != 255)
    assert c_all == c_kept == int((whole != 255).sum()) == int(gains.sum()) and keep.sum() == order.size
    for bad in (0, -1, "x", 1 << 21):
        with pytest.raises(m.MsspeError):
            eng.set_option("panel_thin_matrix_max_mb", bad)


def test_argument_errors(m, eng):
    L = m.load_library()
    g = m.synth.aligned_genomes(2, 1200, seed=1)
    n, Ln = g.shape
    w = m.pack_oligos(["ACGTACGTACGTA"])
    keep, order, gains = np.zeros(2, np.uint8), np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    picked = C.c_int(-1)

    def call(opt, mm, thin=m.ThinOpt(1), fw=w.ctypes.data, nf=1, rw=w.ctypes.data, nr=1, k=keep.ctypes.data,
             o=order.ctypes.data, ga=gains.ctypes.data, npk=C.byref(picked), seqs=g, fn=L.msspe_panel_thin, ctx=None):
        return fn(ctx or eng.ptr, seqs.ctypes.data if seqs is not None else None, n, Ln,
                  C.byref(opt) if opt is not None else None, C.byref(mm) if mm is not None else None,
                  C.byref(thin) if thin is not None else None, fw, nf, rw, nr, None, k, o, ga, npk, None, None, None)

    ok, mm = m.KmerOpt(500, 250, 50, 13, 0, 0), m.MismatchOpt(1, 3)
    assert call(ok, mm) == 0 and picked.value >= 0
    assert call(ok, mm, thin=None) == 1
    assert call(ok, mm, thin=m.ThinOpt(0)) == 1
    assert call(ok, mm, thin=m.ThinOpt(-4)) == 1
    assert call(ok, mm, k=None) == 1
    assert call(ok, mm, o=None) == 1
    assert call(ok, mm, ga=None) == 1
    assert call(ok, mm, npk=None) == 1
    assert call(None, mm) == 1
    assert call(ok, None) == 1
    assert call(ok, mm, fw=None) == 1
    assert call(ok, mm, rw=None) == 1
    assert call(ok, mm, fw=None, nf=0, rw=None, nr=0) == 0
    assert call(ok, mm, seqs=None) == 1
    assert call(ok, m.MismatchOpt(-1, 3)) == 1
    assert call(ok, m.MismatchOpt(14, 3)) == 1
    assert call(ok, m.MismatchOpt(1, 14)) == 1
    assert call(m.KmerOpt(500, 250, 50, 0, 0, 0), m.MismatchOpt(0, 0)) == 2
    assert call(m.KmerOpt(500, 250, 50, 32, 0, 0), mm) == 2
    assert call(m.KmerOpt(500, 250, 10, 13, 0, 0), mm) == 1      # window < k
    assert call(m.KmerOpt(40, 250, 50, 13, 0, 0), mm) == 1       # segment < window
    assert call(m.KmerOpt(500, 0, 50, 13, 0, 0), mm) == 1        # stride < 1
    high = np.array([1 << 26], dtype=np.uint64)                  # a base past k = 13
    assert call(ok, mm, fw=high.ctypes.data) == 1
    assert call(ok, mm, fn=L.msspe_panel_thin_dev, seqs=None) == 1
    assert call(ok, mm, fn=L.msspe_panel_thin_packed_dev, seqs=None) == 1


# ---- the CLI ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_fasta(m, tmp_path_factory):
    g = np.concatenate([m.synth.aligned_genomes(20, 6000, seed=700 + j) for j in range(2)])
    fa = tmp_path_factory.mktemp("thin_cli") / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    return fa, g


def run_cli(fa, csv, *extra):
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rows = [l.split(",") for l in Path(csv).read_text().splitlines()[1:] if l]
    return r.stdout, rows


def block_of(out):
    at = out.index("\nPanel thinning")
    return "".join(l + "\n" for l in out[at:].split("\n")[:4])


def cli_case(fa, g, tmp_path, extra, panel=((), ())):
    base_out, base = run_cli(fa, tmp_path / "a.csv", *extra)
    assert "Panel thinning" not in base_out
    out, rows = run_cli(fa, tmp_path / "b.csv", *extra, "--thin-panel", "true", "--thin-mismatches", "2")
    fwd = [r[2] for r in base if r[0] == "F"]
    rev = [r[2] for r in base if r[0] == "R"]
    all_f, all_r = fwd + list(panel[0]), rev + list(panel[1])
    forced = np.array([0] * len(fwd) + [1] * len(panel[0]) + [0] * len(rev) + [1] * len(panel[1]), dtype=np.uint8)
    I = tm.incidence(g, 500, 250, 50, 13, all_f, all_r, 2, 3)
    keep, order, gains, covered, c_all, c_kept, _ = tm.greedy(I, 1, forced)
    kf = [w for w, q in zip(fwd, keep[:len(fwd)]) if q]
    kr = [w for w, q in zip(rev, keep[len(all_f):len(all_f) + len(rev)]) if q]
    assert [r[2] for r in rows if r[0] == "F"] == kf and [r[2] for r in rows if r[0] == "R"] == kr
    assert 0 < len(kf) + len(kr) < len(fwd) + len(rev)
    assert block_of(out) == tm.render_block(2, 3, 1, len(kf), len(fwd), len(kr), len(rev), int(forced.sum()), c_all,
                                            c_kept, g.shape[0] * tm.n_partitions(g.shape[1], 500, 250))
    return base, rows, out


def test_cli_thins_the_panel(small_fasta, tmp_path):
    fa, g = small_fasta
    base, rows, out = cli_case(fa, g, tmp_path, ())
    stats = {r[2]: r[3:] for r in base}
    assert all(stats[r[2]] == r[3:] for r in rows)   # a survivor's row is what it was
    assert out.index("Coverage report") < out.index("Panel thinning")


def test_cli_with_existing_primers(small_fasta, tmp_path):
    fa, g = small_fasta
    _, first = run_cli(fa, tmp_path / "first.csv")
    panel_rows = [r for r in first if r[0] == "F"][:4] + [r for r in first if r[0] == "R"][:4]
    panel = tmp_path / "panel.csv"
    panel.write_text("direction,name,primers,gc,avg,std,tm\n" + "".join(",".join(r) + "\n" for r in panel_rows))
    pf = [r[2] for r in panel_rows if r[0] == "F"]
    pr = [r[2] for r in panel_rows if r[0] == "R"]
    _, rows, out = cli_case(fa, g, tmp_path, ("--existing-primers", str(panel)), (pf, pr))
    assert not {r[2] for r in rows} & set(pf + pr)
    assert ", 8 forced\n" in out


def test_cli_with_tubes(small_fasta, tmp_path):
    fa, g = small_fasta
    base, rows, out = cli_case(fa, g, tmp_path, ("--tubes", "4"))
    tube = {r[2]: r[7] for r in base}
    assert all(tube[r[2]] == r[7] for r in rows)     # survivors keep their tube numbers
    per_tube = [l for l in out[out.index("Tube assignment"):].splitlines() if l.startswith("  Tube ")]
    assert sum(int(l.split()[2]) for l in per_tube) == len([r for r in rows if r[7]])
