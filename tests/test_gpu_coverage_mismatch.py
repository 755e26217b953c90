"""msspe_segment_coverage_mm* on the device against the numpy model (tests/coverage_mm_model.py) and, at zero
mismatches, against the exact call (msspe_segment_coverage, main.rs:518-594): both word widths, several windows and
strides, primer sets larger than one LDS tile, the three entry points, the argument errors, the 10,000-genome fixture
and the CLI's --coverage-mismatches block."""
import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import coverage_mm_model as cm
from test_coverage_mm_model import draw_primers, rc

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
    fwd = draw_primers(rng, g, n, k)
    rev = [rc(w) for w in draw_primers(rng, g, n, k)]
    return fwd, rev


@pytest.mark.parametrize("k,W,seg,stride", [(8, 30, 200, 90), (13, 50, 500, 250), (16, 40, 300, 300),
                                             (17, 50, 400, 130), (24, 60, 500, 250), (31, 70, 350, 111)])
def test_zero_mismatches_is_the_exact_call(m, eng, k, W, seg, stride):
    g = m.synth.aligned_genomes(24, 4000, seed=k)
    rng = np.random.default_rng(k)
    fwd, rev = primer_sets(rng, g, 120, k)
    fwd = [w for w in fwd[::2]] + draw_primers(rng, g, 60, k, subs_max=0)
    opt = m.KmerOpt(seg, stride, W, k, 0, 0)
    exact = eng.segment_coverage(g, opt, fwd, rev)
    assert exact.any() and not exact.all()
    for E in sorted({0, 1, 3, k // 2, k}):
        best = eng.segment_coverage_mm(g, opt, fwd, rev, 0, E)
        np.testing.assert_array_equal(best == 0, exact == 1)
        assert set(np.unique(best).tolist()) <= {0, 255}


@pytest.mark.parametrize("k", [13, 24])
@pytest.mark.parametrize("M", [0, 1, 2, 3])
def test_grid_equals_the_model(m, eng, k, M):
    g = m.synth.aligned_genomes(10, 2600, seed=40 + k)
    rng = np.random.default_rng(100 * k + M)
    fwd, rev = primer_sets(rng, g, 60, k)
    opt = m.KmerOpt(400, 170, 50, k, 0, 0)
    seen = set()
    for E in sorted({0, 1, 3, k}):
        for f, r in ((fwd, rev), ([], rev), (fwd, []), ([], [])):
            best, counts = eng.segment_coverage_mm(g, opt, f, r, M, E, per_primer=True)
            want_b, want_c = cm.best_matrix(g, 400, 170, 50, k, f, r, M, E)
            np.testing.assert_array_equal(best, want_b)
            np.testing.assert_array_equal(counts, want_c)
            np.testing.assert_array_equal(eng.segment_coverage_mm(g, opt, f, r, M, E), want_b)
            seen |= set(np.unique(want_b).tolist())
    assert seen == set(range(M + 1)) | {255}   # every count up to M occurs somewhere, and segments without a match


@pytest.mark.parametrize("k,W", [(13, 20), (20, 20), (5, 300), (5, 2100)])
def test_short_and_long_windows(m, eng, k, W):
    """W == k (one position per window) and W - k + 1 above one round of positions per block."""
    g = m.synth.aligned_genomes(6, 3000, seed=7)
    rng = np.random.default_rng(k + W)
    fwd, rev = primer_sets(rng, g, 25, k)
    opt = m.KmerOpt(max(W, 300), 150, W, k, 0, 0)
    best, counts = eng.segment_coverage_mm(g, opt, fwd, rev, 2, 1, per_primer=True)
    want_b, want_c = cm.best_matrix(g, opt.segment_size, 150, W, k, fwd, rev, 2, 1, chunk=4)
    np.testing.assert_array_equal(best, want_b)
    np.testing.assert_array_equal(counts, want_c)


@pytest.mark.parametrize("k", [13, 24])
def test_more_primers_than_one_tile(m, eng, k):
    g = m.synth.aligned_genomes(3, 1500, seed=11)
    rng = np.random.default_rng(k)
    fwd = draw_primers(rng, g, 30000, k, random_extra=100)
    rev = [rc(w) for w in draw_primers(rng, g, 20000, k)]
    opt = m.KmerOpt(300, 150, 40, k, 0, 0)
    best, counts = eng.segment_coverage_mm(g, opt, fwd, rev, 2, 3, per_primer=True)
    want_b, want_c = cm.best_matrix(g, 300, 150, 40, k, fwd, rev, 2, 3, chunk=1)
    np.testing.assert_array_equal(best, want_b)
    np.testing.assert_array_equal(counts, want_c)


@pytest.mark.parametrize("k", [13, 24])
def test_entry_points_agree(m, eng, k):
    import torch
    g = m.synth.aligned_genomes(20, 5000, seed=3)
    rng = np.random.default_rng(5)
    fwd, rev = primer_sets(rng, g, 80, k)
    opt = m.KmerOpt(500, 250, 50, k, 0, 0)
    host = eng.segment_coverage_mm(g, opt, fwd, rev, 2, 3, per_primer=True)
    d = torch.from_numpy(np.ascontiguousarray(g)).cuda()
    torch.cuda.synchronize()
    dev = eng.segment_coverage_mm_dev(d.data_ptr(), g.shape[0], g.shape[1], opt, fwd, rev, 2, 3, per_primer=True)
    hp = eng.put_rows_packed(g)
    try:
        packed = eng.segment_coverage_mm_packed(hp, g.shape[0], g.shape[1], opt, fwd, rev, 2, 3, per_primer=True)
        packed_nc = eng.segment_coverage_mm_packed(hp, g.shape[0], g.shape[1], opt, fwd, rev, 2, 3)
    finally:
        eng.device_free(hp)
    for a, b in (host, dev), (host, packed):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(host[0], packed_nc)


def test_argument_errors(m, eng):
    L = m.load_library()
    g = m.synth.aligned_genomes(2, 1200, seed=1)
    n, Ln = g.shape
    w = m.pack_oligos(["ACGTACGTACGTA"])
    best = np.zeros(16, dtype=np.uint8)
    cnt = np.full(2, 7, dtype=np.uint32)

    def call(opt, mm, fw=w.ctypes.data, nf=1, rw=w.ctypes.data, nr=1, out=best.ctypes.data, counts=None, seqs=g,
             n_seq=n, seq_len=Ln):
        return L.msspe_segment_coverage_mm(eng.ptr, seqs.ctypes.data if seqs is not None else None, n_seq, seq_len,
                                           C.byref(opt) if opt is not None else None,
                                           C.byref(mm) if mm is not None else None, fw, nf, rw, nr, out, counts)

    ok = m.KmerOpt(500, 250, 50, 13, 0, 0)
    assert call(ok, m.MismatchOpt(1, 3)) == 0
    assert call(ok, None) == 1
    assert call(ok, m.MismatchOpt(1, 3), out=None) == 1
    assert call(ok, m.MismatchOpt(1, 3), fw=None) == 1
    assert call(ok, m.MismatchOpt(1, 3), rw=None) == 1
    assert call(ok, m.MismatchOpt(1, 3), fw=None, nf=0, rw=None, nr=0) == 0
    assert call(ok, m.MismatchOpt(1, 3), seqs=None) == 1
    assert call(ok, m.MismatchOpt(-1, 3)) == 1
    assert call(ok, m.MismatchOpt(14, 3)) == 1
    assert call(ok, m.MismatchOpt(1, -1)) == 1
    assert call(ok, m.MismatchOpt(1, 14)) == 1
    assert call(ok, m.MismatchOpt(13, 13)) == 0
    assert call(m.KmerOpt(500, 250, 50, 0, 0, 0), m.MismatchOpt(0, 0)) == 2
    assert call(m.KmerOpt(500, 250, 50, 32, 0, 0), m.MismatchOpt(1, 3)) == 2
    assert call(m.KmerOpt(500, 250, 10, 13, 0, 0), m.MismatchOpt(1, 3)) == 1     # window < k
    assert call(m.KmerOpt(40, 250, 50, 13, 0, 0), m.MismatchOpt(1, 3)) == 1      # segment < window
    assert call(m.KmerOpt(500, 0, 50, 13, 0, 0), m.MismatchOpt(1, 3)) == 1       # stride < 1
    high = np.array([1 << 26], dtype=np.uint64)                                  # a base past k = 13
    assert call(ok, m.MismatchOpt(1, 3), fw=high.ctypes.data) == 1
    assert call(ok, m.MismatchOpt(1, 3), rw=high.ctypes.data) == 1
    # no segments: OK, the counts zeroed
    assert call(m.KmerOpt(5000, 250, 50, 13, 0, 0), m.MismatchOpt(1, 3), counts=cnt.ctypes.data) == 0
    assert cnt.tolist() == [0, 0]
    assert L.msspe_segment_coverage_mm(None, g.ctypes.data, n, Ln, C.byref(ok), C.byref(m.MismatchOpt(1, 3)),
                                       w.ctypes.data, 1, w.ctypes.data, 1, best.ctypes.data, None) == 1
    assert L.msspe_segment_coverage_mm_dev(eng.ptr, None, n, Ln, C.byref(ok), C.byref(m.MismatchOpt(1, 3)),
                                           w.ctypes.data, 1, w.ctypes.data, 1, best.ctypes.data, None) == 1
    assert L.msspe_segment_coverage_mm_packed_dev(eng.ptr, None, n, Ln, C.byref(ok), C.byref(m.MismatchOpt(1, 3)),
                                                  w.ctypes.data, 1, w.ctypes.data, 1, best.ctypes.data, None) == 1


def test_config2_scale(m, eng, golden_dir):
    fx = json.loads((golden_dir / "config2_10k.json").read_text())
    kept = fx["primers_kept"]
    g = m.synth.aligned_genomes(fx["rows"], fx["length"])
    o = fx["options"]
    opt = m.KmerOpt(o["segment"], o["stride"], o["window"], o["k"], 0, 0)
    hp = eng.put_rows_packed(g)
    try:
        exact = eng.segment_coverage(g, opt, kept["F"], kept["R"])
        bests = [eng.segment_coverage_mm_packed(hp, g.shape[0], g.shape[1], opt, kept["F"], kept["R"], M, 3)
                 for M in range(4)]
    finally:
        eng.device_free(hp)
    np.testing.assert_array_equal(bests[0] == 0, exact == 1)
    covered = [int((b <= M).sum()) for M, b in enumerate(bests)]
    assert covered == sorted(covered) and covered[2] > covered[0]
    for M in range(1, 4):   # a higher bound keeps every smaller count and only adds segments
        lo, hi = bests[M - 1], bests[M]
        assert (hi[lo <= M - 1] == lo[lo <= M - 1]).all()
    rng = np.random.default_rng(2000)
    P = exact.shape[1]
    pick = rng.choice(g.shape[0] * P, size=2000, replace=False)
    segs = [(int(i // P), int(i % P)) for i in pick]
    want, _ = cm.best_and_counts(g, o["segment"], o["stride"], o["window"], o["k"], kept["F"], kept["R"], 2, 3,
                                 segments=segs, chunk=16)
    np.testing.assert_array_equal(bests[2].reshape(-1)[pick], want)


@pytest.fixture(scope="module")
def small_fasta(m, tmp_path_factory):
    g = np.concatenate([m.synth.aligned_genomes(30, 9000, seed=500 + j) for j in range(2)])
    fa = tmp_path_factory.mktemp("mm_cli") / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    return fa, g


def run_cli(fa, csv, *extra):
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout, Path(csv).read_bytes()


def test_cli_block(small_fasta, tmp_path):
    fa, g = small_fasta
    base_out, base_csv = run_cli(fa, tmp_path / "a.csv")
    zero_out, zero_csv = run_cli(fa, tmp_path / "b.csv", "--coverage-mismatches", "0")
    assert (zero_out, zero_csv) == (base_out, base_csv)
    out, csv = run_cli(fa, tmp_path / "c.csv", "--coverage-mismatches", "2", "--coverage-3p-exact", "3")
    assert csv == base_csv and out.startswith(base_out)
    rows = [l.split(",") for l in csv.decode().splitlines()[1:] if l]
    fwd = [r[2] for r in rows if r[0] == "F"]
    rev = [r[2] for r in rows if r[0] == "R"]
    best, _ = cm.best_matrix(g, 500, 250, 50, 13, fwd, rev, 2, 3)
    want = cm.render_block([f"g{i}" for i in range(len(g))], [g.shape[1]] * len(g), best, 500, 250, 2, 3)
    assert out[len(base_out):] == want
    assert "Segments by best match: 0 mm" in want


def test_host_hook_renders_the_block(m, small_fasta):
    _, g = small_fasta
    g = g[:12, :3000]
    rng = np.random.default_rng(9)
    fwd, rev = primer_sets(rng, g, 20, 13)
    host = C.CDLL(str(ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"))
    buf = C.create_string_buffer(1 << 20)
    recs = "".join(f"g{i}\t{bytes(r).decode()}\n" for i, r in enumerate(g)).encode()
    n = host.odm_coverage_report_mm(recs, "\n".join(fwd).encode(), "\n".join(rev).encode(), 500, 250, 50, 13, 1, 2,
                                    buf, 1 << 20)
    assert n > 0, buf.value.decode()
    best, _ = cm.best_matrix(g, 500, 250, 50, 13, fwd, rev, 1, 2)
    assert buf.value.decode() == cm.render_block([f"g{i}" for i in range(len(g))], [g.shape[1]] * len(g), best, 500,
                                                 250, 1, 2)
