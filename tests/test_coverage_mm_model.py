"""The numpy model of coverage within N mismatches (tests/coverage_mm_model.py) against the exact rule of the
reference's report (oracle/ref_pipeline.py, main.rs:518-594) at N = 0, on hand-built windows, and the CLI's new usage
errors through the host hooks -- no GPU needed."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import coverage_mm_model as cm

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"


def rc(s: str) -> str:
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def draw_primers(rng, genomes, n, k, subs_max=3, random_extra=5):
    """Words taken from genome columns (ACGT only) with 0..subs_max substitutions, plus random words."""
    out = []
    n_seq, L = genomes.shape
    while len(out) < n:
        r, c = int(rng.integers(n_seq)), int(rng.integers(0, L - k + 1))
        w = bytes(genomes[r, c:c + k]).decode()
        if set(w) - set("ACGT"):
            continue
        w = list(w)
        for q in rng.choice(k, size=int(rng.integers(0, subs_max + 1)), replace=False):
            w[q] = "ACGT"[(("ACGT".index(w[q])) + int(rng.integers(1, 4))) % 4]
        out.append("".join(w))
    out += ["".join("ACGT"[x] for x in rng.integers(0, 4, k)) for _ in range(random_extra)]
    return out


@pytest.mark.parametrize("seed,k,seg,stride,win", [(1, 13, 500, 250, 50), (2, 8, 300, 120, 30), (3, 17, 400, 400, 40)])
def test_zero_mismatches_is_the_exact_rule(oracle, seed, k, seg, stride, win):
    import msspe_amd
    import ref_pipeline
    g = msspe_amd.synth.aligned_genomes(8, 2500, seed=seed)
    rng = np.random.default_rng(seed)
    fwd = draw_primers(rng, g, 40, k, subs_max=0)
    rev = [rc(w) for w in draw_primers(rng, g, 40, k, subs_max=0)]
    recs = [(f"g{i}", bytes(r).decode()) for i, r in enumerate(g)]
    sel_f, sel_r = set(fwd), set(rev)
    want = []
    for _, s in recs:
        for part in oracle.partitions(s, seg, stride):
            want.append(any(w in sel_f for w in oracle.find_kmers(part[:win], k)) or
                        any(oracle.reverse_complement(w) in sel_r for w in oracle.find_kmers(part[len(part) - win:], k)))
    for E in (0, 3, k):
        best, _ = cm.best_and_counts(g, seg, stride, win, k, fwd, rev, 0, E)
        np.testing.assert_array_equal(best == 0, np.array(want))
    # and the rendered block's three lines are the reference report's at N = 0
    best, _ = cm.best_matrix(g, seg, stride, win, k, fwd, rev, 0, 3)
    block = cm.render_block([n for n, _ in recs], [len(s) for _, s in recs], best, seg, stride, 0, 3)
    ref = ref_pipeline.coverage_report(fwd, rev, recs, seg, stride, win, k)
    assert block.splitlines()[2:5] == ref.splitlines()[2:5]


def one_segment(head: str, tail: str, mid: int = 10) -> np.ndarray:
    s = head + "A" * mid + tail
    return np.frombuffer(s.encode(), dtype=np.uint8)[None, :]


def test_hand_built_windows():
    k, W = 8, 8
    p = "ACGTTGCA"
    tail_site = "GGGGGGGG"
    seg = one_segment(p, tail_site)
    L = seg.shape[1]
    run = lambda s, f, r, M, E: cm.best_and_counts(s, L, L, W, k, f, r, M, E)[0][0]
    assert run(seg, [p], [], 0, 3) == 0
    five = "T" + p[1:]                        # one substitution at the 5' end
    assert run(seg, [five], [], 0, 3) == 255
    assert run(seg, [five], [], 1, 3) == 1
    three = p[:-1] + "T"                      # the same substitution in the last E bases
    assert run(seg, [three], [], 1, 3) == 255
    assert run(seg, [three], [], 1, 0) == 1
    assert run(seg, [three], [], 8, 1) == 255
    # the reverse direction: the primer is the reverse complement of the tail window, mismatches alike
    rp = rc(tail_site)
    assert run(seg, [], [rp], 0, 8) == 0
    assert run(seg, [], ["A" + rp[1:]], 1, 3) == 1
    assert run(seg, [], [rp[:-1] + "A"], 2, 3) == 255
    # a window holding N or '-' never matches, at any mismatch count
    for bad in ("N", "-", "R"):
        s = one_segment(p[:4] + bad + p[5:], tail_site)
        assert run(s, [p], [], 8, 0) == 255
    # the smallest count wins, over both directions
    assert run(seg, [five, p[:2] + "TT" + p[4:]], [rp[:-3] + "AAA"], 3, 0) == 1


def test_counts_are_segments_not_positions():
    k, W = 6, 20
    p = "ACGTAC"
    g = np.frombuffer(("ACGTACGTACGTACGTACGT" + "C" * 30 + "ACGTACGTACGTACGTACGT").encode(), dtype=np.uint8)[None]
    best, counts = cm.best_and_counts(g, 70, 70, W, k, [p, p, "TTTTTT"], [], 0, 0)
    assert best.tolist() == [0] and counts.tolist() == [1, 1, 0]


@pytest.fixture(scope="module")
def host():
    import msspe_amd
    msspe_amd.load_library()
    return C.CDLL(str(LIB))


def parse(host, *a):
    argv = (C.c_char_p * (len(a) + 1))(b"od-msspe-hip", *[x.encode() for x in a])
    buf = C.create_string_buffer(1 << 16)
    rc_ = host.odm_parse_args(len(a) + 1, argv, buf, 1 << 16)
    return rc_, buf.value.decode()


def test_cli_flags_and_usage_errors(host, monkeypatch):
    for v in ("COVERAGE_MISMATCHES", "COVERAGE_3P_EXACT", "KMER_SIZE"):
        monkeypatch.delenv(v, raising=False)
    rc_, out = parse(host, "-i", "a", "-o", "b")
    kv = dict(l.split("=", 1) for l in out.splitlines())
    assert rc_ == 0 and kv["coverage_mismatches"] == "0" and kv["coverage_3p_exact"] == "3"
    rc_, out = parse(host, "-i", "a", "-o", "b", "--coverage-mismatches", "2", "--coverage-3p-exact", "5")
    kv = dict(l.split("=", 1) for l in out.splitlines())
    assert rc_ == 0 and kv["coverage_mismatches"] == "2" and kv["coverage_3p_exact"] == "5"
    for bad in (("--coverage-mismatches", "-1"), ("--coverage-mismatches", "1.5"), ("--coverage-mismatches", "x"),
                ("--coverage-mismatches", "14"), ("--coverage-mismatches", "1", "--coverage-3p-exact", "-2"),
                ("--coverage-mismatches", "1", "--coverage-3p-exact", "two"),
                ("--coverage-mismatches", "1", "--coverage-3p-exact", "14"),
                ("--kmer-size", "8", "--coverage-mismatches", "9")):
        rc_, out = parse(host, "-i", "a", "-o", "b", *bad)
        assert rc_ == 2 and "--coverage-" in out, (bad, out)
    # the 3' length is read only when mismatches are asked for
    rc_, _ = parse(host, "-i", "a", "-o", "b", "--kmer-size", "8", "--coverage-3p-exact", "9")
    assert rc_ == 0
    rc_, out = parse(host, "-i", "a", "-o", "b", "--coverage-mismatches", "13", "--coverage-3p-exact", "13")
    assert rc_ == 0
    monkeypatch.setenv("COVERAGE_MISMATCHES", "1")
    monkeypatch.setenv("COVERAGE_3P_EXACT", "0")
    kv = dict(l.split("=", 1) for l in parse(host, "-i", "a", "-o", "b")[1].splitlines())
    assert kv["coverage_mismatches"] == "1" and kv["coverage_3p_exact"] == "0"
    monkeypatch.setenv("COVERAGE_MISMATCHES", "20")
    assert parse(host, "-i", "a", "-o", "b")[0] == 2
    # the usage text names both flags with their environment variables
    rc_, out = parse(host, "--help")
    assert rc_ == 2 and "--coverage-mismatches <...>  [env: COVERAGE_MISMATCHES=]" in out
    assert "--coverage-3p-exact <...>  [env: COVERAGE_3P_EXACT=]" in out


def test_cli_usage_error_comes_before_the_engine(host, tmp_path):
    """A bad value is a usage error (status 2) before any device work: no GPU is needed to see it."""
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGTACGT\n")
    argv = [b"od-msspe-hip", b"-i", str(fa).encode(), b"-o", str(tmp_path / "o.csv").encode(), b"--do-align",
            b"false", b"--coverage-mismatches", b"2", b"--coverage-3p-exact", b"99"]
    arr = (C.c_char_p * len(argv))(*argv)
    buf = C.create_string_buffer(1 << 16)
    assert host.odm_run_cli(len(argv), arr, buf, 1 << 16) == 2
    assert "--coverage-3p-exact" in buf.value.decode()
