"""msspe_background_sites* on the device against the numpy model (tests/background_model.py): counts per strand and the
sorted site list, over a grid of k x mismatches x exact 3' bases, odd record shapes, primer sets larger than one LDS
tile, long streams, positions beyond 2^31, the three entry points, list truncation, streams, and the CLI's --background
block and --max-background-sites filter."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import background_model as bm

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


def random_seq(rng, n, p=None):
    return "".join(rng.choice(list("ACGT"), n, p=p))


def spoil(rng, s):
    """N runs and lower-case stretches at random places."""
    if len(s) < 200:
        return s
    out = list(s)
    for _ in range(max(1, len(s) // 4000)):
        a, n = int(rng.integers(0, len(s) - 100)), int(rng.integers(1, 40))
        out[a:a + n] = "N" * n
        b = int(rng.integers(0, len(s) - 100))
        out[b:b + 60] = [c.lower() for c in out[b:b + 60]]
    return "".join(out)[:len(s)]


def draw_primers(rng, records, n_drawn, n_random, k, max_subs=3):
    """n_drawn windows of the background with 0 .. max_subs substitutions, every other one reverse-complemented, then
    n_random random words."""
    out = []
    while len(out) < n_drawn:
        r = records[int(rng.integers(0, len(records)))]
        if len(r) < k:
            continue
        a = int(rng.integers(0, len(r) - k + 1))
        w = r[a:a + k]
        if any(c not in "ACGT" for c in w):
            continue
        w = list(w)
        for q in rng.choice(k, int(rng.integers(0, max_subs + 1)), replace=False):
            w[q] = "ACGT"[int(rng.integers(0, 4))]
        w = "".join(w)
        out.append(bm.revcomp(w) if len(out) % 2 else w)
    return out + [random_seq(rng, k) for _ in range(n_random)]


# ---- the grid -------------------------------------------------------------------------------------------------------
# The background of the grid holds no C, so that one primer can be known to have no site in every case, k = 8 with three
# mismatches included (a random 8-mer has thousands there): C C C C .. G G G G differs from every plus-strand window in
# its first four bases and from every reverse complement (which holds no G) in its last four.  The reverse complements
# hold C, so all four codes pass through the comparison; the other tests use all four letters in the records.
GRID_K = [8, 13, 16, 17, 24, 31]
_grid = {}


def grid_case(k):
    if k not in _grid:
        rng = np.random.default_rng(7000 + k)
        lens = [70001, 3, 45013, 0, 59990, 25000, k - 1, k]
        records = [spoil(rng, random_seq(rng, n, p=[0.3, 0.0, 0.35, 0.35])) for n in lens]
        records[4] = records[0][:30000] + records[4][30000:]   # a repeat: exact primers from it have several sites
        primers = draw_primers(rng, records, 150, 49, k) + ["CCCC" + "A" * (k - 8) + "GGGG"]
        _grid[k] = (records, primers, bm.candidates(records, primers, 3))
    return _grid[k]


@pytest.mark.parametrize("E", [0, 1, 3, "k"])
@pytest.mark.parametrize("M", [0, 1, 2, 3])
@pytest.mark.parametrize("k", GRID_K)
def test_grid_equals_the_model(eng, k, M, E):
    E = k if E == "k" else E
    records, primers, cand = grid_case(k)
    want_counts, want_sites = bm.sites(records, primers, M, E, cand=cand)
    counts, starts, sites = eng.background_sites(records, primers, M, E, capacity=len(want_sites) + 64)
    print(f"k={k} M={M} E={E}: {len(want_sites)} sites, {(want_counts.sum(1) == 0).sum()} primers without, "
          f"plus {want_counts[:, 0].sum()} minus {want_counts[:, 1].sum()}")
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_array_equal(sites, want_sites)
    np.testing.assert_array_equal(starts, bm.record_starts(records)[0])
    per = want_counts.sum(1)
    assert (per == 0).any() and (per > 1).any() and want_counts[:, 0].sum() > 0 and want_counts[:, 1].sum() > 0


# ---- odd shapes -----------------------------------------------------------------------------------------------------
def test_short_empty_and_single_records(eng):
    rng = np.random.default_rng(1)
    k = 13
    body = random_seq(rng, 5000)
    primers = [body[100:113], bm.revcomp(body[4000:4013]), random_seq(rng, k)]
    for records in ([body], ["", body, ""], ["ACGT", body[:12], body, "A" * 12], ["", ""], ["ACGTACGTACGT"], []):
        want_counts, want_sites = bm.sites(records, primers, 1, 2)
        counts, starts, sites = eng.background_sites(records, primers, 1, 2, capacity=1024)
        np.testing.assert_array_equal(counts, want_counts)
        np.testing.assert_array_equal(sites, want_sites)
        np.testing.assert_array_equal(starts, bm.record_starts(records)[0])
    assert eng.background_sites([body], primers, 1, 2)[0].sum() >= 2
    counts, _starts, sites = eng.background_sites([body], [], 1, 2, k=13, capacity=8)   # n = 0
    assert counts.shape == (0, 2) and len(sites) == 0


@pytest.mark.parametrize("k,n", [(13, 3001), (24, 1100)])
def test_more_primers_than_one_tile(eng, k, n):
    rng = np.random.default_rng(k)
    records = [random_seq(rng, 4000), random_seq(rng, 2500)]
    primers = draw_primers(rng, records, n - 200, 200, k, max_subs=2)
    want_counts, want_sites = bm.sites(records, primers, 2, 3)
    counts, _starts, sites = eng.background_sites(records, primers, 2, 3, capacity=len(want_sites) + 8)
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_array_equal(sites, want_sites)
    assert (want_counts.sum(1) > 0).sum() > n // 2


def test_long_stream_many_runs_per_block(eng):
    rng = np.random.default_rng(22)
    records = [random_seq(rng, (1 << 21) + 77), spoil(rng, random_seq(rng, (1 << 21) + 1001)), random_seq(rng, 300000)]
    assert sum(map(len, records)) >= 1 << 22
    primers = draw_primers(rng, records, 6, 2, 13)
    want_counts, want_sites = bm.sites(records, primers, 2, 3)
    counts, _starts, sites = eng.background_sites(records, primers, 2, 3, capacity=len(want_sites) + 8)
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_array_equal(sites, want_sites)
    assert len(want_sites) > 20 and want_counts[:, 0].sum() > 0 and want_counts[:, 1].sum() > 0


def test_positions_beyond_2_31(eng):
    """A stream of a little over 2^31 columns: one poly-A record, then 100 kb of the random kind; the primers (and their
    reverse complements) are far from poly-A and poly-T, so every site lies in the last record."""
    rng = np.random.default_rng(31)
    k, M, E = 13, 2, 3
    try:
        bulk = b"A" * ((1 << 31) + 4099)
    except MemoryError:
        pytest.skip("this machine cannot spare 2 GB of host memory for the poly-A record")
    last = spoil(rng, random_seq(rng, 100000))
    primers = [p for p in draw_primers(rng, [last], 40, 0, k)
               if max(p.count("A"), p.count("T")) < k - M - 2][:16]
    assert len(primers) >= 8
    want_counts, want_sites = bm.sites([last], primers, M, E)
    shift = len(bulk) + 1
    d, total, starts = eng.put_stream_packed([bulk, last])
    try:
        assert total == shift + len(last) and starts.tolist() == [0, shift]
        import torch
        cap = len(want_sites) + 8
        d_sites = torch.zeros(cap * 12, dtype=torch.uint8, device="cuda")
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        counts = eng.background_sites_packed(d, total, primers, M, E, d_sites=d_sites.data_ptr(), capacity=cap,
                                             d_count=d_count.data_ptr())
    finally:
        eng.device_free(d)
    np.testing.assert_array_equal(counts, want_counts)
    assert int(d_count.item()) == len(want_sites) > 0
    got = d_sites.cpu().numpy().view(bm.SITE_DTYPE)[:len(want_sites)]
    got = got[np.lexsort((got["pos"], got["strand"], got["primer"]))]
    want = want_sites.copy()
    want["pos"] = (want["pos"].astype(np.uint64) + np.uint64(shift)).astype(np.uint32)
    assert int(want["pos"].min()) > 1 << 31
    np.testing.assert_array_equal(got, want)


# ---- entry points, capacity, streams ---------------------------------------------------------------------------------
def device_list(eng, d, total, primers, M, E, cap, guard=64):
    import torch
    buf = torch.full(((cap + guard) * 12,), 0xA5, dtype=torch.uint8, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    counts = eng.background_sites_packed(d, total, primers, M, E, d_sites=buf.data_ptr(), capacity=cap,
                                         d_count=d_count.data_ptr())
    raw = buf.cpu().numpy()
    return counts, int(d_count.item()), raw[:cap * 12].view(bm.SITE_DTYPE), raw[cap * 12:]


def test_entry_points_agree_and_truncation_is_visible(m, eng):
    rng = np.random.default_rng(9)
    records = [spoil(rng, random_seq(rng, 60000)), random_seq(rng, 17), random_seq(rng, 30011)]
    primers = draw_primers(rng, records, 60, 20, 13)
    want_counts, want_sites = bm.sites(records, primers, 2, 3)
    n_sites = len(want_sites)
    assert n_sites > 100
    host_counts, starts, host_sites = eng.background_sites(records, primers, 2, 3, capacity=n_sites)
    np.testing.assert_array_equal(host_counts, want_counts)
    np.testing.assert_array_equal(host_sites, want_sites)
    np.testing.assert_array_equal(eng.background_sites(records, primers, 2, 3)[0], want_counts)   # counts only
    d, total, starts2 = eng.put_stream_packed(records)
    try:
        np.testing.assert_array_equal(starts2, starts)
        np.testing.assert_array_equal(eng.background_sites_packed(d, total, primers, 2, 3), want_counts)
        words = m.pack_oligos(primers)
        np.testing.assert_array_equal(eng.background_sites_packed(d, total, words, 2, 3, k=13), want_counts)
        counts, count, recs, guard = device_list(eng, d, total, primers, 2, 3, n_sites + 10)
        assert count == n_sites and (guard == 0xA5).all()
        np.testing.assert_array_equal(counts, want_counts)
        got = recs[:n_sites]
        np.testing.assert_array_equal(got[np.lexsort((got["pos"], got["strand"], got["primer"]))], want_sites)
        # a capacity below the count: the true count, `capacity` valid records, nothing written behind them
        cap = n_sites // 3
        counts, count, recs, guard = device_list(eng, d, total, primers, 2, 3, cap)
        assert count == n_sites and (guard == 0xA5).all()
        np.testing.assert_array_equal(counts, want_counts)
        all_sites = {tuple(r) for r in want_sites.tolist()}
        kept = [tuple(r) for r in recs.tolist()]
        assert len(set(kept)) == cap and set(kept) <= all_sites
    finally:
        eng.device_free(d)
    with pytest.raises(m.MsspeError) as e:
        eng.background_sites(records, primers, 2, 3, capacity=cap)
    assert e.value.code == 5 and e.value.count == n_sites and len(e.value.sites) == cap
    np.testing.assert_array_equal(e.value.counts, want_counts)
    assert {tuple(r) for r in e.value.sites.tolist()} <= all_sites


def test_argument_errors(m, eng):
    records = ["ACGTACGTACGTACGTACGTACGT"]
    for bad_m, bad_e in ((14, 0), (0, 14), (-1, 0), (0, -1)):
        with pytest.raises(m.MsspeError) as e:
            eng.background_sites(records, ["ACGTACGTACGTA"], bad_m, bad_e)
        assert e.value.code == 1
    for k in (0, 32):
        with pytest.raises(m.MsspeError) as e:
            eng.background_sites(records, np.zeros(1, dtype=np.uint64), 0, 0, k=k)
        assert e.value.code == 2
    with pytest.raises(m.MsspeError) as e:
        eng.background_sites(records, np.array([1 << 26], dtype=np.uint64), 0, 0, k=13)
    assert e.value.code == 1 and "bits above" in str(e.value)


def test_second_stream_and_kept_work_buffers(m, eng):
    import torch
    rng = np.random.default_rng(77)
    rec_a = [random_seq(rng, 50000), random_seq(rng, 900)]
    rec_b = [random_seq(rng, 7000)]
    prim_a = draw_primers(rng, rec_a, 300, 20, 13)
    prim_b = draw_primers(rng, rec_b, 10, 2, 20, max_subs=0)   # unchanged windows: each has its own site at least
    want_a, want_b = bm.sites(rec_a, prim_a, 2, 3)[0], bm.sites(rec_b, prim_b, 3, 1)[0]
    da, la, _ = eng.put_stream_packed(rec_a)
    db, lb, _ = eng.put_stream_packed(rec_b)
    stream = torch.cuda.Stream()
    try:
        eng.set_stream(stream.cuda_stream)
        for _ in range(2):   # alternating n, k and L on kept work buffers
            np.testing.assert_array_equal(eng.background_sites_packed(da, la, prim_a, 2, 3), want_a)
            np.testing.assert_array_equal(eng.background_sites_packed(db, lb, prim_b, 3, 1), want_b)
    finally:
        eng.reset_stream()
        eng.device_free(da)
        eng.device_free(db)
    np.testing.assert_array_equal(eng.background_sites(rec_a, prim_a, 2, 3)[0], want_a)
    assert want_a.sum() > 300 and want_b.sum() >= 10


# ---- the CLI ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_inputs(m, tmp_path_factory):
    rng = np.random.default_rng(2024)
    g = np.concatenate([m.synth.aligned_genomes(30, 9000, seed=500 + j) for j in range(2)])
    d = tmp_path_factory.mktemp("bg_cli")
    fa = d / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    # a background that shares stretches with the targets (so that some primers land in it), in lower case in part
    t0 = bytes(g[0]).decode().replace("-", "")
    records = [random_seq(rng, 30000) + t0[:3000] + random_seq(rng, 500), t0[5000:7000].lower() + bm.revcomp(t0[3000:6000]),
               "acgu" * 10 + "NNNN" + random_seq(rng, 12000).replace("T", "U", 50)]
    bg = d / "background.fa"
    bg.write_text("".join(f">b{i} background\n" + "\n".join(r[a:a + 70] for a in range(0, len(r), 70)) + "\n"
                          for i, r in enumerate(records)))
    normalised = [r.upper().replace("U", "T") for r in records]   # to_records: upper case, U -> T
    return fa, bg, normalised


def run_cli(fa, csv, *extra):
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout, Path(csv).read_bytes()


def csv_primers(csv):
    rows = [l.split(",") for l in csv.decode().splitlines()[1:] if l]
    return [r[1] for r in rows], [r[2] for r in rows]


def test_cli_block_and_filter(cli_inputs, tmp_path):
    fa, bg, records = cli_inputs
    base_out, base_csv = run_cli(fa, tmp_path / "a.csv")
    out, csv = run_cli(fa, tmp_path / "b.csv", "--background", str(bg))
    assert csv == base_csv and out.startswith(base_out)       # report only: the run itself is the parent's
    names, words = csv_primers(csv)
    counts, _ = bm.sites(records, words, 2, 3)
    assert out[len(base_out):] == bm.render(names, counts, 2, 3)
    assert (counts.sum(1) > 0).any() and (counts.sum(1) == 0).any()
    out1, _ = run_cli(fa, tmp_path / "c.csv", "--background", str(bg), "--background-mismatches", "1",
                      "--background-3p-exact", "5")
    assert out1[len(base_out):] == bm.render(names, bm.sites(records, words, 1, 5)[0], 1, 5)
    # the filter, seen without the vertex cover in the way: at a threshold no pair reaches, the CSV is the candidates
    quiet = ("--delta-g-threshold", "-1000000")
    _, all_csv = run_cli(fa, tmp_path / "d.csv", *quiet)
    all_names, all_words = csv_primers(all_csv)
    all_counts, _ = bm.sites(records, all_words, 2, 3)
    per = all_counts.sum(1)
    limit = int(np.sort(per)[len(per) * 3 // 4])
    assert (per > limit).any() and (per <= limit).any()
    f_out, f_csv = run_cli(fa, tmp_path / "e.csv", *quiet, "--background", str(bg), "--max-background-sites", str(limit))
    f_names, f_words = csv_primers(f_csv)
    assert f_words == [w for w, c in zip(all_words, per) if c <= limit]       # dropped: exactly the model's
    assert f_out.endswith(bm.render(f_names, bm.sites(records, f_words, 2, 3)[0], 2, 3))
    # --keep-all keeps them
    k_out, k_csv = run_cli(fa, tmp_path / "f.csv", "--keep-all", "true", "--background", str(bg),
                           "--max-background-sites", "0")
    _, ka_csv = run_cli(fa, tmp_path / "g.csv", "--keep-all", "true")
    assert k_csv == ka_csv
    # with the screen on: no dropped candidate comes back, and every conflict-free survivor set is a subset
    s_out, s_csv = run_cli(fa, tmp_path / "h.csv", "--background", str(bg), "--max-background-sites", str(limit))
    assert set(csv_primers(s_csv)[1]) <= set(f_words)
