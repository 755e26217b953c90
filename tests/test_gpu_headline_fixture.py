"""bench.py's headline screen at full size against the oracle's whole rows (tests/golden/headline_65536.json, written by
tools/make_headline_fixture.py; tests/test_headline_fixture.py checks it is what it claims).

The 65,536^2 decisions-only call is the one call of the suite whose block holds more than 2^31 pairs, that runs as
nine launches, whose rows span four column segments of the row kernel, and whose hand-over lists fill and flush
between launches.  The fixture's 2,336 rows sit where that goes wrong: eight 256-row groups spread over the range
(G; half of them at or above row 32,768), 16 rows on each side of every launch boundary (B) and the last 32 rows (T).

The dealt-rows edge screen (msspe_amd.distributed.screen_dealt_rows_edges: the rows a rank owns are appended to the
pool and screened as one block, and edge.a is mapped back through the row list) is checked on the same pool for two
ranks of eight, and over every rank of small worlds."""
import hashlib
import json
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N, K, THR = 65536, 13, -9000.0
EDGE_CAP = 4 << 20


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def fx(golden_dir):
    d = json.loads((golden_dir / "headline_65536.json").read_text())
    d["row_sets"] = {name: [r for r0, r1 in ranges for r in range(r0, r1)] for name, ranges in d["row_sets"].items()}
    d["set_of"] = {r: name for name, rows in d["row_sets"].items() for r in rows}
    d["index"] = {r: i for i, r in enumerate(d["rows"])}
    return d


@pytest.fixture(scope="module")
def pool(m, fx):
    p = m.synth.random_pool(N, K)
    assert hashlib.sha256(p.tobytes()).hexdigest() == fx["pool"]["sha256"]
    return p


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def d_pool(m, pool):
    import torch
    return torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()


@pytest.fixture(scope="module")
def screen(m, eng, d_pool):
    """The headline call as bench.py makes it: counts and bitmap of the whole 65,536^2 block, default options, on
    the caller's stream."""
    import torch
    d_rc = torch.zeros(N, dtype=torch.int32, device="cuda")
    d_bm = torch.zeros((N, N // 64), dtype=torch.int64, device="cuda")
    eng.pair_stage_stats()                       # (resets the counters)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        t0 = time.perf_counter()
        eng.cross_dimer_dev(d_pool.data_ptr(), N, K, m.Chem.ntthal(), THR, (0, N), (0, N), d_rc.data_ptr(),
                            d_bm.data_ptr())
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        stats = eng.pair_stage_stats()
    finally:
        eng.reset_stream()
    out = {"rc": d_rc.cpu().numpy().astype(np.int64), "bm": d_bm.cpu().numpy().view(np.uint64), "stats": stats,
           "seconds": seconds}
    del d_bm
    torch.cuda.empty_cache()
    return out


def row_digest(cf_row: np.ndarray) -> str:
    """The fixture's digest: 8-byte BLAKE2b of one row's decisions packed as the engine's bitmap row."""
    return hashlib.blake2b(np.packbits(cf_row, bitorder="little").tobytes(), digest_size=8).hexdigest()


def bitmap_row_digest(bm_row: np.ndarray) -> str:
    return hashlib.blake2b(bm_row.view(np.uint8).tobytes(), digest_size=8).hexdigest()


def oracle_rows(oracle, tables, pool, rows, want_dg=False, want_t=False):
    """The oracle over rows x all columns of the pool: the rows are appended and screened as rows [n, n + len(rows))
    of the longer pool (the oracle runs rows in parallel), and the appended columns are dropped."""
    n = len(pool)
    ext = np.concatenate([pool, pool[list(rows)]])
    _, dg, cf, tt = oracle.pool_pairs(tables, ext, oracle.ntthal_args(), THR, oracle.ANY, rows=(n, n + len(rows)),
                                      want_dg=want_dg, want_t=want_t)
    return (dg[:, :n] if want_dg else None), cf[:, :n], (tt[:, :n] if want_t else None)


def oligo(pool, r):
    return bytes(pool[r]).decode()


def describe_rows(oracle, tables, pool, fx, bad, got_bits):
    """Up to 3 differing fixture rows, each with the first columns where the screen and the oracle disagree."""
    lines = []
    rows = bad[:3]
    dg, cf, _ = oracle_rows(oracle, tables, pool, rows, want_dg=True)
    for q, r in enumerate(rows):
        i = fx["index"][r]
        got = got_bits(r)
        cols = np.flatnonzero(got != cf[q])
        lines.append(f"row {r} (set {fx['set_of'][r]}): {int(got.sum())} conflicts, fixture {fx['counts'][i]}, "
                     f"oracle now {int(cf[q].sum())}; {cols.size} columns differ")
        s = oligo(pool, r)
        for c in cols[:5]:
            lines.append(f"    col {int(c)}: {s} x {oligo(pool, int(c))}  screen {int(got[c])}  oracle "
                         f"{int(cf[q, c])}  oracle dG {float(dg[q, c])!r}")
    return "\n".join(lines)


def bitmap_keys(bm, rows, chunk=1024):
    """Sorted row * N + column of every set bit of the bitmap rows `rows` (ascending)."""
    out = []
    for c0 in range(0, len(rows), chunk):
        rr = np.asarray(rows[c0:c0 + chunk], dtype=np.int64)
        i, j = np.nonzero(np.unpackbits(bm[rr].view(np.uint8), axis=1, bitorder="little"))
        out.append(rr[i] * N + j)
    return np.concatenate(out)


def test_headline_screen_equals_the_oracle_fixture(screen, fx, pool, oracle, oracle_tables):
    """Every fixture row of the headline screen: popcount, row count and bitmap-row digest are the oracle's."""
    bm, rc, stats = screen["bm"], screen["rc"], screen["stats"]
    print(f"headline screen: {screen['seconds']:.3f} s, {int(rc.sum())} conflicts")
    np.testing.assert_array_equal(np.bitwise_count(bm).sum(axis=1).astype(np.int64), rc)
    assert stats["replay_mismatch"] == 0 and stats["list"]["replay_mismatch"] == 0, stats
    rows = np.asarray(fx["rows"])
    pop = np.bitwise_count(bm[rows]).sum(axis=1).astype(np.int64)
    bad = [int(r) for i, r in enumerate(rows)
           if (pop[i], rc[r], bitmap_row_digest(bm[r])) != (fx["counts"][i], fx["counts"][i], fx["digests"][i])]
    if bad:
        by_set = {s: sum(fx["set_of"][r] == s for r in bad) for s in ("G", "B", "T")}
        got_bits = lambda r: np.unpackbits(bm[r].view(np.uint8), bitorder="little")[:N]   # noqa: E731
        pytest.fail(f"{len(bad)} of {rows.size} fixture rows differ (by set: {by_set}):\n"
                    + describe_rows(oracle, oracle_tables, pool, fx, bad, got_bits))


class _RecordingEngine:
    """Stands in for the engine in screen_dealt_rows_edges, which keeps only (a, b) of each edge: every call is
    forwarded, and the edge screen is also run a second time, with the same pool and block, into buffers of this
    object's own, so that the test can read the dG of the records as well."""

    def __init__(self, eng):
        self._eng = eng
        self.records = None

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def cross_dimer_edges_dev(self, d_pool, n, k, chem, threshold, rows, cols, d_edges, capacity, d_count):
        import torch
        self._eng.cross_dimer_edges_dev(d_pool, n, k, chem, threshold, rows, cols, d_edges, capacity, d_count)
        mine = torch.zeros(capacity * 2, dtype=torch.int64, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        self._eng.cross_dimer_edges_dev(d_pool, n, k, chem, threshold, rows, cols, mine.data_ptr(), capacity,
                                        cnt.data_ptr())
        torch.cuda.synchronize()
        c = int(cnt.item())
        assert c <= capacity
        self.records = mine[: 2 * c].cpu().numpy().view(np.dtype([("a", np.uint32), ("b", np.uint32),
                                                                   ("dg", np.float64)])).copy()


@pytest.fixture(scope="module")
def dealt(m, eng, d_pool):
    """Ranks 0 and 7 of eight through screen_dealt_rows_edges: (rows, sorted edge keys a * N + b, the records of the
    same screen with a mapped back through the rows, sorted by key)."""
    from msspe_amd import distributed
    out = {}
    for rank in (0, 7):
        rows = distributed.dealt_rows(N, 8, rank)
        rec = _RecordingEngine(eng)
        edges, count = distributed.screen_dealt_rows_edges(rec, d_pool, rows, K, m.Chem.ntthal(), THR, EDGE_CAP)
        assert 0 < count <= EDGE_CAP and len(edges) == count
        e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        del edges
        keys = e[:, 0] * N + e[:, 1]
        r = rec.records
        assert r["a"].size == count and np.all(r["a"] >= N) and np.all(r["a"] < N + rows.size)
        rk = rows[r["a"] - N].astype(np.int64) * N + r["b"]
        order = np.argsort(rk, kind="stable")
        out[rank] = (rows, np.sort(keys), rk[order], r["dg"][order])
    return out


def test_dealt_rows_edges_at_full_size(dealt, screen, fx):
    """Ranks 0 and 7 of eight: the edges, mapped back through the dealt rows, are the headline bitmap's bits of all
    8,192 rows, once each, and rebuild the fixture's rows that the rank owns (G in rank 0, T in rank 7)."""
    for rank, (rows, keys, rec_keys, _) in dealt.items():
        assert rows.size == 8192 and np.all((rows // 256) % 8 == rank)
        dup = keys[1:][np.diff(keys) == 0]
        assert dup.size == 0, f"rank {rank}: duplicate edges {[(int(x) // N, int(x) % N) for x in dup[:5]]}"
        want = bitmap_keys(screen["bm"], rows)
        if not np.array_equal(keys, want):
            extra, missing = np.setdiff1d(keys, want), np.setdiff1d(want, keys)
            pytest.fail(f"rank {rank}: {keys.size} edges, {want.size} bitmap bits; edges not in the bitmap "
                        f"{[(int(x) // N, int(x) % N) for x in extra[:5]]}, bits without an edge "
                        f"{[(int(x) // N, int(x) % N) for x in missing[:5]]}")
        np.testing.assert_array_equal(rec_keys, keys)          # the recorded run found the same edges
        mine = [r for r in fx["rows"] if (r // 256) % 8 == rank]
        assert len(mine) >= 32
        for r in mine:
            lo, hi = np.searchsorted(keys, [r * N, (r + 1) * N])
            cf = np.zeros(N, dtype=np.uint8)
            cf[keys[lo:hi] - r * N] = 1
            i = fx["index"][r]
            assert (hi - lo, row_digest(cf)) == (fx["counts"][i], fx["digests"][i]), \
                f"rank {rank}, row {r} (set {fx['set_of'][r]})"


@pytest.mark.parametrize("world", [2, 3])
def test_dealt_rows_edges_union_small_worlds(m, eng, world):
    """Every rank's edges, mapped back through its dealt rows, together are the whole pool's edge list, once each;
    a rank's edge count is the sum of its rows' conflicts from the exact-planes call."""
    import torch
    from msspe_amd import distributed
    n, cap = 3000, 1 << 18
    pool = m.synth.random_pool(n, K, seed=3000 + world)
    strs = m.synth.pool_strings(pool)
    chem = m.Chem.ntthal()
    want_edges, want_count = eng.cross_dimer_edges(strs, chem, THR, capacity=cap)
    want = np.stack([want_edges["a"], want_edges["b"]], 1).astype(np.int64)
    rc = eng.cross_dimer(strs, chem, THR, want_dg=True)["row_conflicts"].astype(np.int64)
    assert want_count == rc.sum() > 1000
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    got = []
    for rank in range(world):
        rows = distributed.dealt_rows(n, world, rank)
        assert world == 1 or not np.array_equal(rows, np.arange(rows.size))
        edges, count = distributed.screen_dealt_rows_edges(eng, d_pool, rows, K, chem, THR, cap)
        e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        assert count == len(e) == int(rc[rows].sum()), f"rank {rank} of {world}"
        assert np.all(np.isin(e[:, 0], rows)), f"rank {rank} of {world}: an edge outside the rank's rows"
        got.append(e)
    u = np.concatenate(got)
    u = u[np.lexsort((u[:, 1], u[:, 0]))]
    np.testing.assert_array_equal(u, want)


def test_headline_rows_exact_planes_at_full_width(m, eng, d_pool, pool, fx, dealt, oracle, oracle_tables):
    """Four fixture rows (one in the first group, one at or above 32,768, one on a launch boundary, the last) as
    one-row blocks against all 65,536 columns with the dG and Tm planes: both bit-equal to the oracle's, their
    decisions the fixture's, and the dG of the dealt-rows edges of those rows (ranks 0 and 7) the oracle's too."""
    import torch
    rng = np.random.default_rng(4)
    g = np.asarray(fx["row_sets"]["G"])
    pick = [int(rng.choice(g[g < 256])), int(rng.choice(g[g >= 32768])), int(rng.choice(fx["row_sets"]["B"])), N - 1]
    o_dg, o_cf, o_t = oracle_rows(oracle, oracle_tables, pool, pick, want_dg=True, want_t=True)
    cut = m.g_cut(THR)
    d_rc = torch.zeros(N, dtype=torch.int32, device="cuda")
    d_bm = torch.zeros((1, N // 64), dtype=torch.int64, device="cuda")
    d_dg = torch.empty((1, N), dtype=torch.float64, device="cuda")
    d_tm = torch.empty((1, N), dtype=torch.float64, device="cuda")
    checked_edges = 0
    for q, r in enumerate(pick):
        d_rc.zero_()
        d_dg.fill_(float("nan"))
        d_tm.fill_(float("nan"))
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            eng.cross_dimer_dev(d_pool.data_ptr(), N, K, m.Chem.ntthal(), THR, (r, r + 1), (0, N), d_rc.data_ptr(),
                                d_bm.data_ptr(), d_dg.data_ptr(), d_tm.data_ptr())
            torch.cuda.synchronize()
        finally:
            eng.reset_stream()
        dg, tm = d_dg.cpu().numpy()[0], d_tm.cpu().numpy()[0]
        bm = d_bm.cpu().numpy().view(np.uint64)[0]
        np.testing.assert_array_equal(dg, o_dg[q], err_msg=f"dG, row {r}")
        np.testing.assert_array_equal(dg.view(np.uint64), o_dg[q].view(np.uint64), err_msg=f"dG bits, row {r}")
        np.testing.assert_array_equal(tm, o_t[q], err_msg=f"Tm, row {r}")
        np.testing.assert_array_equal(tm.view(np.uint64), o_t[q].view(np.uint64), err_msg=f"Tm bits, row {r}")
        i = fx["index"][r]
        dec = (dg <= cut).astype(np.uint8)
        np.testing.assert_array_equal(dec, o_cf[q], err_msg=f"dG <= g_cut vs the oracle's decisions, row {r}")
        assert (int(dec.sum()), row_digest(dec)) == (fx["counts"][i], fx["digests"][i]), f"row {r}"
        assert bitmap_row_digest(bm) == fx["digests"][i] and int(d_rc[r].item()) == fx["counts"][i], f"row {r}"
        for rows, _, rec_keys, rec_dg in dealt.values():
            lo, hi = np.searchsorted(rec_keys, [r * N, (r + 1) * N])
            if hi == lo:
                continue
            cols = rec_keys[lo:hi] - r * N
            np.testing.assert_array_equal(cols, np.flatnonzero(o_cf[q]), err_msg=f"dealt edges, row {r}")
            np.testing.assert_array_equal(rec_dg[lo:hi].view(np.uint64), o_dg[q, cols].view(np.uint64),
                                          err_msg=f"dG of the dealt edges, row {r}")
            checked_edges += hi - lo
    assert checked_edges > 500           # rows of G and T are in ranks 0 and 7
