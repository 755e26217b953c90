"""tests/golden/headline_65536.json is what it claims (no GPU): the oracle's decisions on about 2,340 whole rows of
bench.py's headline screen (65,536 random 13-mers, thal ANY, default ntthal chemistry, threshold -9000), written by
tools/make_headline_fixture.py.  tests/test_gpu_headline_fixture.py holds the GPU screen to it."""
import hashlib
import json

import numpy as np
import pytest


@pytest.fixture(scope="module")
def fx(golden_dir):
    d = json.loads((golden_dir / "headline_65536.json").read_text())
    d["row_sets"] = {name: [r for r0, r1 in ranges for r in range(r0, r1)] for name, ranges in d["row_sets"].items()}
    return d


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


def row_digest(cf_row: np.ndarray) -> str:
    """The fixture's digest of one row's decisions: the bytes of the engine's bitmap row."""
    return hashlib.blake2b(np.packbits(cf_row, bitorder="little").tobytes(), digest_size=8).hexdigest()


def test_the_pool_is_bench_pool(fx, m):
    p = fx["pool"]
    assert (p["n"], p["k"], p["seed"], fx["k"]) == (65536, 13, m.synth.POOL_SEED, 13)
    pool = m.synth.random_pool(p["n"], p["k"])
    assert hashlib.sha256(pool.tobytes()).hexdigest() == p["sha256"]     # RNG or generator drift
    assert (fx["threshold"], fx["mode"]) == (-9000.0, "ANY")
    c = m.Chem.ntthal()
    assert fx["chem"] == {"mv": c.mv, "dv": c.dv, "dntp": c.dntp, "dna_conc": c.dna_conc, "max_loop": c.max_loop,
                          "temp_c": c.temp_c}


def test_row_sets(fx, m):
    n = fx["pool"]["n"]
    rows = np.asarray(fx["rows"], dtype=np.int64)
    assert rows.size == len(fx["counts"]) == len(fx["digests"])
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n            # sorted, unique, in range
    sets = {k: np.asarray(v, dtype=np.int64) for k, v in fx["row_sets"].items()}
    assert sorted(sets) == ["B", "G", "T"]
    np.testing.assert_array_equal(sets["G"], m.group_rows(n, 32, 0))
    assert sets["G"].size == 2048 and np.count_nonzero(sets["G"] >= 32768) == 1024
    bounds = fx["launch_boundaries"]
    assert len(bounds) >= 2 and all(0 < b < n for b in bounds)
    np.testing.assert_array_equal(sets["B"], sorted({r for b in bounds for r in range(b - 16, b + 16)}))
    np.testing.assert_array_equal(sets["T"], np.arange(n - 32, n))
    np.testing.assert_array_equal(rows, np.unique(np.concatenate(list(sets.values()))))
    assert all(len(d) == 16 and int(d, 16) >= 0 for d in fx["digests"])


def test_conflict_rate(fx):
    n = fx["pool"]["n"]
    counts = np.asarray(fx["counts"], dtype=np.int64)
    assert np.all((counts >= 0) & (counts <= n))
    assert 0.004 < counts.sum() / (counts.size * float(n)) < 0.007    # 0.54 % of random 13-mer pairs conflict


def test_four_rows_recomputed_by_the_oracle(fx, m, oracle, oracle_tables):
    """A seeded draw of 4 fixture rows (one at or above 32,768, one on a launch boundary) against all 65,536 columns.
    The rows are appended to the pool and screened as rows [n, n + 4) of it, so the oracle runs them in parallel;
    the 4 appended columns are dropped."""
    n = fx["pool"]["n"]
    rows = np.asarray(fx["rows"])
    rng = np.random.default_rng(65536)
    pick = [int(rng.choice(fx["row_sets"]["B"])), int(rng.choice(rows[rows >= 32768]))]
    while len(pick) < 4:
        r = int(rng.choice(rows))
        if r not in pick:
            pick.append(r)
    pool = m.synth.random_pool(n, fx["k"])
    ext = np.concatenate([pool, pool[pick]])
    _, _, cf, _ = oracle.pool_pairs(oracle_tables, ext, oracle.ntthal_args(), fx["threshold"], oracle.ANY,
                                    rows=(n, n + len(pick)), want_dg=False)
    index = {r: i for i, r in enumerate(fx["rows"])}
    for q, r in enumerate(pick):
        i = index[r]
        assert (int(cf[q, :n].sum()), row_digest(cf[q, :n])) == (fx["counts"][i], fx["digests"][i]), r
