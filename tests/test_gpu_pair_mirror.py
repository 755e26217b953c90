"""The mirrored bound first stage (option pair_mirror; csrc/thal_pairs_row.hip k_pairs_bound, capi.cpp run_chain).

On a square same-pool block whose tables are strand-symmetric term by term the bound stage fills each unordered pair
once -- rows in the columns' sorted order, row p against the sorted columns q >= p -- and hands a pair it cannot cull on
in both orders.  Every decision is still made by the exact stages, so bitmap and counts must be the oracle's with the
mirror on and off, at every pool size that changes the geometry (one lane, one group, a group and a lane, several
launches and flushes, two column segments), and every other kind of call must run as before (bound_mirrored == 0).

Pool (the recipe of test_gpu_pair_bound.py, specials first so that every prefix holds them): a perfect duplex, a
self-complementary oligo, A*k / T*k, 20 pairs within 300 cal/mol of the cut, one random oligo at two indices, random
oligos up to 700."""
import numpy as np
import pytest

import param_variants as pv
from pair_mirror_model import broken_sections

pytestmark = pytest.mark.gpu

THR = -9000.0
N_POOL = 700
SIZES = (1, 2, 63, 64, 65, 129, 700)
CHEMS = {"ntthal25": {}, "high_salt": {"mv": 600.0, "dv": 20.0}}
MAX_ASYM = 27 / 64        # two lower bounds of one real-number minimum, at most 27 terms rounded down to 1/64 cal/mol


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


_pools, _oracle = {}, {}


def pool_of(m, oracle, oracle_tables, k):
    if k not in _pools:
        rng = np.random.default_rng(9300 + k)
        dup = "".join(rng.choice(list("ACGT"), k))
        half = "".join(rng.choice(list("ACGT"), k // 2))
        pool = [dup, oracle.reverse_complement(dup), (half + oracle.reverse_complement(half) + "A")[:k], "A" * k, "T" * k]
        near, tries = [], 0
        while len(near) < 20:
            tries += 1
            assert tries < 200000, "no near-cut pairs found"
            a = "".join(rng.choice(list("ACGT"), k, p=[0.15, 0.35, 0.35, 0.15]))
            b = list(oracle.reverse_complement(a))
            for p in rng.choice(k, size=int(rng.integers(0, 5)), replace=False):
                b[p] = "ACGT"[int(rng.integers(0, 4))]
            b = "".join(b)
            if abs(oracle.thal(oracle_tables, a, b).dG - THR) < 300.0:
                near.append((a, b))
        for a, b in near:
            pool += [a, b]
        rnd = m.synth.pool_strings(m.synth.random_pool(N_POOL - len(pool) - 1, k, seed=900 + k))
        pool += [rnd[0], rnd[3], rnd[0]] + rnd[1:3] + rnd[4:]      # rnd[0] sits at two indices
        assert len(pool) == N_POOL and pool[45] == pool[47]
        _pools[k] = pool
    return _pools[k]


def oracle_of(m, oracle, oracle_tables, k, chem_name, tables=None):
    """The oracle's dG plane of the 700-oligo pool: once per (length, chemistry, table set), shared and left unchanged."""
    key = (k, chem_name, id(tables))
    if key not in _oracle:
        _, dg, _, _ = oracle.pool_pairs(tables or oracle_tables, pool_of(m, oracle, oracle_tables, k),
                                        oracle.ntthal_args(**CHEMS[chem_name]), THR)
        dg.setflags(write=False)
        _oracle[key] = dg
    return _oracle[key]


def bits(bm, n):
    return np.unpackbits(np.ascontiguousarray(bm).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def screen(eng, pool, chem, mirror, bound=1):
    """Decisions of the whole pool with pair_bound = bound and pair_mirror = mirror: (bitmap, row counts, statistics)."""
    eng.set_option("pair_bound", bound)
    eng.set_option("pair_mirror", mirror)
    eng.pair_stage_stats()
    eng.hand_over_lists()
    try:
        out = eng.cross_dimer(pool, chem, THR, want_dg=False)
        eng.last_overflow_pairs()      # raises if a hand-over list was overrun
    finally:
        eng.set_option("pair_bound", "auto")
        eng.set_option("pair_mirror", "auto")
    stats = eng.pair_stage_stats()
    stats["lists"] = eng.hand_over_lists()
    return out["bitmap"], out["row_conflicts"], stats


def test_option_values(eng, m):
    assert eng.info("pair_mirror") == 2
    for v, want in ((0, 0), (1, 1), ("auto", 2)):
        eng.set_option("pair_mirror", v)
        assert eng.info("pair_mirror") == want
    with pytest.raises(m.MsspeError):
        eng.set_option("pair_mirror", 2)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", [13, 9])
@pytest.mark.parametrize("chem_name", list(CHEMS))
def test_small_pools_equal_the_oracle(eng, m, oracle, oracle_tables, n, k, chem_name):
    pool = pool_of(m, oracle, oracle_tables, k)[:n]
    want = oracle_of(m, oracle, oracle_tables, k, chem_name)[:n, :n] <= m.g_cut(THR)
    chem = m.Chem.ntthal(**CHEMS[chem_name])
    for mirror in ("auto", 0):
        bm, counts, stats = screen(eng, pool, chem, mirror)
        np.testing.assert_array_equal(bits(bm, n), want, err_msg=f"pair_mirror={mirror}")
        np.testing.assert_array_equal(counts, want.sum(1).astype(np.uint32), err_msg=f"pair_mirror={mirror}")
        assert stats["bound_mirrored"] == (n * (n - 1) // 2 if mirror == "auto" else 0)
        assert stats["deferred"] == 0      # the bound stage ran, not the exact row kernel
        if n == N_POOL:
            print(f"k={k} {chem_name} pair_mirror={mirror}: conflicts {int(want.sum())}, survivors {stats['bound_survivors']}, "
                  f"lists {stats['lists']}")
            assert stats["lists"][0] >= stats["bound_survivors"] > 0


_launch_oracle = []


def launch_pool_and_oracle(m, oracle, oracle_tables):
    """1,500 random 13-mers and the oracle's conflicts among them: once for both cases, left unchanged."""
    if not _launch_oracle:
        pool = m.synth.pool_strings(m.synth.random_pool(1500, 13, seed=5))
        _, _, cf, _ = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(), THR, want_dg=False)
        want = cf.astype(bool)
        want.setflags(write=False)
        _launch_oracle.append((pool, want))
    return _launch_oracle[0]


@pytest.mark.parametrize("mirror", ["auto", 0])
def test_several_launches_and_flushes(eng, m, oracle, oracle_tables, mirror):
    """A list of 2^20 entries and 1,500 oligos: mirrored, 1,125,750 processed pairs, at most 2^19 per launch;
    un-mirrored, 2,250,000 pairs, at most 2^20 per launch and a flush between the launches."""
    pool, want = launch_pool_and_oracle(m, oracle, oracle_tables)
    eng.set_option("list_cap_log2", 20)
    eng.profile_enable(True)
    try:
        eng.profile_read()
        bm, counts, stats = screen(eng, pool, m.Chem.ntthal(), mirror)
        launches, _ = eng.profile_read()
    finally:
        eng.profile_enable(False)
        eng.set_option("list_cap_log2", 0)
    print(f"pair_mirror={mirror}: {launches} first-stage launches, survivors {stats['bound_survivors']}, lists {stats['lists']}")
    assert launches >= 3 and stats["bound_mirrored"] == (1500 * 1499 // 2 if mirror == "auto" else 0)
    np.testing.assert_array_equal(bits(bm, 1500), want)
    np.testing.assert_array_equal(counts, want.sum(1).astype(np.uint32))


@pytest.mark.parametrize("bound", [1, 0])
@pytest.mark.parametrize("mirror", ["auto", 0])
def test_launch_count_is_the_plans(eng, m, mirror, bound):
    """The same screen, pair_bound on and off: the first-stage launches the profile counts are the launches of the plan
    (csrc/screen_plan.hpp through msspe_host_screen_plan) for the stage that ran -- 3 in each of the four cases."""
    pool = m.synth.pool_strings(m.synth.random_pool(1500, 13, seed=5))
    stage = "row" if bound == 0 else "bound_mirror" if mirror == "auto" else "bound"
    plan = m.capi.host_screen_plan(stage, 0, 1500, 0, 1500, 1 << 20)
    eng.set_option("list_cap_log2", 20)
    eng.profile_enable(True)
    try:
        eng.profile_read()
        _, _, stats = screen(eng, pool, m.Chem.ntthal(), mirror, bound)
        launches, _ = eng.profile_read()
    finally:
        eng.profile_enable(False)
        eng.set_option("list_cap_log2", 0)
    print(f"pair_bound={bound} pair_mirror={mirror}: {launches} first-stage launches, plan '{stage}' has {len(plan)}")
    assert stats["bound_mirrored"] == (1500 * 1499 // 2 if stage == "bound_mirror" else 0)
    assert (stats["bound_survivors"] > 0) == (bound == 1)      # the stage the plan was asked for is the one that ran
    assert launches == len(plan) == 3


def test_two_column_segments(eng, m, oracle, oracle_tables):
    """16,449 oligos: 256 column groups, one more group and one more lane.  Mirror on and off agree everywhere; 64 seeded
    rows are the oracle's."""
    n = 256 * 64 + 64 + 1
    pool = m.synth.random_pool(n, 13, seed=41)
    res = {mirror: screen(eng, pool, m.Chem.ntthal(), mirror) for mirror in ("auto", 0)}
    np.testing.assert_array_equal(res["auto"][0], res[0][0])
    np.testing.assert_array_equal(res["auto"][1], res[0][1])
    assert res["auto"][2]["bound_mirrored"] == n * (n - 1) // 2 and res[0][2]["bound_mirrored"] == 0
    rows = sorted(int(r) for r in np.random.default_rng(6).choice(n, 64, replace=False))
    ext = np.concatenate([pool, pool[rows]])
    _, _, cf, _ = oracle.pool_pairs(oracle_tables, ext, oracle.ntthal_args(), THR, rows=(n, n + 64), want_dg=False)
    np.testing.assert_array_equal(bits(res["auto"][0][rows], n), cf[:, :n].astype(bool))


def test_the_devices_own_bound_is_symmetric(eng, m, oracle, oracle_tables):
    """msspe_cross_dimer_bound_dev keeps computing every ordered pair: where both orders are bounded they differ by
    rounding only, and "no chain" is common to both."""
    import torch
    k = 13
    pool = pool_of(m, oracle, oracle_tables, k)
    n = len(pool)
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    for chem_name in CHEMS:
        d_b = torch.full((n, n), 12345.0, dtype=torch.float64, device="cuda")
        eng.synchronize()
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            eng.cross_dimer_bound_dev(d_pool.data_ptr(), n, k, m.Chem.ntthal(**CHEMS[chem_name]), THR, (0, n), (0, n),
                                      d_b.data_ptr())
            torch.cuda.synchronize()
        finally:
            eng.reset_stream()
        b = d_b.cpu().numpy()
        assert not (b == 12345.0).any()
        both = np.isfinite(b) & np.isfinite(b.T)
        asym = np.abs(np.where(both, b, 0.0) - np.where(both, b.T, 0.0))[both]
        print(f"{chem_name}: {int(both.sum())} pairs bounded in both orders, |b[i,j] - b[j,i]| <= {asym.max() * 64:.0f}/64")
        assert both.sum() > n and (asym <= MAX_ASYM).all()
        # +inf (no chain) in one order: never a finite bound in the other (-inf: not bounded there, says nothing)
        assert not ((b == np.inf) & np.isfinite(b.T)).any()


def test_calls_the_mirror_leaves_alone(eng, m, oracle, oracle_tables):
    import torch
    k = 13
    pool = pool_of(m, oracle, oracle_tables, k)
    n = len(pool)
    dg = oracle_of(m, oracle, oracle_tables, k, "ntthal25")
    chem = m.Chem.ntthal()
    eng.set_option("pair_bound", 1)
    try:
        # ---- a sub-block: rows and columns differ
        r0, r1, c0, c1 = 37, n - 50, 70, n - 21
        nr, nc = r1 - r0, c1 - c0
        words = (nc + 63) // 64
        d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
        d_rc = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_bm = torch.zeros(nr * words, dtype=torch.int64, device="cuda")
        eng.pair_stage_stats()
        eng.synchronize()
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            eng.cross_dimer_dev(d_pool.data_ptr(), n, k, chem, THR, (r0, r1), (c0, c1), d_rc.data_ptr(), d_bm.data_ptr())
            torch.cuda.synchronize()
        finally:
            eng.reset_stream()
        stats = eng.pair_stage_stats()
        assert stats["bound_mirrored"] == 0 and stats["bound_survivors"] > 0
        want = dg[r0:r1, c0:c1] <= m.g_cut(THR)
        np.testing.assert_array_equal(bits(d_bm.cpu().numpy().reshape(nr, words).view(np.uint64), nc), want)
        np.testing.assert_array_equal(d_rc.cpu().numpy()[r0:r1], want.sum(1))
        # ---- a call with a dG plane, and an edge list
        sub = pool[:200]
        out = eng.cross_dimer(sub, chem, THR, want_dg=True)
        assert eng.pair_stage_stats()["bound_mirrored"] == 0
        np.testing.assert_array_equal(out["dg"], dg[:200, :200])
        edges, count = eng.cross_dimer_edges(sub, chem, THR)
        assert eng.pair_stage_stats()["bound_mirrored"] == 0
        want = dg[:200, :200] <= m.g_cut(THR)
        got = np.zeros_like(want)
        got[edges["a"], edges["b"]] = True
        assert count == int(want.sum())
        np.testing.assert_array_equal(got, want)
    finally:
        eng.set_option("pair_bound", "auto")


def test_asymmetric_bundle_runs_unmirrored(m, oracle, oracle_tables, tmp_path):
    """One stacked pair differs from its strand-swapped partner: the bound stage runs, every ordered pair on its own."""
    k = 13
    path = pv.write_bundle(broken_sections(), tmp_path / "broken.bundle")
    tables = oracle.Tables(path)
    pool = pool_of(m, oracle, oracle_tables, k)
    want = oracle_of(m, oracle, oracle_tables, k, "ntthal25", tables) <= m.g_cut(THR)
    e = m.Engine(0, params_path=str(path))
    try:
        bm, counts, stats = screen(e, pool, m.Chem.ntthal(), "auto")
    finally:
        e.close()
    assert stats["bound_mirrored"] == 0 and stats["bound_survivors"] > 0
    np.testing.assert_array_equal(bits(bm, len(pool)), want)
    np.testing.assert_array_equal(counts, want.sum(1).astype(np.uint32))


def test_two_runs_give_the_same_counters(eng, m, oracle, oracle_tables):
    pool = pool_of(m, oracle, oracle_tables, 13)
    runs = [screen(eng, pool, m.Chem.ntthal(), "auto") for _ in range(2)]
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    assert runs[0][2] == runs[1][2] and runs[0][2]["bound_mirrored"] > 0
