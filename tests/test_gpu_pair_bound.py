"""The bound first stage of the decision-only ANY screen (option pair_bound; csrc/thal_pairs_row.hip k_pairs_bound).

A screen that asks for counts and a bitmap only may run, in front of the exact stages, an instance of the row kernel
that computes a lower bound of every dG thal() could report for the pair -- the minimum over all chains of stacked pairs
and loops at the chemistry's temperature, in integers rounded down.  A pair whose bound is more than E = 1 cal/mol
above the cut is finished; every other pair goes to hand-over list 0.  So every decision must be the exact kernels',
hence the oracle's, bit for bit, whatever the chemistry, the tables and the threshold; and the bound itself
(msspe_cross_dimer_bound_dev) must never exceed the oracle's dG by more than E.

Pools: 640 seeded random oligos of 9, 12 and 13 bases; a perfect duplex, a self-complementary oligo, A*k / T*k (169
cells at 13 bases: more than the 52 stored cells, a size hand-over); and 20 pairs within 300 cal/mol of the cut."""
import numpy as np
import pytest

import param_variants as pv

pytestmark = pytest.mark.gpu

THR = -9000.0
E = 1.0            # cal/mol: fast_tables.hpp BoundTables::kMargin
N_RANDOM = 640
KS = (9, 12, 13)
# high_salt: mv + 120 sqrt(dv - dntp) = 600 + 120 sqrt(20) = 1136.7 > 1000 makes the per-pair salt step negative
CHEMS = {
    "ntthal25": ("ntthal", {}),
    "ntthal37": ("ntthal", {"temp_c": 37.0}),
    "primer3": ("primer3", {}),
    "high_salt": ("ntthal", {"mv": 600.0, "dv": 20.0}),
    "max_loop": ("ntthal", None),   # max_loop = 2k - 4, filled in per length
}


def chem_pair(m, oracle, name, k):
    kind, kw = CHEMS[name]
    kw = {"max_loop": 2 * k - 4} if kw is None else kw
    return getattr(m.Chem, kind)(**kw), (oracle.ntthal_args if kind == "ntthal" else oracle.p3_args)(**kw)


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
    """640 random oligos, the specials, and 20 pairs whose dG (ntthal, 25 C) lies within 300 cal/mol of the cut."""
    if k not in _pools:
        rng = np.random.default_rng(9100 + k)
        pool = m.synth.pool_strings(m.synth.random_pool(N_RANDOM, k, seed=700 + k))
        dup = "".join(rng.choice(list("ACGT"), k))
        half = "".join(rng.choice(list("ACGT"), k // 2))
        # (an oligo of odd length cannot be its own reverse complement: the palindrome then carries one more base)
        pool += [dup, oracle.reverse_complement(dup), (half + oracle.reverse_complement(half) + "A")[:k], "A" * k, "T" * k]
        near, tries = [], 0
        while len(near) < 20:
            tries += 1
            assert tries < 200000, "no near-cut pairs found"
            a = "".join(rng.choice(list("ACGT"), k, p=[0.15, 0.35, 0.35, 0.15]))
            b = list(oracle.reverse_complement(a))
            for p in rng.choice(k, size=int(rng.integers(0, 5)), replace=False):
                b[p] = "ACGT"[int(rng.integers(0, 4))]
            b = "".join(b)
            g = oracle.thal(oracle_tables, a, b).dG
            if abs(g - THR) < 300.0:
                near.append((a, b))
        for a, b in near:
            pool += [a, b]
        _pools[k] = (pool, [(N_RANDOM + 5 + 2 * q, N_RANDOM + 6 + 2 * q) for q in range(20)])
    return _pools[k]


def oracle_of(m, oracle, oracle_tables, k, chem_name, tables=None):
    """The oracle's dG plane of the pool: once per (length, chemistry, table set), shared and left unchanged."""
    key = (k, chem_name, id(tables))
    if key not in _oracle:
        pool, _ = pool_of(m, oracle, oracle_tables, k)
        _, oargs = chem_pair(m, oracle, chem_name, k)
        _, dg, _, _ = oracle.pool_pairs(tables or oracle_tables, pool, oargs, THR)
        dg.setflags(write=False)
        _oracle[key] = dg
    return _oracle[key]


def bits(bm, n):
    return np.unpackbits(np.ascontiguousarray(bm).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def screen(eng, pool, chem, thr, mode):
    """Decisions of the whole pool with pair_bound = mode: (bitmap as bool, row counts, statistics)."""
    eng.set_option("pair_bound", mode)
    eng.pair_stage_stats()
    eng.hand_over_lists()
    try:
        out = eng.cross_dimer(pool, chem, thr, want_dg=False)
    finally:
        eng.set_option("pair_bound", "auto")
    stats = eng.pair_stage_stats()
    stats["lists"] = eng.hand_over_lists()
    return bits(out["bitmap"], len(pool)), out["row_conflicts"], stats


def check_decisions(eng, m, pool, chem, thr, dg, modes=(1, 0)):
    want = dg <= m.g_cut(thr)
    res = {}
    for mode in modes:
        got, counts, stats = screen(eng, pool, chem, thr, mode)
        np.testing.assert_array_equal(got, want, err_msg=f"pair_bound={mode}")
        np.testing.assert_array_equal(counts, want.sum(1).astype(np.uint32), err_msg=f"pair_bound={mode}")
        res[mode] = stats
    return want, res


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("chem_name", list(CHEMS))
def test_decisions_equal_the_exact_stages_and_the_oracle(eng, m, oracle, oracle_tables, k, chem_name):
    pool, _ = pool_of(m, oracle, oracle_tables, k)
    chem, oargs = chem_pair(m, oracle, chem_name, k)
    dg = oracle_of(m, oracle, oracle_tables, k, chem_name)
    # the oracle's own decisions at this threshold are those of its dG plane under the exact cut
    _, _, cf, _ = oracle.pool_pairs(oracle_tables, pool, oargs, THR, want_dg=False)
    want, res = check_decisions(eng, m, pool, chem, THR, dg)
    np.testing.assert_array_equal(want, cf.astype(bool))
    print(f"k={k} {chem_name}: conflicts {int(want.sum())}, bound survivors {res[1]['bound_survivors']}, lists {res[1]['lists']}")
    assert res[0]["bound_survivors"] == 0
    # the bound ran; every conflict is among what it handed on (its survivors and the size hand-overs: list 0)
    assert res[1]["lists"][0] >= res[1]["bound_survivors"] > 0 and res[1]["lists"][0] >= int(want.sum())
    assert res[1]["deferred"] == 0      # the exact row kernel did not run; survivors are not "deferred"


def test_non_stock_tables(m, oracle, oracle_tables, tmp_path_factory):
    """Another parameter file (tests/param_variants.py loops_and_bonuses: other loop rows), oracle on the same file."""
    k = 13
    path = pv.write_bundle(pv.variant_sections("loops_and_bonuses"), tmp_path_factory.mktemp("tables") / "v.bundle")
    tables = oracle.Tables(path)
    e = m.Engine(0, params_path=str(path))
    try:
        pool, _ = pool_of(m, oracle, oracle_tables, k)
        dg = oracle_of(m, oracle, oracle_tables, k, "ntthal25", tables)
        want, res = check_decisions(e, m, pool, m.Chem.ntthal(), THR, dg)
        assert res[1]["bound_survivors"] > 0 and int(want[:N_RANDOM, :N_RANDOM].sum()) > 0
        check_bound_plane(e, m, pool, m.Chem.ntthal(), dg)
    finally:
        e.close()


def test_thresholds(eng, m, oracle, oracle_tables):
    """-9000, -3000 (most pairs survive: auto must end on the exact kernel), 0, +500 (a cut above 0: the bound must
    not run), and cuts that are pairs' own dG as float32 with both float32 neighbours."""
    k = 13
    pool, near = pool_of(m, oracle, oracle_tables, k)
    chem = m.Chem.ntthal()
    dg = oracle_of(m, oracle, oracle_tables, k, "ntthal25")
    for thr in (-9000.0, -3000.0, 0.0):
        _, res = check_decisions(eng, m, pool, chem, thr, dg, modes=(1, 0, "auto"))
        print(f"thr={thr}: forced {res[1]['bound_survivors']}, auto {res['auto']['bound_survivors']} survivors")
        assert res[1]["bound_survivors"] > 0
    # auto at -3000: the probe's survivors are counted apart; the screen itself ran the exact kernel
    _, res = check_decisions(eng, m, pool, chem, -3000.0, dg, modes=("auto",))
    assert res["auto"]["bound_survivors"] == 0
    _, res = check_decisions(eng, m, pool, chem, -9000.0, dg, modes=("auto",))
    assert res["auto"]["bound_survivors"] > 0
    _, res = check_decisions(eng, m, pool, chem, 500.0, dg, modes=(1, "auto"))
    assert res[1]["bound_survivors"] == 0 and res["auto"]["bound_survivors"] == 0
    for (i, j) in near[:4] + [(0, 1)]:
        g32 = np.float32(dg[i, j]) if np.isfinite(dg[i, j]) else np.float32(-9000.0)
        for thr in (np.nextafter(g32, np.float32(-np.inf)), g32, np.nextafter(g32, np.float32(np.inf))):
            if float(thr) <= 0.0:
                check_decisions(eng, m, pool, chem, float(thr), dg, modes=(1,))


def check_bound_plane(eng, m, pool, chem, dg):
    import torch
    n, k = len(pool), len(pool[0])
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    d_b = torch.full((n, n), 12345.0, dtype=torch.float64, device="cuda")
    eng.synchronize()
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        eng.cross_dimer_bound_dev(d_pool.data_ptr(), n, k, chem, THR, (0, n), (0, n), d_b.data_ptr())
        torch.cuda.synchronize()
    finally:
        eng.reset_stream()
    b = d_b.cpu().numpy()
    assert not (b == 12345.0).any()
    has = np.isfinite(dg)
    assert (b[has] <= dg[has] + E).all(), f"bound above dG + E: worst {np.max(b[has] - dg[has])}"
    # (-inf: pairs that stage hands on unbounded -- in a pool this small many waves mix compositions and shed lanes)
    finite = np.isfinite(b)
    assert (has & finite).any()
    gap = dg[has & finite] - b[has & finite]
    print(f"k={k}: bound below dG by {gap.mean():.1f} cal/mol on average, {gap.min():.4f} at least; "
          f"{int((~finite & has).sum())} pairs not bounded")
    return b


@pytest.mark.parametrize("k", KS)
def test_the_bound_never_exceeds_the_oracle(eng, m, oracle, oracle_tables, k):
    pool, _ = pool_of(m, oracle, oracle_tables, k)
    for chem_name in ("ntthal25", "high_salt"):
        chem, _ = chem_pair(m, oracle, chem_name, k)
        check_bound_plane(eng, m, pool, chem, oracle_of(m, oracle, oracle_tables, k, chem_name))


def test_survivor_cap(eng, m, oracle, oracle_tables):
    """25 C, -9000, the random part of the pool: survivors <= 1.5 x conflicts + 0.1 % of the pairs (the CPU experiment
    behind the stage gives 1.005 x): keeps a loose bound from passing unnoticed."""
    k = 13
    pool, _ = pool_of(m, oracle, oracle_tables, k)
    pool = pool[:N_RANDOM]
    dg = oracle_of(m, oracle, oracle_tables, k, "ntthal25")[:N_RANDOM, :N_RANDOM]
    want, res = check_decisions(eng, m, pool, m.Chem.ntthal(), THR, dg, modes=(1,))
    conflicts, surv = int(want.sum()), res[1]["bound_survivors"]
    print(f"conflicts {conflicts}, survivors {surv} ({surv / max(conflicts, 1):.3f} x), pairs {want.size}")
    # (conflicts among the pairs that stage hands on for their size are not survivors: no lower limit follows)
    assert conflicts > 0 and 0 < surv <= 1.5 * conflicts + 0.001 * want.size


def test_sub_block_between_guard_words(eng, m, oracle, oracle_tables):
    """One sub-block with partial column groups and rows: the bitmap block between guard words that stay intact, counts
    outside the block's rows untouched."""
    import torch
    k = 13
    pool, _ = pool_of(m, oracle, oracle_tables, k)
    n = len(pool)
    dg = oracle_of(m, oracle, oracle_tables, k, "ntthal25")
    r0, r1, c0, c1 = 37, n - 50, 70, n - 21
    nr, nc = r1 - r0, c1 - c0
    words, guard = (nc + 63) // 64, 4096
    want = dg[r0:r1, c0:c1] <= m.g_cut(THR)
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    d_rc = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_bm = torch.full((2 * guard + nr * words,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    eng.set_option("pair_bound", 1)
    eng.pair_stage_stats()
    eng.synchronize()
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        eng.cross_dimer_dev(d_pool.data_ptr(), n, k, m.Chem.ntthal(), THR, (r0, r1), (c0, c1), d_rc.data_ptr(),
                            d_bm.data_ptr() + 8 * guard)
        torch.cuda.synchronize()
    finally:
        eng.reset_stream()
        eng.set_option("pair_bound", "auto")
    assert eng.pair_stage_stats()["bound_survivors"] > 0
    g_bm = d_bm.cpu().numpy()
    assert (g_bm[:guard] == 0x5A5A5A5A5A5A5A5A).all() and (g_bm[-guard:] == 0x5A5A5A5A5A5A5A5A).all()
    np.testing.assert_array_equal(bits(g_bm[guard:-guard].reshape(nr, words).view(np.uint64), nc), want)
    rc = np.zeros(n, dtype=np.int64)
    rc[r0:r1] = want.sum(1)
    np.testing.assert_array_equal(d_rc.cpu().numpy().astype(np.int64), rc)


def test_routing_leaves_plane_and_edge_calls_alone(eng, m, oracle, oracle_tables):
    """want_dg = True and an edge-list call run what they ran before: no bound survivors, the oracle's values."""
    k = 13
    pool, _ = pool_of(m, oracle, oracle_tables, k)
    pool = pool[:200] + pool[N_RANDOM:]
    idx = list(range(200)) + list(range(N_RANDOM, N_RANDOM + len(pool) - 200))
    dg = oracle_of(m, oracle, oracle_tables, k, "ntthal25")[np.ix_(idx, idx)]
    eng.set_option("pair_bound", 1)
    try:
        eng.pair_stage_stats()
        out = eng.cross_dimer(pool, m.Chem.ntthal(), THR, want_dg=True)
        assert eng.pair_stage_stats()["bound_survivors"] == 0
        np.testing.assert_array_equal(out["dg"], dg)
        edges, count = eng.cross_dimer_edges(pool, m.Chem.ntthal(), THR)
        assert eng.pair_stage_stats()["bound_survivors"] == 0
    finally:
        eng.set_option("pair_bound", "auto")
    want = dg <= m.g_cut(THR)
    assert count == int(want.sum())
    got = np.zeros_like(want)
    got[edges["a"], edges["b"]] = True
    np.testing.assert_array_equal(got, want)


def test_two_runs_give_the_same_counters(eng, m, oracle, oracle_tables):
    k = 13
    pool, _ = pool_of(m, oracle, oracle_tables, k)
    runs = [screen(eng, pool, m.Chem.ntthal(), THR, 1) for _ in range(2)]
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    assert runs[0][2] == runs[1][2] and runs[0][2]["bound_survivors"] > 0
