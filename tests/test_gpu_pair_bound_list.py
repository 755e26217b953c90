"""The bound list stage (option pair_bound_list; csrc/thal_pairs_bound_list.hip k_pairs_bound_list, capi.cpp run_chain).

A lane that leaves the bound first stage without a bound of its own -- 53..63 stored cells, dragged, shed by the slot fit
-- goes to list U, once per unordered pair under the mirror, and gets the same min-plus bound from a list kernel before the
exact lists; what that cannot cull joins list 0.  So (1) its value (msspe_cross_dimer_bound_list_dev) is the very integer
of tests/pair_bound_model.py, == on float64, and the plane is -inf / +inf exactly where pair_bound_list_model.py says;
(2) every decision stays the exact stages', hence the oracle's, and is bit-identical with the stage on and off, on every
kind of block; (3) the counters say that it ran, and that list 0 got shorter.

Pools: pair_bound_list_model.skewed_pool -- P(A) = P(T) = 0.35, so that a sixth of the 13-mer pairs have 53..63 stored
cells -- with mixed_pool's extras and A-rich / T-rich oligos; every test asserts that its pool holds the classes it is
about.  The Python model is slow on large tables: values are compared on seeded samples of each class (every pair on the
diagonal included), the -inf / +inf pattern and the agreement with the first stage's own plane on every pair.
The two-stem family has no pair beyond 52 stored cells (test_pair_bound_list_model.py): nothing of it reaches this stage."""
import numpy as np
import pytest

import param_variants as pv
from pair_bound_model import EDGE_CHEMS, bound_pair, long_loops_cheap_sections
from pair_bound_list_model import BATCH, class_plane, pair_class, skewed_pool
from pair_mirror_model import broken_sections

pytestmark = pytest.mark.gpu

THR = -9000.0
MARKER = 12345.0
VALUE_CHEMS = {"ntthal25": {}, "t0": EDGE_CHEMS["t0"], "t100": EDGE_CHEMS["t100"], "mv1000_dv100": EDGE_CHEMS["mv1000_dv100"]}
N_VALUES = 200        # skewed oligos of a value pool
N_DECISIONS = 300     # ... of the decision pool
SAMPLE = {"u": 250, "shed": 100, "row": 100}


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


def bits(bm, n):
    return np.unpackbits(np.ascontiguousarray(bm).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


_pools, _classes, _oracle = {}, {}, {}


def pool_of(k, n_random):
    if (k, n_random) not in _pools:
        _pools[(k, n_random)] = skewed_pool(k, n_random, seed=8100 + k)
        c = class_plane(_pools[(k, n_random)], _pools[(k, n_random)])
        c.setflags(write=False)
        _classes[(k, n_random)] = c
    return _pools[(k, n_random)], _classes[(k, n_random)]


def oracle_of(oracle, tables, pool, key, **chem_kw):
    """The oracle's conflicts of the pool at THR: once per key, shared and left unchanged."""
    if key not in _oracle:
        _, _, cf, _ = oracle.pool_pairs(tables, pool, oracle.ntthal_args(**chem_kw), THR, want_dg=False)
        want = cf.astype(bool)
        want.setflags(write=False)
        _oracle[key] = want
    return _oracle[key]


def planes(eng, m, pool, chem, thr=THR):
    """(the first stage's plane, the plane with the list stage behind it) of the whole pool."""
    import torch
    n, k = len(pool), len(pool[0])
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    out = []
    eng.synchronize()
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for call in (eng.cross_dimer_bound_dev, eng.cross_dimer_bound_list_dev):
            d_b = torch.full((n, n), MARKER, dtype=torch.float64, device="cuda")
            call(d_pool.data_ptr(), n, k, chem, thr, (0, n), (0, n), d_b.data_ptr())
            torch.cuda.synchronize()
            out.append(d_b.cpu().numpy())
    finally:
        eng.reset_stream()
    for b in out:
        assert not (b == MARKER).any() and not np.isnan(b).any()
    return out


def check_plane(eng, m, pool, cls, chem, bt, what):
    first, b = planes(eng, m, pool, chem)
    # ---- the pattern, every pair: -inf exactly for two self-complementary oligos and more than 63 stored cells, +inf
    #      exactly for pairs without a complementary cell, a value everywhere else
    np.testing.assert_array_equal(b == -np.inf, (cls == "sym") | (cls == "over"), err_msg=f"{what}: -inf")
    np.testing.assert_array_equal(b == np.inf, cls == "none", err_msg=f"{what}: +inf")
    # ---- what the first stage bounded itself is unchanged, bit for bit
    kept = first != -np.inf
    np.testing.assert_array_equal(b[kept], first[kept], err_msg=f"{what}: a pair the first stage bounded")
    assert not np.isfinite(first[cls == "u"]).any()      # 53..63 stored cells: never the first stage's
    # ---- the values: seeded samples of 53..63-cell pairs, of the lanes the first stage dragged or shed, of its own, and
    #      the whole diagonal
    shed = (first == -np.inf) & (cls == "row")
    groups = {"u": cls == "u", "shed": shed, "row": kept & (cls == "row")}
    rng = np.random.default_rng(len(pool))
    n_checked = {}
    for name, mask in groups.items():
        idx = np.argwhere(mask)
        assert len(idx) > 0, f"{what}: the pool has no pair of class {name}"
        if len(idx) > SAMPLE[name]:
            idx = idx[rng.choice(len(idx), SAMPLE[name], replace=False)]
        for i, j in idx:
            assert b[i, j] == bound_pair(bt, pool[i], pool[j]), (what, name, pool[i], pool[j], b[i, j])
        n_checked[name] = len(idx)
    for i in range(len(pool)):
        if np.isfinite(b[i, i]):
            assert b[i, i] == bound_pair(bt, pool[i], pool[i]), (what, "diagonal", pool[i])
    print(f"{what}: {int((cls == 'u').sum())} pairs with 53..63 cells, {int(shed.sum())} dragged or shed, "
          f"{int(((cls == 'sym') | (cls == 'over')).sum())} left at -inf; values checked {n_checked}")
    return b


# ---- (1) values -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [13, 11, 9])
@pytest.mark.parametrize("chem_name", list(VALUE_CHEMS))
def test_values_equal_the_model(eng, m, k, chem_name):
    pool, cls = pool_of(k, N_VALUES)
    chem = m.Chem.ntthal(**VALUE_CHEMS[chem_name])
    bt = m.capi.host_bound_tables(None, chem, THR)
    assert bt["usable"] == 1
    check_plane(eng, m, pool, cls, chem, bt, f"k={k} {chem_name}")


def test_values_with_self_complementary_oligos(eng, m):
    """12 bases: ATAT... and GCGC... are their own reverse complements -- those pairs stay at -inf whatever their size."""
    pool, cls = pool_of(12, N_VALUES)
    assert (cls == "sym").sum() == 4
    check_plane(eng, m, pool, cls, m.Chem.ntthal(), m.capi.host_bound_tables(None, m.Chem.ntthal(), THR), "k=12")


def test_values_long_loops_cheap(m, tmp_path):
    """A bundle under which long loops win the minimum: their table rows show in the values."""
    path = pv.write_bundle(long_loops_cheap_sections(), tmp_path / "long_loops_cheap.bundle")
    e = m.Engine(0, params_path=str(path))
    try:
        pool, cls = pool_of(13, N_VALUES)
        check_plane(e, m, pool, cls, m.Chem.ntthal(), m.capi.host_bound_tables(path, m.Chem.ntthal(), THR), "long_loops_cheap")
    finally:
        e.close()


# ---- (2) decisions and (3) counters ------------------------------------------------------------------------------------
def set_options(eng, bound, mirror, bound_list):
    eng.set_option("pair_bound", bound)
    eng.set_option("pair_mirror", mirror)
    eng.set_option("pair_bound_list", bound_list)


def read_stats(eng):
    eng.last_overflow_pairs()      # raises if a hand-over list, list U included, was overrun
    stats = eng.pair_stage_stats()
    stats["lists"] = eng.hand_over_lists()
    return stats


def screen(eng, pool, chem, bound_list, mirror="auto", bound=1, thr=THR):
    """Decisions of the whole pool: (bitmap as bool, row counts, statistics)."""
    set_options(eng, bound, mirror, bound_list)
    eng.pair_stage_stats()
    eng.hand_over_lists()
    try:
        out = eng.cross_dimer(pool, chem, thr, want_dg=False)
        stats = read_stats(eng)
    finally:
        set_options(eng, "auto", "auto", "auto")
    return bits(out["bitmap"], len(pool)), out["row_conflicts"], stats


def check_on_and_off(res, want, what):
    """res[1] / res[0]: (bitmap, counts, stats) with the stage on / off.  Both are the oracle's and bit-identical; the
    counters say the stage ran and that list 0 got shorter."""
    for mode in (1, 0):
        np.testing.assert_array_equal(res[mode][0], want, err_msg=f"{what} pair_bound_list={mode}")
        np.testing.assert_array_equal(res[mode][1], want.sum(1), err_msg=f"{what} pair_bound_list={mode}")
    np.testing.assert_array_equal(res[1][0], res[0][0])
    np.testing.assert_array_equal(res[1][1], res[0][1])
    on, off = res[1][2], res[0][2]
    print(f"{what}: U {on['bound_list_pairs']} entries, {on['bound_list_survivors']} ordered pairs handed on; "
          f"lists[0] {off['lists'][0]} -> {on['lists'][0]}; first-stage survivors {on['bound_survivors']}")
    assert off["bound_list_pairs"] == 0 and off["bound_list_survivors"] == 0
    assert on["bound_list_pairs"] > 0 and on["bound_list_survivors"] > 0
    assert on["lists"][0] < off["lists"][0]
    assert on["bound_survivors"] == off["bound_survivors"]      # the first stage's own survivors: unchanged
    assert on["lists"][0] >= on["bound_survivors"] + on["bound_list_survivors"]


def test_option_values(eng, m):
    assert eng.info("pair_bound_list") == 2
    for v, want in ((0, 0), (1, 1), ("auto", 2)):
        eng.set_option("pair_bound_list", v)
        assert eng.info("pair_bound_list") == want
    with pytest.raises(m.MsspeError):
        eng.set_option("pair_bound_list", 2)


@pytest.mark.parametrize("mirror", ["auto", 0])
def test_square_screen(eng, m, oracle, oracle_tables, mirror):
    pool, cls = pool_of(13, N_DECISIONS)
    n = len(pool)
    assert (cls == "u").sum() > 1000 and (cls == "over").sum() > 100 and (np.diag(cls) == "u").any()
    want = oracle_of(oracle, oracle_tables, pool, "square")
    res = {mode: screen(eng, pool, m.Chem.ntthal(), mode, mirror) for mode in (1, 0)}
    check_on_and_off(res, want, f"square pair_mirror={mirror}")
    assert res[1][2]["bound_mirrored"] == (n * (n - 1) // 2 if mirror == "auto" else 0)
    # every pair with 53..63 stored cells is on U: once per ordered pair without the mirror; under it, once per
    # unordered pair whichever order is filled -- counted here where both orders are of that class
    both = (cls == "u") & (cls.T == "u")
    n_diag = int(np.diag(both).sum())
    n_u = (int(both.sum()) - n_diag) // 2 + n_diag if mirror == "auto" else int((cls == "u").sum())
    assert n_u > 1000 and res[1][2]["bound_list_pairs"] >= n_u


def screen_block(eng, m, pool, rows, cols, bound_list):
    import torch
    n, k = len(pool), len(pool[0])
    nr, nc = rows[1] - rows[0], cols[1] - cols[0]
    words = (nc + 63) // 64
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    d_rc = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_bm = torch.zeros(nr * words, dtype=torch.int64, device="cuda")
    set_options(eng, 1, "auto", bound_list)
    eng.pair_stage_stats()
    eng.hand_over_lists()
    eng.synchronize()
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        eng.cross_dimer_dev(d_pool.data_ptr(), n, k, m.Chem.ntthal(), THR, rows, cols, d_rc.data_ptr(), d_bm.data_ptr())
        torch.cuda.synchronize()
    finally:
        eng.reset_stream()
        set_options(eng, "auto", "auto", "auto")
    stats = read_stats(eng)
    return bits(d_bm.cpu().numpy().reshape(nr, words).view(np.uint64), nc), d_rc.cpu().numpy()[rows[0]:rows[1]], stats


def test_row_block_inside_its_columns(eng, m, oracle, oracle_tables):
    """Rows (40, 200) of columns (10, n): a rank's row block, off the origin -- never mirrored, no twin bit."""
    pool, cls = pool_of(13, N_DECISIONS)
    rows, cols = (40, 200), (10, len(pool))
    assert (cls[rows[0]:rows[1], cols[0]:cols[1]] == "u").sum() > 1000
    want = oracle_of(oracle, oracle_tables, pool, "square")[rows[0]:rows[1], cols[0]:cols[1]]
    res = {mode: screen_block(eng, m, pool, rows, cols, mode) for mode in (1, 0)}
    check_on_and_off(res, want, "row block")
    assert res[1][2]["bound_mirrored"] == 0
    assert res[1][2]["bound_list_pairs"] >= int((cls[rows[0]:rows[1], cols[0]:cols[1]] == "u").sum())


def test_ab_screen(eng, m, oracle, oracle_tables):
    pool, cls = pool_of(13, N_DECISIONS)
    A, B = pool[:150], pool[150:]
    assert (cls[:150, 150:] == "u").sum() > 1000
    want = oracle_of(oracle, oracle_tables, pool, "square")[:150, 150:]
    res = {}
    for mode in (1, 0):
        set_options(eng, 1, "auto", mode)
        eng.pair_stage_stats()
        eng.hand_over_lists()
        try:
            out = eng.cross_dimer_ab(A, B, m.Chem.ntthal(), THR, want_dg=False)
            stats = read_stats(eng)
        finally:
            set_options(eng, "auto", "auto", "auto")
        res[mode] = (bits(out["bitmap"], len(B)), out["row_conflicts"], stats)
    check_on_and_off(res, want, "A/B")
    assert res[1][2]["bound_mirrored"] == 0


def test_asymmetric_bundle(m, oracle, tmp_path):
    """One stacked pair differs from its strand-swapped partner (mirror_ok = 0): every ordered pair on its own."""
    path = pv.write_bundle(broken_sections(), tmp_path / "broken.bundle")
    pool, _ = pool_of(13, N_DECISIONS)
    want = oracle_of(oracle, oracle.Tables(path), pool, "broken")
    e = m.Engine(0, params_path=str(path))
    try:
        res = {mode: screen(e, pool, m.Chem.ntthal(), mode) for mode in (1, 0)}
    finally:
        e.close()
    check_on_and_off(res, want, "asymmetric bundle")
    assert res[1][2]["bound_mirrored"] == 0


# ---- edge cases of list U ----------------------------------------------------------------------------------------------
# 8 A + 5 C ending in A against 8 T + 5 C ending in T: 64 cells, 56 stored, in both orders; among themselves no cell
def at_family(n_a, n_b, seed):
    rng = np.random.default_rng(seed)
    A = ["".join(rng.permutation(list("AAAAAAACCCCC"))) + "A" for _ in range(n_a)]
    B = ["".join(rng.permutation(list("TTTTTTTCCCCC"))) + "T" for _ in range(n_b)]
    for a in A:
        assert pair_class(a, B[0]) == "u" and pair_class(B[0], a) == "u" and pair_class(a, A[0]) == "none"
    assert pair_class(B[0], B[-1]) == "none"
    return A + B


@pytest.mark.parametrize("n_a,n_b,mirror,entries", [(1, 1, "auto", 1), (1, 1, 0, 2), (7, 73, "auto", BATCH - 1),
                                                    (16, 32, "auto", BATCH), (19, 27, "auto", BATCH + 1), (19, 27, 0, 2 * BATCH + 2)])
def test_list_lengths_round_the_batch_size(eng, m, oracle, oracle_tables, n_a, n_b, mirror, entries):
    """U of one entry, and of one fewer / exactly / one more than a batch of 512 (a short list runs at depth 1)."""
    pool = at_family(n_a, n_b, seed=n_a * 100 + n_b)
    _, _, cf, _ = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(), THR, want_dg=False)
    res = {mode: screen(eng, pool, m.Chem.ntthal(), mode, mirror) for mode in (1, 0)}
    for mode in (1, 0):
        np.testing.assert_array_equal(res[mode][0], cf.astype(bool))
        np.testing.assert_array_equal(res[mode][1], cf.sum(1))
    assert res[1][2]["bound_list_pairs"] == entries and res[0][2]["bound_list_pairs"] == 0
    assert res[0][2]["lists"][0] == 2 * n_a * n_b      # every pair with a cell was handed on for its size
    assert res[1][2]["lists"][0] == res[1][2]["bound_list_survivors"] <= 2 * n_a * n_b
    print(f"{n_a} x {n_b} pair_mirror={mirror}: U {entries}, handed on {res[1][2]['bound_list_survivors']}")


def test_empty_list(eng, m):
    """An {A, C}-only pool has no complementary cell at all: nothing on U, nothing on list 0, no conflict."""
    rng = np.random.default_rng(3)
    pool = ["".join(r) for r in rng.choice(list("AC"), size=(200, 13))]
    for mode in (1, 0):
        got, counts, stats = screen(eng, pool, m.Chem.ntthal(), mode)
        assert not got.any() and not counts.any()
        assert stats["bound_list_pairs"] == 0 and stats["bound_list_survivors"] == 0 and stats["lists"][0] == 0


def test_diagonal_entry(eng, m, oracle, oracle_tables):
    """10 A + 3 T ending in A: 60 cells with itself, 57 stored.  The diagonal pair is on U without a twin bit; at a cut it
    cannot be culled at, it is handed on once."""
    d = "AAAAAAAAATTTA"
    pool = [d, "C" * 13, "C" * 13, "C" * 13]
    assert pair_class(d, d) == "u" and pair_class(d, pool[1]) == "none"
    dg = oracle.thal(oracle_tables, d, d).dG
    thr = float(np.float32(min(dg + 500.0, 0.0)))      # the pair conflicts: no valid bound can cull it
    _, _, cf, _ = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(), thr, want_dg=False)
    assert cf[0, 0] and cf.sum() == 1
    for mirror in ("auto", 0):
        got, counts, stats = screen(eng, pool, m.Chem.ntthal(), 1, mirror, thr=thr)
        np.testing.assert_array_equal(got, cf.astype(bool))
        assert stats["bound_list_pairs"] == 1 and stats["bound_list_survivors"] == 1 and stats["lists"][0] == 1


_flush_pool = []


@pytest.mark.parametrize("mirror", ["auto", 0])
def test_several_flushes_reuse_the_list(eng, m, oracle, oracle_tables, mirror):
    """list_cap_log2 = 20 and 1,500 skewed oligos: several first-stage launches with flushes between them, so that
    ovf_list2 is list U, then an output list of the exact chain, then list U again."""
    if not _flush_pool:
        pool = skewed_pool(13, 1500, seed=8200, n_rich=0)[:1500]
        _flush_pool.append((pool, oracle_of(oracle, oracle_tables, pool, "flush")))
    pool, want = _flush_pool[0]
    eng.set_option("list_cap_log2", 20)
    eng.profile_enable(True)
    try:
        eng.profile_read()
        res = {mode: screen(eng, pool, m.Chem.ntthal(), mode, mirror) for mode in (1, 0)}
        launches, _ = eng.profile_read()
    finally:
        eng.profile_enable(False)
        eng.set_option("list_cap_log2", 0)
    assert launches >= 2 * 3
    check_on_and_off(res, want, f"1,500 oligos, list of 2^20, pair_mirror={mirror}")


def test_two_runs_give_the_same_counters(eng, m):
    pool, _ = pool_of(13, N_DECISIONS)
    runs = [screen(eng, pool, m.Chem.ntthal(), 1) for _ in range(2)]
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    assert runs[0][2] == runs[1][2] and runs[0][2]["bound_list_pairs"] > 0


@pytest.mark.parametrize("thr", [-3000.0, 0.0])
def test_auto_leaves_the_stage_off_with_the_bound_stage(eng, m, oracle, oracle_tables, thr):
    """At -3000 and 0 most pairs of a random pool survive the bound: pair_bound = auto runs the exact kernel, and list U
    stays empty."""
    pool = m.synth.pool_strings(m.synth.random_pool(640, 13, seed=713))
    _, _, cf, _ = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(), thr, want_dg=False)
    got, counts, stats = screen(eng, pool, m.Chem.ntthal(), "auto", bound="auto", thr=thr)
    np.testing.assert_array_equal(got, cf.astype(bool))
    np.testing.assert_array_equal(counts, cf.sum(1))
    assert stats["bound_survivors"] == 0 and stats["bound_list_pairs"] == 0 and stats["bound_list_survivors"] == 0
