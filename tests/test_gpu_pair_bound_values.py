"""The bound first stage's VALUES (csrc/thal_pairs_row.hip k_pairs_bound: build_bound_table, the generated scan
row_bound_pinned.inc, run_pair_bound) against tests/pair_bound_model.py, pair for pair and exactly.

A pair the stage culls gets no second look, and a bound that is wrongly too low or wrongly too high but still below
dG passes every decision test.  msspe_cross_dimer_bound_dev writes the stage's value of every pair: +inf (no chain),
-inf (not bounded there: handed on) or (pick + init) / 64.  The model divides the same int32 by 64, so the comparison
is == on float64, with no tolerance.  The model itself is pinned to the oracle on the CPU (test_pair_bound_model.py).

(a) mixed pools at every length 2 .. 13; (b) column blocks of one base composition, where the stage must bound every
pair the sizing rule of wave_pairs_row lets it (pair_bound_model.bounded_in_uniform_wave); (c) constructed two-stem
pairs whose winning chains take many loop shapes, under the stock tables and under a bundle that makes long loops
cheap; (d) the corners of the chemistry domain; (e) decisions at every length; (f) block shapes round the mirror
condition of run_chain (row0 == col0 && row1 == col1).  Every decision is compared with the oracle's."""
import numpy as np
import pytest

import param_variants as pv
import test_gpu_pair_mirror as mirror_tests      # its 700-oligo pool and oracle plane: computed once for both files
from pair_bound_model import (EDGE_CHEMS, SLOTS, UNUSABLE_CHEMS, bound_pair, bound_pair_trace, bounded_in_uniform_wave,
                              long_loops_cheap_sections, mixed_pool, stored_cells, two_stem_family)

pytestmark = pytest.mark.gpu

THR = -9000.0
MARKER = 12345.0
KS = tuple(range(2, 14))
N_RANDOM = 96


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cheap(m, oracle, tmp_path_factory):
    """The long-loop bundle: (its engine, an oracle Tables on the same file, its path)."""
    path = pv.write_bundle(long_loops_cheap_sections(), tmp_path_factory.mktemp("tables") / "long_loops_cheap.bundle")
    e = m.Engine(0, params_path=str(path))
    yield e, oracle.Tables(path), path
    e.close()


bits = mirror_tests.bits
_pools, _oracle = {}, {}


def pool_of(k):
    if k not in _pools:
        _pools[k] = mixed_pool(k, N_RANDOM, seed=5200 + k)
    return _pools[k]


def oracle_of(oracle, oracle_tables, k, chem_name):
    """The oracle's dG plane of the mixed pool: once per (length, chemistry), shared and left unchanged."""
    if (k, chem_name) not in _oracle:
        kw = {**EDGE_CHEMS, **UNUSABLE_CHEMS, "ntthal25": {}}[chem_name]
        _, dg, _, _ = oracle.pool_pairs(oracle_tables, pool_of(k), oracle.ntthal_args(**kw), THR)
        dg.setflags(write=False)
        _oracle[(k, chem_name)] = dg
    return _oracle[(k, chem_name)]


def threshold_of(dg):
    """The float32 value of the 2nd percentile of the oracle's finite dG values; 0 where that is positive (the stage
    runs for cuts <= 0 only)."""
    thr = float(np.float32(np.percentile(dg[np.isfinite(dg)], 2)))
    return thr if thr < 0.0 else 0.0


def device_plane(eng, m, pool, chem, rows, cols, thr=THR):
    """The stage's value of every pair of the block; the plane is pre-filled with a marker that must be gone."""
    import torch
    n, k = len(pool), len(pool[0])
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    d_b = torch.full((rows[1] - rows[0], cols[1] - cols[0]), MARKER, dtype=torch.float64, device="cuda")
    eng.synchronize()
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        eng.cross_dimer_bound_dev(d_pool.data_ptr(), n, k, chem, thr, rows, cols, d_b.data_ptr())
        torch.cuda.synchronize()
    finally:
        eng.reset_stream()
    b = d_b.cpu().numpy()
    assert not (b == MARKER).any()
    assert not np.isnan(b).any()
    return b


def model_plane(bt, rows, cols, only=None):
    """bound_pair of every (row, column) oligo pair, +inf for "no chain"; only: a boolean mask of the pairs to compute
    (NaN elsewhere).  Equal pairs are computed once."""
    want = np.full((len(rows), len(cols)), np.nan)
    memo = {}
    for i, a in enumerate(rows):
        for j, b in enumerate(cols):
            if only is not None and not only[i, j]:
                continue
            if (a, b) not in memo:
                lb = bound_pair(bt, a, b)
                memo[(a, b)] = np.inf if lb is None else lb
            want[i, j] = memo[(a, b)]
    return want


def check_values(b, want, what=""):
    """Wherever the plane is finite it is the model's value; +inf only where the model has no chain; where the model has
    no chain the plane is +inf or -inf.  (Pairs whose model value was not computed, NaN, are left out.)"""
    known = ~np.isnan(want)
    fin = np.isfinite(b) & known
    np.testing.assert_array_equal(b[fin], want[fin], err_msg=f"{what}: a bounded pair's value")
    assert (want[(b == np.inf) & known] == np.inf).all(), f"{what}: +inf where the model has a chain"
    assert not np.isfinite(b[(want == np.inf)]).any(), f"{what}: a value where the model has no chain"
    return fin


def screen(eng, pool, chem, thr, bound, mirror):
    """Decisions of the whole pool with pair_bound = bound and pair_mirror = mirror: (bitmap as bool, counts, statistics)."""
    eng.set_option("pair_bound", bound)
    eng.set_option("pair_mirror", mirror)
    eng.pair_stage_stats()
    try:
        out = eng.cross_dimer(pool, chem, thr, want_dg=False)
        eng.last_overflow_pairs()      # raises if a hand-over list was overrun
    finally:
        eng.set_option("pair_bound", "auto")
        eng.set_option("pair_mirror", "auto")
    return bits(out["bitmap"], len(pool)), out["row_conflicts"], eng.pair_stage_stats()


def check_decisions(eng, m, pool, chem, thr, dg, bounds=(1, 0), mirrors=("auto", 0)):
    """Bitmap and counts are the oracle's under every setting; the counters say which stage ran."""
    n = len(pool)
    want = dg <= m.g_cut(thr)
    res = {}
    for bound in bounds:
        for mirror in mirrors:
            got, counts, stats = screen(eng, pool, chem, thr, bound, mirror)
            np.testing.assert_array_equal(got, want, err_msg=f"pair_bound={bound} pair_mirror={mirror}")
            np.testing.assert_array_equal(counts, want.sum(1).astype(np.uint32), err_msg=f"pair_bound={bound} pair_mirror={mirror}")
            if bound == 0:
                assert stats["bound_survivors"] == 0 and stats["bound_mirrored"] == 0
            if mirror == 0:
                assert stats["bound_mirrored"] == 0
            res[(bound, mirror)] = stats
            res["bitmap"] = got
    return want, res


# ---- (a) mixed pools, every length ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_mixed_pool_values_equal_the_model(eng, m, oracle, oracle_tables, k):
    pool = pool_of(k)
    n = len(pool)
    b = device_plane(eng, m, pool, m.Chem.ntthal(), (0, n), (0, n))
    want = model_plane(m.capi.host_bound_tables(None, m.Chem.ntthal(), THR), pool, pool)
    fin = check_values(b, want, f"k={k}")
    # (waves of a pool this small mix compositions and shed lanes: no bounded share is asserted here, see the blocks below)
    dg = oracle_of(oracle, oracle_tables, k, "ntthal25")
    both = fin & np.isfinite(dg)
    print(f"k={k}: {int((b != -np.inf).sum())} of {n * n} pairs bounded ({(b != -np.inf).mean():.4f}), {int(fin.sum())} with a value, "
          f"worst lb - dG = {np.max(b[both] - dg[both]):.4f} cal/mol")
    assert fin.any()


# ---- (b) one composition per column block: the stage must bound everything it can --------------------------------------
BLOCKS = {13: ((3, 3, 3, 4), (1, 5, 5, 2), (6, 1, 1, 5), (0, 0, 0, 13)), 8: ((2, 2, 2, 2),), 5: ((1, 1, 1, 2),)}
N_COLS = 130      # two full waves and a partial one


def block_pool(k, comp):
    """(the row oligos: 64 random ones and the specials, 130 seeded permutations of the column multiset)."""
    rng = np.random.default_rng(6100 + k + sum(c * 17 ** q for q, c in enumerate(comp)))
    base = np.array(list("".join(x * c for x, c in zip("ACGT", comp))))
    return mixed_pool(k, 64, seed=6000 + k), ["".join(rng.permutation(base)) for _ in range(N_COLS)]


def test_the_blocks_hold_what_they_are_for():
    """From the rule alone, before the device is asked: every block has at least 1,000 pairs it calls bounded, and one
    block at least has a pair handed on for its size."""
    for_size = 0
    for k, comps in BLOCKS.items():
        for comp in comps:
            rows, cols = block_pool(k, comp)
            ok = np.array([[bounded_in_uniform_wave(a, b) for b in cols] for a in rows])
            assert ok.sum() >= 1000, (k, comp)
            for_size += sum(stored_cells(a, b) > SLOTS for a in rows for b in cols)
    assert for_size > 0


@pytest.mark.parametrize("k,comp", [(k, comp) for k, comps in BLOCKS.items() for comp in comps])
def test_uniform_column_blocks_are_bounded_exactly_where_the_rule_says(eng, m, k, comp):
    rows, cols = block_pool(k, comp)
    R = len(rows)
    b = device_plane(eng, m, rows + cols, m.Chem.ntthal(), (0, R), (R, R + N_COLS))
    ok = np.array([[bounded_in_uniform_wave(x, y) for y in cols] for x in rows])
    np.testing.assert_array_equal(b != -np.inf, ok, err_msg="the pairs handed on unbounded are not the sizing rule's")
    want = model_plane(m.capi.host_bound_tables(None, m.Chem.ntthal(), THR), rows, cols, only=ok)
    np.testing.assert_array_equal(b[ok], want[ok])
    print(f"k={k} {comp}: {int(ok.sum())} of {ok.size} pairs bounded, {int(np.isfinite(b).sum())} with a value")


# ---- (c) the two-stem family: stock tables and the long-loop bundle ---------------------------------------------------
def check_family_values(e, m, path):
    fam = two_stem_family()
    n = len(fam)
    A, B = [a for a, _ in fam], [b for _, b in fam]
    bt = m.capi.host_bound_tables(path, m.Chem.ntthal(), THR)
    b = device_plane(e, m, A + B, m.Chem.ntthal(), (0, n), (n, 2 * n))
    # (every a against every b: 287,296 pairs, but a few thousand different ones)
    check_values(b, model_plane(bt, A, B), "family")
    shapes = set()
    for i, (x, y) in enumerate(fam):
        lb, tr = bound_pair_trace(bt, x, y)
        shapes.update(tr)
        # every family pair: its value, or handed on for its size
        if b[i, i] == -np.inf:
            assert stored_cells(x, y) > SLOTS, (x, y, stored_cells(x, y))
        else:
            assert b[i, i] == lb, (x, y, b[i, i], lb)
    print(f"family: {int(np.isfinite(np.diag(b)).sum())} of {n} family pairs with a value, their chains use {len(shapes)} "
          f"loop shapes, longest side {max(max(s) for s in shapes)}; {int((b == -np.inf).sum())} of {b.size} pairs of the block not bounded")
    return A + B


def test_family_values_stock(eng, m):
    check_family_values(eng, m, None)


def test_family_values_and_decisions_long_loops_cheap(m, oracle, cheap):
    e, tables, path = cheap
    pool = check_family_values(e, m, path)
    n = len(pool)
    _, dg, _, _ = oracle.pool_pairs(tables, pool, oracle.ntthal_args(), THR)
    want, res = check_decisions(e, m, pool, m.Chem.ntthal(), THR, dg)
    fam_conflicts = int(np.diag(want[:n // 2, n // 2:]).sum())
    print(f"long_loops_cheap: {int(want.sum())} conflicts, {fam_conflicts} among the family pairs, "
          f"survivors {res[(1, 'auto')]['bound_survivors']} mirrored / {res[(1, 0)]['bound_survivors']} not")
    assert fam_conflicts > 0 and fam_conflicts < n // 2
    assert res[(1, "auto")]["bound_survivors"] > 0 and res[(1, 0)]["bound_survivors"] > 0
    assert res[(1, "auto")]["bound_mirrored"] == n * (n - 1) // 2


# ---- (d) the corners of the chemistry domain ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [13, 7])
@pytest.mark.parametrize("chem_name", list(EDGE_CHEMS))
def test_chemistry_edges(eng, m, oracle, oracle_tables, k, chem_name):
    pool = pool_of(k)
    n = len(pool)
    chem = m.Chem.ntthal(**EDGE_CHEMS[chem_name])
    dg = oracle_of(oracle, oracle_tables, k, chem_name)
    thr = threshold_of(dg)
    bt = m.capi.host_bound_tables(None, chem, thr)
    assert bt["usable"] == 1
    b = device_plane(eng, m, pool, chem, (0, n), (0, n), thr)
    fin = check_values(b, model_plane(bt, pool, pool), f"k={k} {chem_name}")
    both = fin & np.isfinite(dg)
    want, res = check_decisions(eng, m, pool, chem, thr, dg, mirrors=("auto",))
    print(f"k={k} {chem_name}: threshold {thr}, {int(want.sum())} conflicts, survivors {res[(1, 'auto')]['bound_survivors']}, "
          f"{int((b != -np.inf).sum())} of {n * n} pairs bounded, worst lb - dG = {np.max(b[both] - dg[both]):.4f} cal/mol")
    if thr < 0.0:
        assert want.any() and (~want & np.isfinite(dg)).any()
    elif not want.any():
        assert not res["bitmap"].any()


@pytest.mark.parametrize("k", [13, 7])
@pytest.mark.parametrize("chem_name", list(UNUSABLE_CHEMS))
def test_unusable_chemistries_screen_without_the_bound(eng, m, oracle, oracle_tables, k, chem_name):
    """Outside 0 .. 100 C build_bound_tables declines: pair_bound = 1 screens with the exact stages alone, and the
    diagnostic plane refuses."""
    pool = pool_of(k)
    n = len(pool)
    chem = m.Chem.ntthal(**UNUSABLE_CHEMS[chem_name])
    dg = oracle_of(oracle, oracle_tables, k, chem_name)
    thr = threshold_of(dg)
    assert m.capi.host_bound_tables(None, chem, thr)["usable"] == 0
    _, res = check_decisions(eng, m, pool, chem, thr, dg, bounds=(1,), mirrors=("auto",))
    assert res[(1, "auto")]["bound_survivors"] == 0 and res[(1, "auto")]["bound_mirrored"] == 0
    import torch
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    d_b = torch.full((n, n), MARKER, dtype=torch.float64, device="cuda")
    eng.synchronize()
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        with pytest.raises(m.MsspeError):
            eng.cross_dimer_bound_dev(d_pool.data_ptr(), n, k, chem, thr, (0, n), (0, n), d_b.data_ptr())
        torch.cuda.synchronize()
    finally:
        eng.reset_stream()
    assert (d_b.cpu().numpy() == MARKER).all()


# ---- (e) every length, decisions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_decisions_at_every_length(eng, m, oracle, oracle_tables, k):
    pool = pool_of(k)
    n = len(pool)
    dg = oracle_of(oracle, oracle_tables, k, "ntthal25")
    thr = threshold_of(dg)
    want, res = check_decisions(eng, m, pool, m.Chem.ntthal(), thr, dg, bounds=(1, 0, "auto"))
    print(f"k={k}: threshold {thr}, {int(want.sum())} conflicts, survivors {res[(1, 'auto')]['bound_survivors']} forced / "
          f"{res[('auto', 'auto')]['bound_survivors']} auto")
    assert res[(1, "auto")]["bound_mirrored"] == n * (n - 1) // 2
    # pair_bound = auto runs the stage, mirrored, or leaves the screen to the exact kernel
    assert res[("auto", "auto")]["bound_mirrored"] in (0, n * (n - 1) // 2)
    if thr < 0.0:
        assert want.any() and (~want & np.isfinite(dg)).any()


# ---- (f) block shapes round the mirror condition -----------------------------------------------------------------------
GUARD_WORD, GUARD = 0x5A5A5A5A5A5A5A5A, 4096


def screen_block(eng, m, pool, rows, cols):
    """cross_dimer_dev of one block with pair_bound = 1, the bitmap between guard words: (bitmap as bool, all n row
    counts, statistics)."""
    import torch
    n, k = len(pool), len(pool[0])
    nr, nc = rows[1] - rows[0], cols[1] - cols[0]
    words = (nc + 63) // 64
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    d_rc = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_bm = torch.full((2 * GUARD + nr * words,), GUARD_WORD, dtype=torch.int64, device="cuda")
    eng.set_option("pair_bound", 1)
    eng.pair_stage_stats()
    eng.synchronize()
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        eng.cross_dimer_dev(d_pool.data_ptr(), n, k, m.Chem.ntthal(), THR, rows, cols, d_rc.data_ptr(),
                            d_bm.data_ptr() + 8 * GUARD)
        torch.cuda.synchronize()
    finally:
        eng.reset_stream()
        eng.set_option("pair_bound", "auto")
    eng.last_overflow_pairs()
    g_bm = d_bm.cpu().numpy()
    assert (g_bm[:GUARD] == GUARD_WORD).all() and (g_bm[-GUARD:] == GUARD_WORD).all()
    return (bits(g_bm[GUARD:-GUARD].reshape(nr, words).view(np.uint64), nc), d_rc.cpu().numpy().astype(np.int64),
            eng.pair_stage_stats())


def check_block(eng, m, oracle, oracle_tables, rows, cols):
    pool = mirror_tests.pool_of(m, oracle, oracle_tables, 13)
    dg = mirror_tests.oracle_of(m, oracle, oracle_tables, 13, "ntthal25")
    want = dg[rows[0]:rows[1], cols[0]:cols[1]] <= m.g_cut(THR)
    got, counts, stats = screen_block(eng, m, pool, rows, cols)
    np.testing.assert_array_equal(got, want)
    rc = np.zeros(len(pool), dtype=np.int64)
    rc[rows[0]:rows[1]] = want.sum(1)
    np.testing.assert_array_equal(counts, rc)      # the block's rows, and nothing outside them
    return want, stats


@pytest.mark.parametrize("size", [1, 63, 64, 65, 300])
def test_square_block_off_the_origin_is_mirrored(eng, m, oracle, oracle_tables, size):
    """rows = cols = (130, 130 + size): rows are sorted positions and pool indices come back through perm, so the
    block's offset must not matter."""
    want, stats = check_block(eng, m, oracle, oracle_tables, (130, 130 + size), (130, 130 + size))
    assert stats["bound_mirrored"] == size * (size - 1) // 2
    if size == 300:
        assert want.any() and stats["bound_survivors"] > 0


@pytest.mark.parametrize("rows", [(0, 350), (350, 700)])
def test_a_ranks_row_block_is_not_mirrored(eng, m, oracle, oracle_tables, rows):
    """row0 == col0 only, row1 == col1 only: a rank's row block against the whole pool runs every ordered pair."""
    want, stats = check_block(eng, m, oracle, oracle_tables, rows, (0, mirror_tests.N_POOL))
    assert stats["bound_mirrored"] == 0 and stats["bound_survivors"] > 0 and want.any()
