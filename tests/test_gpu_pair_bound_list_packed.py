"""The packed bound list stage on the device (option pair_bound_list_packed; csrc/thal_pairs_bound_list.hip
k_pairs_bound_list_packed, capi.cpp run_chain).

Values: msspe_cross_dimer_bound_list_packed_dev runs the packed instances of both stages; every value is the integer of
tests/pair_bound_packed_model.py on the coarse tables of msspe_host_bound_packed times the unit, == on float64, every
pair of every plane; -inf and +inf exactly where pair_bound_list_model.class_plane says.  Decisions: the oracle's under
every setting; with the packed list stage on, list 0 is the same whether the first stage is the packed or the windowed
instance (every first-stage survivor then meets the packed bound); with it off, every counter is the exact-unit route's:
checked here as auto == 0 on screens below auto's limit; that this route's counts are what they were before the packed
instance existed is pinned by test_gpu_pair_bound_list.py, -packed.py and -window.py, which run under auto at such sizes.
List U of every size round a pass of 1,024 and a run of 7 passes, a screen whose batches run at depth 2 and more, a
hand-over list of 2^20 entries against the exact-unit stage, identical counters on identical runs, and a bundle the packed units cannot hold."""
import numpy as np
import pytest

import param_variants as pv
import test_gpu_pair_bound_list as bl      # its skewed pools and the oracle's conflicts: computed once for the files that share them
from pair_bound_list_model import class_plane, n_cells, pair_class, skewed_pool
from pair_bound_model import stored_cells
from pair_bound_packed_model import NONE, packed_tables, plane_model, unpackable_sections

pytestmark = pytest.mark.gpu

THR = -9000.0
MARKER = 12345.0
PASS = 1024      # thal_pairs_bound_list.hip kPLThreads: entries per pass of the packed instance


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
def pk(m):
    p = packed_tables(m)
    assert p["usable"] == 1
    return p


def test_option_values(eng, m):
    assert eng.info("pair_bound_list_packed") == 2
    for v, want in ((0, 0), (1, 1), ("auto", 2)):
        eng.set_option("pair_bound_list_packed", v)
        assert eng.info("pair_bound_list_packed") == want
    with pytest.raises(m.MsspeError):
        eng.set_option("pair_bound_list_packed", 2)


# ---- the plane ---------------------------------------------------------------------------------------------------------
def list_planes(eng, m, pool, rows, cols, thr=THR):
    """(the packed list plane, the exact-unit list plane) of the block; pre-filled with a marker that must be gone."""
    import torch
    n, k = len(pool), len(pool[0])
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    out = []
    eng.synchronize()
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for call in (eng.cross_dimer_bound_list_packed_dev, eng.cross_dimer_bound_list_dev):
            d_b = torch.full((rows[1] - rows[0], cols[1] - cols[0]), MARKER, dtype=torch.float64, device="cuda")
            call(d_pool.data_ptr(), n, k, m.Chem.ntthal(), thr, rows, cols, d_b.data_ptr())
            torch.cuda.synchronize()
            out.append(d_b.cpu().numpy())
    finally:
        eng.reset_stream()
    for b in out:
        assert not (b == MARKER).any() and not np.isnan(b).any()
    return out


def check_list_plane(eng, m, pk, pool, rows, cols, what):
    R, Cc = pool[rows[0]:rows[1]], pool[cols[0]:cols[1]]
    b, exact = list_planes(eng, m, pool, rows, cols)
    cls = class_plane(R, Cc)
    pick, vmin, vmax = plane_model(pk, R, Cc)
    assert vmin == NONE or (pk["lo"] <= vmin and vmax <= pk["hi"])
    want = np.where(pick == NONE, np.inf, (pick + pk["init"]) * pk["unit"])
    np.testing.assert_array_equal(b == -np.inf, (cls == "sym") | (cls == "over"), err_msg=f"{what}: -inf")
    np.testing.assert_array_equal(b == np.inf, cls == "none", err_msg=f"{what}: +inf")
    np.testing.assert_array_equal(b == -np.inf, exact == -np.inf)
    fin = np.isfinite(b)
    np.testing.assert_array_equal(b[fin], want[fin], err_msg=f"{what}: a bounded pair's value")
    assert (b[fin] <= exact[fin]).all() and (exact[fin] - b[fin] < 27 * pk["unit"]).all(), what
    print(f"{what}: {int(fin.sum())} values == the model's, {int((cls == 'u').sum())} of them with 53..63 stored cells, "
          f"{int((b == -np.inf).sum())} at -inf")
    return b, cls


def test_square_plane_equals_the_model(eng, m, pk):
    pool, cls = bl.pool_of(13, bl.N_VALUES)
    assert (cls == "u").sum() > 1000 and (cls == "over").sum() > 50 and (cls == "none").sum() > 0
    check_list_plane(eng, m, pk, pool, (0, len(pool)), (0, len(pool)), "square")


def test_off_origin_block_plane_equals_the_model(eng, m, pk):
    pool, cls = bl.pool_of(13, bl.N_VALUES)
    rows, cols = (37, 150), (61, len(pool))
    assert (cls[rows[0]:rows[1], cols[0]:cols[1]] == "u").sum() > 500
    check_list_plane(eng, m, pk, pool, rows, cols, "A x B block off the origin")


def test_plane_of_the_table_sizes_at_the_edges(eng, m, pk):
    """One cell; exactly 63 stored cells (the last the table holds); 66 stored cells and all A against all T (passed on:
    -inf)."""
    a = "AAAAAAAAACCCA"
    rng = np.random.default_rng(63)
    b63 = ["".join(rng.permutation(list("TTTTTTTCCCCCC"))) for _ in range(70)]
    b66 = ["".join(rng.permutation(list("TTTTTTTGCCCCC"))) for _ in range(5)]
    one = ["ACCCCCCCCCCCC", "TCCCCCCCCCCCC"]
    pool = [a] + b63 + b66 + one + ["A" * 13, "T" * 13]
    assert all(stored_cells(a, b) == 63 and pair_class(a, b) == "u" for b in b63)
    assert all(stored_cells(a, b) == 66 and pair_class(a, b) == "over" for b in b66)
    assert n_cells(one[0], one[1]) == 1 and pair_class("A" * 13, "T" * 13) == "over"
    b, cls = check_list_plane(eng, m, pk, pool, (0, len(pool)), (0, len(pool)), "edge sizes")
    assert np.isfinite(b[0, 1:71]).all() and (b[0, 71:76] == -np.inf).all() and np.isfinite(b[76, 77])
    assert b[78, 79] == -np.inf


def test_plane_with_self_complementary_oligos(eng, m, pk):
    """12 bases: ATAT... and GCGC... are their own reverse complements -- those pairs stay at -inf whatever their size."""
    pool, cls = bl.pool_of(12, bl.N_VALUES)
    assert (cls == "sym").sum() == 4 and (cls == "u").sum() > 100
    check_list_plane(eng, m, pk, pool, (0, len(pool)), (0, len(pool)), "k=12")


# ---- decisions ---------------------------------------------------------------------------------------------------------
EXTRA = ("pair_bound_list_packed", "pair_bound_window", "pair_bound_packed", "list_cap_log2")


def with_options(eng, opts, fn):
    """fn() under the options (reset afterwards; bl's helpers set and reset pair_bound, pair_mirror and pair_bound_list)."""
    for key, v in opts.items():
        assert key in EXTRA
        eng.set_option(key, v)
    try:
        return fn()
    finally:
        for key in opts:
            eng.set_option(key, 0 if key == "list_cap_log2" else "auto")


def run_shape(eng, m, pool, shape, mirror):
    n = len(pool)
    if shape == "square":
        return bl.screen(eng, pool, m.Chem.ntthal(), 1, mirror)
    if shape == "row_block":
        return bl.screen_block(eng, m, pool, (40, 200), (10, n), 1)      # (never mirrored)
    bl.set_options(eng, 1, mirror, 1)
    eng.pair_stage_stats()
    eng.hand_over_lists()
    try:
        out = eng.cross_dimer_ab(pool[:150], pool[150:], m.Chem.ntthal(), THR, want_dg=False)
        stats = bl.read_stats(eng)
    finally:
        bl.set_options(eng, "auto", "auto", "auto")
    return bl.bits(out["bitmap"], n - 150), out["row_conflicts"], stats


def want_shape(want, shape, n):
    return want if shape == "square" else (want[40:200, 10:n] if shape == "row_block" else want[:150, 150:])


@pytest.mark.parametrize("mirror", ["auto", 0])
@pytest.mark.parametrize("shape", ["square", "row_block", "ab"])
def test_decisions_are_the_oracles_under_every_setting(eng, m, oracle, oracle_tables, shape, mirror):
    pool, _ = bl.pool_of(13, bl.N_DECISIONS)
    n = len(pool)
    assert n == 323
    want = want_shape(bl.oracle_of(oracle, oracle_tables, pool, "square"), shape, n)
    res = {}
    for packed in (0, 1, "auto"):
        for window in (0, 1):
            res[packed, window] = with_options(eng, {"pair_bound_list_packed": packed, "pair_bound_window": window},
                                               lambda: run_shape(eng, m, pool, shape, mirror))
    for key, (got, counts, stats) in res.items():
        np.testing.assert_array_equal(got, want, err_msg=f"{shape} pair_mirror={mirror} (packed, window)={key}")
        np.testing.assert_array_equal(counts, want.sum(1), err_msg=f"{shape} pair_mirror={mirror} (packed, window)={key}")
        assert stats["bound_list_pairs"] > 0
    for window in (0, 1):
        off, on, auto = res[0, window][2], res[1, window][2], res["auto", window][2]
        # a screen this small: auto is the exact-unit list stage, counter for counter
        assert auto == off
        # the coarser bound culls no pair the exact-unit bound keeps: list 0 can only grow; list U and the first stage do not move
        assert on["bound_list_pairs"] == off["bound_list_pairs"] and on["bound_survivors"] == off["bound_survivors"]
        assert on["bound_list_survivors"] >= off["bound_list_survivors"] and on["lists"][0] >= off["lists"][0]
    # packed list stage on: every first-stage survivor of the windowed route meets the packed bound -- list 0 is what the
    # packed first stage and its list stage leave, entry for entry in number
    assert res[1, 1][2]["lists"][0] == res[1, 0][2]["lists"][0]
    assert res[0, 1][2]["lists"][0] <= res[0, 0][2]["lists"][0]
    print(f"{shape} pair_mirror={mirror}: lists[0] exact list stage {res[0, 0][2]['lists'][0]} (window: {res[0, 1][2]['lists'][0]}), "
          f"packed list stage {res[1, 0][2]['lists'][0]} (window: {res[1, 1][2]['lists'][0]})")


# ---- list U of every size ----------------------------------------------------------------------------------------------
def test_empty_list(eng, m):
    rng = np.random.default_rng(3)
    pool = ["".join(r) for r in rng.choice(list("AC"), size=(200, 13))]
    got, counts, stats = with_options(eng, {"pair_bound_list_packed": 1}, lambda: bl.screen(eng, pool, m.Chem.ntthal(), 1))
    assert not got.any() and not counts.any()
    assert stats["bound_list_pairs"] == 0 and stats["bound_list_survivors"] == 0 and stats["lists"][0] == 0


@pytest.mark.parametrize("n_a,n_b,entries", [(1, 1, 1), (33, 31, PASS - 1), (32, 32, PASS), (25, 41, PASS + 1),
                                             (3, 2389, 7 * PASS - 1), (64, 112, 7 * PASS), (67, 107, 7 * PASS + 1)])
def test_list_lengths_round_a_pass_and_seven(eng, m, oracle, oracle_tables, n_a, n_b, entries):
    """at_family: every (A, B) pair has 56 stored cells, A x A and B x B none -- under the mirror list U holds exactly
    n_a x n_b entries."""
    assert n_a * n_b == entries
    pool = bl.at_family(n_a, n_b, seed=n_a * 100 + n_b)
    res = {p: with_options(eng, {"pair_bound_list_packed": p}, lambda: bl.screen(eng, pool, m.Chem.ntthal(), 1, "auto"))
           for p in (1, 0)}
    if len(pool) <= 200:
        _, _, cf, _ = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(), THR, want_dg=False)
        np.testing.assert_array_equal(res[0][0], cf.astype(bool))
    np.testing.assert_array_equal(res[1][0], res[0][0])
    np.testing.assert_array_equal(res[1][1], res[0][1])
    for p in (1, 0):
        assert res[p][2]["bound_list_pairs"] == entries
        assert res[p][2]["lists"][0] == res[p][2]["bound_list_survivors"] <= 2 * entries
    assert res[1][2]["bound_list_survivors"] >= res[0][2]["bound_list_survivors"]
    print(f"{n_a} x {n_b}: U {entries}, handed on {res[1][2]['bound_list_survivors']} packed / {res[0][2]['bound_list_survivors']} exact")


_deep = []


def deep_pool(oracle, oracle_tables):
    if not _deep:
        pool = skewed_pool(13, 2000, seed=8300, n_rich=0)[:2000]
        _deep.append((pool, bl.oracle_of(oracle, oracle_tables, pool, "deep")))
    return _deep[0]


def test_batches_of_depth_two_and_more(eng, m, oracle, oracle_tables):
    """2,000 skewed oligos: list U holds more entries than one pass of every block (n_cu x 1,024), so every block sorts
    batches of depth >= 2."""
    pool, want = deep_pool(oracle, oracle_tables)
    got, counts, stats = with_options(eng, {"pair_bound_list_packed": 1}, lambda: bl.screen(eng, pool, m.Chem.ntthal(), 1, "auto"))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(counts, want.sum(1))
    assert stats["bound_list_pairs"] > eng.info("n_cu") * PASS
    print(f"2,000 oligos: U {stats['bound_list_pairs']} entries on {eng.info('n_cu')} blocks, handed on {stats['bound_list_survivors']}")


# ---- edge cases --------------------------------------------------------------------------------------------------------
def screen_raw(eng, pool, chem, mirror="auto"):
    """bl.screen without the overrun check: (bitmap, counts, overflow error or None, bound list counters)."""
    bl.set_options(eng, 1, mirror, 1)
    eng.pair_stage_stats()
    try:
        out = eng.cross_dimer(pool, chem, THR, want_dg=False)
        err = None
        try:
            eng.last_overflow_pairs()
        except Exception as e:      # noqa: BLE001 -- whatever the binding raises for an overrun list: both stages must raise alike
            err = type(e).__name__
        stats = eng.pair_stage_stats()
    finally:
        bl.set_options(eng, "auto", "auto", "auto")
    return bl.bits(out["bitmap"], len(pool)), out["row_conflicts"], err, stats


def test_list_of_2_to_the_20_behaves_as_under_the_exact_stage(eng, m, oracle, oracle_tables):
    """list_cap_log2 = 20 on the 2,000-oligo pool: flushes between the launches, list U reused by the exact chain and
    refilled.  Whatever the exact-unit stage does at that capacity -- an overrun included -- the packed one does too."""
    pool, want = deep_pool(oracle, oracle_tables)
    res = {p: with_options(eng, {"pair_bound_list_packed": p, "list_cap_log2": 20}, lambda: screen_raw(eng, pool, m.Chem.ntthal()))
           for p in (1, 0)}
    assert res[1][2] == res[0][2]
    if res[0][2] is None:
        for p in (1, 0):
            np.testing.assert_array_equal(res[p][0], want)
            np.testing.assert_array_equal(res[p][1], want.sum(1))
    assert res[1][3]["bound_list_pairs"] == res[0][3]["bound_list_pairs"] > 0


def test_two_runs_give_the_same_counters(eng, m):
    pool, _ = bl.pool_of(13, bl.N_DECISIONS)
    runs = [with_options(eng, {"pair_bound_list_packed": 1}, lambda: bl.screen(eng, pool, m.Chem.ntthal(), 1)) for _ in range(2)]
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    assert runs[0][2] == runs[1][2] and runs[0][2]["bound_list_pairs"] > 0


def test_a_bundle_whose_range_fits_no_unit_runs_the_exact_stage(m, oracle, tmp_path):
    path = pv.write_bundle(unpackable_sections(), tmp_path / "unpackable.bundle")
    assert m.capi.host_bound_packed(path)["usable"] == 0 and m.capi.host_bound_tables(path)["usable"] == 1
    pool, _ = bl.pool_of(13, bl.N_DECISIONS)
    want = bl.oracle_of(oracle, oracle.Tables(path), pool, "unpackable")
    e = m.Engine(0, params_path=str(path))
    try:
        res = {p: with_options(e, {"pair_bound_list_packed": p}, lambda: bl.screen(e, pool, m.Chem.ntthal(), 1)) for p in (0, 1, "auto")}
        import torch
        d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
        d_b = torch.zeros((len(pool), len(pool)), dtype=torch.float64, device="cuda")
        with pytest.raises(m.MsspeError):
            e.cross_dimer_bound_list_packed_dev(d_pool.data_ptr(), len(pool), 13, m.Chem.ntthal(), THR, (0, len(pool)),
                                                (0, len(pool)), d_b.data_ptr())
    finally:
        e.close()
    for p, (got, counts, stats) in res.items():
        np.testing.assert_array_equal(got, want, err_msg=f"pair_bound_list_packed={p}")
        np.testing.assert_array_equal(counts, want.sum(1))
        assert stats == res[0][2] and stats["bound_list_pairs"] > 0      # the exact-unit stage, counter for counter
