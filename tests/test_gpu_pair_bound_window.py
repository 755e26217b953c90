"""The windowed packed bound first stage on the device (option pair_bound_window; csrc/thal_pairs_row.hip
k_pairs_bound_window, the generated scans row_bound_ring_pinned.inc and row_bound_ring_pair_pinned.inc).

Values: msspe_cross_dimer_bound_window_dev writes the instance's value of every pair -- +inf (no chain), -inf (not
bounded there) or (pick + init) * unit -- and tests/pair_bound_window_model.py computes the same integer from the coarse
tables and the constants of msspe_host_bound_window: == on float64, no tolerance, every pair of every plane, on the
stock tables and on a bundle whose long loops are cheap, so that the far candidate is the minimum of many cells.  The
+-inf pattern is the packed instance's own, and no value is above the packed instance's.

Decisions: a 600-primer random pool and the skewed pool of the bound list stage's tests, pair_bound_window on and off,
mirrored and not, with and without the bound list stage, as a whole square, a square off the origin and a rank's row
block: the oracle's bits under every setting, identical across the settings; the counters say which instance ran."""
import numpy as np
import pytest

import param_variants as pv
import test_gpu_pair_bound_list as bl      # its 323-oligo skewed pool and the oracle's conflicts: computed once for both files
from pair_bound_model import bounded_in_uniform_wave, long_loops_cheap_sections, mixed_pool, two_stem_family
from pair_bound_packed_model import NONE
from pair_bound_window_model import plane_model, window_tables

pytestmark = pytest.mark.gpu

THR = -9000.0
MARKER = 12345.0
KC = 4      # slots per chunk of the generated scan


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
    p = window_tables(m)
    assert p["usable"] == 1 and p["window"]["usable"] == 1
    return p


@pytest.fixture(scope="module")
def cheap(m, tmp_path_factory):
    """(engine, tables) on the bundle whose far entries are negative: the far candidate wins in most cells."""
    path = pv.write_bundle(long_loops_cheap_sections(), tmp_path_factory.mktemp("window") / "long_loops_cheap.bundle")
    p = window_tables(m, path)
    assert p["window"]["usable"] == 1 and min(p["window"]["ifar"], p["window"]["bfar"]) < 0
    e = m.Engine(0, params_path=str(path))
    yield e, p
    e.close()


def device_planes(eng, m, pool, rows, cols):
    """(the windowed instance's plane, the packed instance's) of the block; pre-filled with a marker that must be gone."""
    import torch
    n, k = len(pool), len(pool[0])
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    out = []
    eng.synchronize()
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for call in (eng.cross_dimer_bound_window_dev, eng.cross_dimer_bound_packed_dev):
            d_b = torch.full((rows[1] - rows[0], cols[1] - cols[0]), MARKER, dtype=torch.float64, device="cuda")
            call(d_pool.data_ptr(), n, k, m.Chem.ntthal(), THR, rows, cols, d_b.data_ptr())
            torch.cuda.synchronize()
            out.append(d_b.cpu().numpy())
    finally:
        eng.reset_stream()
    for b in out:
        assert not (b == MARKER).any() and not np.isnan(b).any()
    return out


def model_values(pk, rows, cols):
    """The model's plane in cal/mol (+inf: no chain), computed on the different oligos only."""
    ur, ri = np.unique(np.array(rows), return_inverse=True)
    uc, ci = np.unique(np.array(cols), return_inverse=True)
    pick, vmin, vmax = plane_model(pk, list(ur), list(uc))
    assert vmin == NONE or (pk["lo"] <= vmin and vmax <= pk["hi"])          # every cell value fits the slot word's field
    want = np.where(pick == NONE, np.inf, (pick + pk["init"]) * pk["unit"])
    return want[np.ix_(ri, ci)]


def check_planes(b, packed, want, pk, what):
    """b: the windowed plane.  +-inf exactly where the packed plane has them, every value the model's, none above the
    packed instance's; returns (pairs with a value, pairs the window lowered)."""
    np.testing.assert_array_equal(b == -np.inf, packed == -np.inf, err_msg=f"{what}: -inf")
    np.testing.assert_array_equal(b == np.inf, packed == np.inf, err_msg=f"{what}: +inf")
    fin = np.isfinite(b)
    np.testing.assert_array_equal(b[fin], want[fin], err_msg=f"{what}: a bounded pair's value")
    assert (want[b == np.inf] == np.inf).all() and not np.isfinite(b[want == np.inf]).any(), what
    assert (b[fin] <= packed[fin]).all() and (np.mod(b[fin], pk["unit"]) == 0).all(), what
    return int(fin.sum()), int((b[fin] < packed[fin]).sum())


def test_option_values(eng, m):
    assert eng.info("pair_bound_window") == 2
    for v, want in ((0, 0), (1, 1), ("auto", 2)):
        eng.set_option("pair_bound_window", v)
        assert eng.info("pair_bound_window") == want
    with pytest.raises(m.MsspeError):
        eng.set_option("pair_bound_window", 2)


# ---- values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(2, 14))
def test_square_values_equal_the_model(eng, m, pk, cheap, k):
    """Mixed pools at every length.  Up to F + 1 bases no row lies above a window: the plane is the packed plane."""
    pool = mixed_pool(k, 200 if k == 13 else 72, seed=5700 + k)
    n = len(pool)
    for name, (e, tables) in (("stock", (eng, pk)), ("long_loops_cheap", cheap)):
        b, packed = device_planes(e, m, pool, (0, n), (0, n))
        n_fin, n_low = check_planes(b, packed, model_values(tables, pool, pool), tables, f"{name} k={k}")
        print(f"{name} k={k}: {n_fin} of {n * n} pairs with a value, {n_low} below the packed instance's")
        assert n_fin >= 100
        if k <= tables["window"]["F"] + 1:
            np.testing.assert_array_equal(b, packed)
        if k == 13:
            assert n_low > 0


def test_two_stem_family_as_an_ab_block(m, cheap):
    """The family's long loops on the bundle that makes them cheap: where the relaxation acts."""
    e, tables = cheap
    fam = two_stem_family()
    n = len(fam)
    A, B = [a for a, _ in fam], [b for _, b in fam]
    b, packed = device_planes(e, m, A + B, (0, n), (n, 2 * n))
    n_fin, n_low = check_planes(b, packed, model_values(tables, A, B), tables, "family")
    assert n_fin >= 100 and np.isfinite(np.diag(b)).any() and n_low > 0


def row_starts(row, col):
    """First slot of every stored row of (row, col)'s table in a wave of col's composition (wave_pairs_row: row i takes as
    many slots as col has bases complementary to row[i]); the total behind them."""
    comp = {x: col.count(x) for x in "ACGT"}
    starts, s = [], 0
    for x in row[:-1]:
        starts.append(s)
        s += comp["TGCA"["ACGT".index(x)]]
    return starts, s


def uniform_columns(comp, n_cols, seed):
    rng = np.random.default_rng(seed)
    base = np.array(list("".join(x * c for x, c in zip("ACGT", comp))))
    return ["".join(rng.permutation(base)) for _ in range(n_cols)]


#          name             row oligo        columns' (A, C, G, T)  what it is about
UNIFORM = [("on_boundary", "AAAAAAAAAAAAC", (3, 3, 3, 4)),     # every row 4 slots wide: each window starts on a chunk boundary
           ("inside_chunk", "CACCACCCACCAG", (3, 3, 3, 4)),    # rows 3 or 4 wide: window starts inside chunks
           ("full_table", "AAAAAAAACCTTA", (2, 2, 4, 5)),      # 8 x 5 + 2 x 4 + 2 x 2 = 52 slots: the last chunk is an entry chunk
           ("homopolymer", "ACGTTGCAAGTCA", (0, 0, 0, 13)),    # columns T...T: only the A rows hold cells, windows have empty rows
           ("homopolymer_g", "ACTAGCATTACGA", (0, 0, 13, 0))]


@pytest.mark.parametrize("name,row,comp", UNIFORM, ids=[u[0] for u in UNIFORM])
@pytest.mark.parametrize("n_cols", [65, 1100])
def test_single_composition_column_blocks(m, pk, cheap, eng, name, row, comp, n_cols):
    """One row against columns of one base composition (one composition per wave: the slot-to-row boundaries the scan's
    entry is computed from), 65 columns -- a full and a partial wave -- and 1,100, a group for each of the block's waves."""
    F = pk["window"]["F"]
    cols = uniform_columns(comp, 1 if comp.count(0) == 3 else n_cols, seed=5800 + n_cols)
    cols = cols * (n_cols if len(cols) == 1 else 1)
    starts, total = row_starts(row, cols[0])
    entry = [starts[i - F] for i in range(F, 13)]      # the first slot of row i - F, for every row i with rows above its window
    if name == "on_boundary":
        assert all(s % KC == 0 for s in entry)
    if name == "inside_chunk":
        assert sum(s % KC != 0 for s in entry) >= 6
    if name == "full_table":
        assert total == 52 and (F != 2 or any(s // KC == 12 for s in entry))
    if name.startswith("homopolymer"):
        assert any(starts[i] == starts[i + 1] for i in range(11)) and 0 < total <= 52
    ok = np.array([[bounded_in_uniform_wave(row, y) for y in cols]])
    assert ok.any()
    for what, (e, tables) in (("stock", (eng, pk)), ("long_loops_cheap", cheap)):
        b, packed = device_planes(e, m, [row] + cols, (0, 1), (1, 1 + n_cols))
        np.testing.assert_array_equal(b != -np.inf, ok, err_msg=f"{name}: the pairs handed on unbounded are not the sizing rule's")
        n_fin, _ = check_planes(b, packed, model_values(tables, [row], cols), tables, f"{what} {name} x {n_cols}")
        assert n_fin > 0


# ---- decisions ---------------------------------------------------------------------------------------------------------
def screen(eng, m, pool, rows, cols, window, mirror, bound_list):
    """(bitmap as bool, the block's row counts, statistics) of one device screen of the block."""
    import torch
    n, k = len(pool), len(pool[0])
    nr, nc = rows[1] - rows[0], cols[1] - cols[0]
    words = (nc + 63) // 64
    opts = {"pair_bound": 1, "pair_mirror": mirror, "pair_bound_list": bound_list, "pair_bound_window": window}
    for key, v in opts.items():
        eng.set_option(key, v)
    eng.pair_stage_stats()
    eng.hand_over_lists()
    try:
        d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
        d_rc = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_bm = torch.zeros(nr * words, dtype=torch.int64, device="cuda")
        eng.synchronize()
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            eng.cross_dimer_dev(d_pool.data_ptr(), n, k, m.Chem.ntthal(), THR, rows, cols, d_rc.data_ptr(), d_bm.data_ptr())
            torch.cuda.synchronize()
        finally:
            eng.reset_stream()
        got = bl.bits(d_bm.cpu().numpy().reshape(nr, words).view(np.uint64), nc)
        counts = d_rc.cpu().numpy()[rows[0]:rows[1]]
        stats = bl.read_stats(eng)      # raises if a hand-over list, list U included, was overrun
    finally:
        for key in opts:
            eng.set_option(key, "auto")
    return got, np.asarray(counts), stats


_random = {}


def random_pool(oracle, oracle_tables):
    """600 seeded random 13-mers and one more -- an odd size: partial waves, a partial last launch -- with the oracle's
    conflicts: once for every test."""
    if not _random:
        pool = mixed_pool(13, 600, seed=5900)[:601]
        _random["pool"] = pool
        _random["want"] = bl.oracle_of(oracle, oracle_tables, pool, "window_random_601")
    return _random["pool"], _random["want"]


def blocks(n):
    """whole square | a square off the origin (mirrored where the mirror is on) | a rank's row block (never mirrored)"""
    return {"square": ((0, n), (0, n)), "off_origin": ((67, n - 3), (67, n - 3)), "row_block": ((40, 201), (0, n))}


@pytest.mark.parametrize("mirror", ["auto", 0])
@pytest.mark.parametrize("form", ["square", "off_origin", "row_block"])
@pytest.mark.parametrize("which", ["random", "skewed"])
def test_decisions_are_the_oracles_under_every_setting(eng, m, oracle, oracle_tables, which, form, mirror):
    if which == "random":
        pool, want_all = random_pool(oracle, oracle_tables)
    else:
        pool, _ = bl.pool_of(13, bl.N_DECISIONS)
        want_all = bl.oracle_of(oracle, oracle_tables, pool, "square")
    n = len(pool)
    assert n % 2 == 1
    rows, cols = blocks(n)[form]
    want = want_all[rows[0]:rows[1], cols[0]:cols[1]]
    #          pair_bound_window, pair_bound_list
    settings = [(0, "auto"), (1, "auto"), (1, 0), (0, 0)]
    res = {s: screen(eng, m, pool, rows, cols, s[0], mirror, s[1]) for s in settings}
    for s, (got, counts, stats) in res.items():
        np.testing.assert_array_equal(got, want, err_msg=f"{which} {form} window={s[0]} list={s[1]} pair_mirror={mirror}")
        np.testing.assert_array_equal(counts, want.sum(1), err_msg=f"{which} {form} window={s[0]} list={s[1]} pair_mirror={mirror}")
        np.testing.assert_array_equal(got, res[(0, "auto")][0])
        np.testing.assert_array_equal(counts, res[(0, "auto")][1])
    off, on, no_list, neither = (res[s][2] for s in settings)
    print(f"{which} {form} pair_mirror={mirror}: packed survivors {off['bound_survivors']}, windowed {on['bound_window_survivors']}; "
          f"U {off['bound_list_pairs']} -> {on['bound_list_pairs']}; lists[0] {off['lists'][0]} -> {on['lists'][0]}")
    mirrored = mirror == "auto" and form != "row_block"
    nr = rows[1] - rows[0]
    for stats in (off, on, no_list, neither):
        assert stats["bound_mirrored"] == (nr * (nr - 1) // 2 if mirrored else 0)
    # off: the packed instance; on: the windowed one -- its survivors are list U's, it appends none to list 0 itself
    assert off["bound_window_survivors"] == 0 and off["bound_survivors"] > 0
    assert on["bound_survivors"] == 0 and on["bound_window_survivors"] >= off["bound_survivors"]
    # U holds unordered pairs under the mirror, the counters ordered ones
    assert on["bound_list_pairs"] >= off["bound_list_pairs"] + on["bound_window_survivors"] // (2 if mirrored else 1)
    # the exact-unit bound of the list stage culls at least what the packed bound culls: list 0 is no longer
    assert on["lists"][0] <= off["lists"][0]
    # without the bound list stage the route falls back to the packed instance: the very same counters
    assert no_list == neither and no_list["bound_window_survivors"] == 0 and no_list["bound_list_pairs"] == 0
    assert no_list["bound_survivors"] == off["bound_survivors"]


def test_auto_keeps_small_screens_on_the_packed_instance(eng, m, oracle, oracle_tables):
    """auto: screens below 2^23 pairs stay on the packed instance (the first stage is not what their time is)."""
    pool, want = random_pool(oracle, oracle_tables)
    n = len(pool)
    got, _, stats = screen(eng, m, pool, (0, n), (0, n), "auto", "auto", "auto")
    np.testing.assert_array_equal(got, want)
    assert stats["bound_window_survivors"] == 0 and stats["bound_survivors"] > 0
