"""The packed bound first stage on the device (option pair_bound_packed; csrc/thal_pairs_row.hip k_pairs_bound_packed,
the generated scan row_bound_packed_pinned.inc).

Values: msspe_cross_dimer_bound_packed_dev writes the instance's value of every pair -- +inf (no chain), -inf (not
bounded there) or (pick + init) * unit -- and tests/pair_bound_packed_model.py computes the same integer from the
coarse tables of msspe_host_bound_packed: == on float64, no tolerance, every pair of every plane.  The +-inf pattern
is the exact-unit instance's own, pair for pair (the sizing rules are shared), and on column blocks of one base
composition it is what pair_bound_model.bounded_in_uniform_wave says.

Decisions: the skewed pool of the bound list stage's tests, pair_bound_packed 0 / 1 / auto, mirrored and not, as a
square screen, a row block and an A/B screen: the oracle's bits under every setting, identical across the settings,
list U untouched, and at least as many survivors as the exact-unit instance leaves.  A bundle whose range fits no
coarse unit runs the exact-unit instance."""
import numpy as np
import pytest

import param_variants as pv
import test_gpu_pair_bound_list as bl      # its 323-oligo skewed pool and the oracle's conflicts: computed once for both files
from pair_bound_model import bounded_in_uniform_wave, mixed_pool, two_stem_family
from pair_bound_packed_model import NONE, packed_tables, plane_model, unpackable_sections

pytestmark = pytest.mark.gpu

THR = -9000.0
MARKER = 12345.0


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


def device_planes(eng, m, pool, rows, cols, chem=None, thr=THR):
    """(the packed instance's plane, the exact-unit instance's) of the block; pre-filled with a marker that must be gone."""
    import torch
    n, k = len(pool), len(pool[0])
    chem = chem or m.Chem.ntthal()
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    out = []
    eng.synchronize()
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for call in (eng.cross_dimer_bound_packed_dev, eng.cross_dimer_bound_dev):
            d_b = torch.full((rows[1] - rows[0], cols[1] - cols[0]), MARKER, dtype=torch.float64, device="cuda")
            call(d_pool.data_ptr(), n, k, chem, thr, rows, cols, d_b.data_ptr())
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


def check_planes(b, exact, want, pk, what):
    """b: the packed plane.  Finite exactly where the exact-unit plane is, -inf and +inf likewise; every value the
    model's; never above the exact-unit value, and below it by less than the 27 floored terms of the longest chain."""
    np.testing.assert_array_equal(b == -np.inf, exact == -np.inf, err_msg=f"{what}: -inf")
    np.testing.assert_array_equal(b == np.inf, exact == np.inf, err_msg=f"{what}: +inf")
    fin = np.isfinite(b)
    np.testing.assert_array_equal(b[fin], want[fin], err_msg=f"{what}: a bounded pair's value")
    assert (want[b == np.inf] == np.inf).all() and not np.isfinite(b[want == np.inf]).any(), what
    assert (b[fin] <= exact[fin]).all() and (exact[fin] - b[fin] < 27 * pk["unit"]).all(), what
    assert (np.mod(b[fin], pk["unit"]) == 0).all(), what
    return fin


def test_option_values(eng, m):
    assert eng.info("pair_bound_packed") == 2
    for v, want in ((0, 0), (1, 1), ("auto", 2)):
        eng.set_option("pair_bound_packed", v)
        assert eng.info("pair_bound_packed") == want
    with pytest.raises(m.MsspeError):
        eng.set_option("pair_bound_packed", 2)


# ---- values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n_random", [(13, 250), (12, 96), (9, 96)])
def test_square_values_equal_the_model(eng, m, pk, k, n_random):
    pool = mixed_pool(k, n_random, seed=5400 + k)
    n = len(pool)
    b, exact = device_planes(eng, m, pool, (0, n), (0, n))
    fin = check_planes(b, exact, model_values(pk, pool, pool), pk, f"k={k}")
    print(f"k={k}: {int(fin.sum())} of {n * n} pairs with a value, {int((b == -np.inf).sum())} not bounded, "
          f"exact - packed at most {np.max(exact[fin] - b[fin]):.3f} cal/mol")
    # (waves of a pool this small mix compositions and shed lanes: no bounded share is asserted, only that values were compared;
    #  the single-row blocks below assert the pattern against the sizing rule)
    assert fin.sum() >= 100


def test_two_stem_family_as_an_ab_block(eng, m, pk):
    fam = two_stem_family()
    n = len(fam)
    A, B = [a for a, _ in fam], [b for _, b in fam]
    b, exact = device_planes(eng, m, A + B, (0, n), (n, 2 * n))
    fin = check_planes(b, exact, model_values(pk, A, B), pk, "family")
    assert fin.sum() >= 100 and np.isfinite(np.diag(b)).any()      # (the family pairs themselves: many loop shapes on their chains)
    print(f"family: {int(fin.sum())} of {b.size} pairs with a value, {int(np.isfinite(np.diag(b)).sum())} of {n} family pairs")


COMP = (3, 3, 3, 4)


def uniform_columns(n_cols, seed):
    rng = np.random.default_rng(seed)
    base = np.array(list("".join(x * c for x, c in zip("ACGT", COMP))))
    return ["".join(rng.permutation(base)) for _ in range(n_cols)]


@pytest.mark.parametrize("n_cols", [1, 63, 64, 65, 1100])
def test_single_row_blocks_round_the_wave_edge(eng, m, pk, n_cols):
    """One row against 1, 63, 64, 65 columns of one base composition, and against 1,100: 18 column groups, so that each
    of the block's 16 waves draws one.  +-inf exactly where the sizing rule of a uniform wave says."""
    rows = mixed_pool(13, 6, seed=5500)
    cols = uniform_columns(n_cols, seed=5600 + n_cols)
    R = len(rows)
    want = model_values(pk, rows, cols)
    for r in range(R):
        b, exact = device_planes(eng, m, rows + cols, (r, r + 1), (R, R + n_cols))
        ok = np.array([[bounded_in_uniform_wave(rows[r], y) for y in cols]])
        np.testing.assert_array_equal(b != -np.inf, ok, err_msg=f"row {rows[r]}: the pairs handed on unbounded are not the sizing rule's")
        check_planes(b, exact, want[r:r + 1], pk, f"row {rows[r]} x {n_cols}")


# ---- decisions ---------------------------------------------------------------------------------------------------------
def set_options(eng, packed, mirror):
    eng.set_option("pair_bound", 1)
    eng.set_option("pair_mirror", mirror)
    eng.set_option("pair_bound_packed", packed)


def reset_options(eng):
    for key in ("pair_bound", "pair_mirror", "pair_bound_packed"):
        eng.set_option(key, "auto")


def run_form(eng, m, pool, form, packed, mirror):
    """(bitmap as bool, the block's row counts, statistics) of one screen."""
    import torch
    n, k = len(pool), len(pool[0])
    set_options(eng, packed, mirror)
    eng.pair_stage_stats()
    eng.hand_over_lists()
    try:
        if form == "square":
            out = eng.cross_dimer(pool, m.Chem.ntthal(), THR, want_dg=False)
            got, counts = bl.bits(out["bitmap"], n), out["row_conflicts"]
        elif form == "ab":
            out = eng.cross_dimer_ab(pool[:150], pool[150:], m.Chem.ntthal(), THR, want_dg=False)
            got, counts = bl.bits(out["bitmap"], n - 150), out["row_conflicts"]
        else:
            rows, cols = ROW_BLOCK[0], (ROW_BLOCK[1][0], n)
            nr, nc = rows[1] - rows[0], cols[1] - cols[0]
            words = (nc + 63) // 64
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
        stats = bl.read_stats(eng)
    finally:
        reset_options(eng)
    return got, np.asarray(counts), stats


ROW_BLOCK = ((40, 200), (10, None))


def want_of(form, want, n):
    if form == "square":
        return want
    if form == "ab":
        return want[:150, 150:]
    return want[ROW_BLOCK[0][0]:ROW_BLOCK[0][1], ROW_BLOCK[1][0]:n]


@pytest.mark.parametrize("mirror", ["auto", 0])
@pytest.mark.parametrize("form", ["square", "row_block", "ab"])
def test_decisions_are_the_oracles_under_every_setting(eng, m, oracle, oracle_tables, form, mirror):
    pool, _ = bl.pool_of(13, bl.N_DECISIONS)
    n = len(pool)
    assert n == 323
    want = want_of(form, bl.oracle_of(oracle, oracle_tables, pool, "square"), n)
    res = {packed: run_form(eng, m, pool, form, packed, mirror) for packed in (0, 1, "auto")}
    for packed, (got, counts, stats) in res.items():
        np.testing.assert_array_equal(got, want, err_msg=f"{form} pair_bound_packed={packed} pair_mirror={mirror}")
        np.testing.assert_array_equal(counts, want.sum(1), err_msg=f"{form} pair_bound_packed={packed} pair_mirror={mirror}")
        np.testing.assert_array_equal(got, res[0][0])
        np.testing.assert_array_equal(counts, res[0][1])
        assert stats["bound_list_pairs"] == res[0][2]["bound_list_pairs"] > 0      # the sizing did not move
        assert stats["bound_mirrored"] == (n * (n - 1) // 2 if form == "square" and mirror == "auto" else 0)
    exact, on, auto = res[0][2], res[1][2], res["auto"][2]
    print(f"{form} pair_mirror={mirror}: survivors {exact['bound_survivors']} exact / {on['bound_survivors']} packed, "
          f"U {on['bound_list_pairs']}, lists[0] {exact['lists'][0]} / {on['lists'][0]}")
    assert on["bound_survivors"] >= exact["bound_survivors"]      # (this pool's A/B block leaves no survivor under either)
    assert auto["bound_survivors"] == on["bound_survivors"] and auto["lists"] == on["lists"]      # auto is the packed instance


def test_a_bundle_whose_range_fits_no_unit_runs_the_exact_instance(m, oracle, tmp_path):
    path = pv.write_bundle(unpackable_sections(), tmp_path / "unpackable.bundle")
    assert m.capi.host_bound_packed(path)["usable"] == 0 and m.capi.host_bound_tables(path)["usable"] == 1
    pool, _ = bl.pool_of(13, bl.N_DECISIONS)
    n = len(pool)
    want = bl.oracle_of(oracle, oracle.Tables(path), pool, "unpackable")
    e = m.Engine(0, params_path=str(path))
    try:
        res = {packed: run_form(e, m, pool, "square", packed, "auto") for packed in (0, 1, "auto")}
        for packed, (got, counts, stats) in res.items():
            np.testing.assert_array_equal(got, want, err_msg=f"pair_bound_packed={packed}")
            np.testing.assert_array_equal(counts, want.sum(1))
            # the very same kernel ran: the counters are identical
            assert stats == res[0][2] and stats["bound_mirrored"] == n * (n - 1) // 2
        # ... and the packed plane form refuses, leaving the plane alone
        import torch
        d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
        d_b = torch.full((n, n), MARKER, dtype=torch.float64, device="cuda")
        e.synchronize()
        e.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            with pytest.raises(m.MsspeError):
                e.cross_dimer_bound_packed_dev(d_pool.data_ptr(), n, 13, m.Chem.ntthal(), THR, (0, n), (0, n), d_b.data_ptr())
            torch.cuda.synchronize()
        finally:
            e.reset_stream()
        assert (d_b.cpu().numpy() == MARKER).all()
    finally:
        e.close()
