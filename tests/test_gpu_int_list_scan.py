"""The integer list stage's predecessor scan (thal_pairs_int.hip, k_pairs_int_list) on pools that live in it.

A pair's table has one cell per complementary (base of oligo 1, base of oligo 2) combination: sum over b of
n1(b) * n2(3 - b), from the two compositions alone.  The first stage stores 52 cells of a 13-mer pair and hands
larger tables on; the list stage stores 63 (the cells of the last row take no slot in either).  Random 13-mers put
2 % of their pairs there.  The oligos here are A/T-rich with one or two C / G, so that three quarters of the pairs
have 53 ... 63 stored cells: tables the first stage cannot hold and the list stage can, scanned with far chunks
(rows i-3 and above), near chunks, bulges on either strand and 1 x 1 loops in every one of them.

Bar: every decision, and the dG / Tm planes in a second call, bit for bit with the oracle; both first stages
(pair_kernel auto and int) and both chemistries.  The engine's counters must show that the pairs really went
through the list stage: at least half handed on by the first stage, fewer than 5 % left to the f64 kernels.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 13
N = 523                      # not a multiple of 64
FIRST_STAGE_CELLS = 52       # int_core.hpp kSlotsSmall; thal_pairs_row.hip kRowSlots
LIST_STAGE_CELLS = 63        # kSlotsList - 1 (one slot stays free for the last row's writes)
# (A, C, G, T) counts of a 13-mer; the order of the bases is random
COMPOSITIONS = [(5, 1, 1, 6), (6, 1, 1, 5), (5, 1, 1, 6), (6, 1, 1, 5), (5, 2, 1, 5), (5, 1, 2, 5), (6, 1, 0, 6)]


def list_stage_pool(n: int = N, seed: int = 7) -> list[str]:
    rng = np.random.default_rng(seed)
    pool = []
    for _ in range(n):
        a, c, g, t = COMPOSITIONS[int(rng.integers(len(COMPOSITIONS)))]
        pool.append("".join(rng.permutation(list("A" * a + "C" * c + "G" * g + "T" * t))))
    assert all(len(s) == K for s in pool)
    return pool


def share_in_list_stage_range(pool: list[str]) -> float:
    """Share of the ordered pairs whose stored cells (cells minus the cells of the last row) lie in 53 ... 63.  The
    last row is the row of oligo 1's last base in the kernel's order; a pair counts only if it is in range whichever
    end of oligo 1 that is."""
    codes = np.array([["ACGT".index(ch) for ch in s] for s in pool])
    counts = np.stack([(codes == b).sum(1) for b in range(4)], 1)          # (n, 4)
    partners = counts[:, ::-1]                                             # [j, b] = n_j(3 - b)
    cells = counts @ partners.T                                            # [i, j] = sum_b n_i(b) n_j(3 - b)
    in_range = np.ones_like(cells, dtype=bool)
    for end in (0, -1):
        last_row = partners[:, codes[:, end]].T                            # [i, j] = n_j(3 - end base of i)
        stored = cells - last_row
        in_range &= (stored > FIRST_STAGE_CELLS) & (stored <= LIST_STAGE_CELLS)
    return float(in_range.mean())


def bits(bm, n):
    return np.unpackbits(bm.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


@pytest.fixture(scope="module")
def eng():
    import msspe_amd
    e = msspe_amd.Engine(0)
    yield e
    e.close()


def test_the_pool_lives_in_the_list_stage():
    assert share_in_list_stage_range(list_stage_pool()) >= 0.6


@pytest.mark.parametrize("pair_kernel", ["auto", "int"])
@pytest.mark.parametrize("chem", ["od-msspe", "primer3"])
def test_list_stage_scan_equals_the_oracle(eng, oracle, oracle_tables, chem, pair_kernel):
    import msspe_amd as m
    pool = list_stage_pool()
    share = share_in_list_stage_range(pool)
    print(f"share of pairs with 53 ... 63 stored cells: {share:.4f}")
    assert share >= 0.6                          # before anything runs on the GPU
    n = len(pool)
    g_chem, o_args = {"od-msspe": (m.Chem.ntthal(), oracle.ntthal_args()),
                      "primer3": (m.Chem.primer3(), oracle.p3_args())}[chem]
    # the cut runs through the bulk of the values: the whole-number median of the oracle's finite dG
    _, dg0, _, _ = oracle.pool_pairs(oracle_tables, pool, o_args, 0.0)
    thr = float(np.round(np.median(dg0[np.isfinite(dg0)])))
    cnt, dg, cf, tt = oracle.pool_pairs(oracle_tables, pool, o_args, thr, want_t=True)
    assert 0.2 < cnt / (n * n) < 0.8
    eng.set_option("pair_kernel", pair_kernel)
    try:
        eng.pair_stage_stats()                   # (both reads reset their counters)
        eng.last_overflow_pairs()
        fast = eng.cross_dimer(pool, g_chem, thr, want_dg=False, want_tm=False)
        handed_on = eng.last_overflow_pairs()
        stats = eng.pair_stage_stats()
        out = eng.cross_dimer(pool, g_chem, thr, want_dg=True, want_tm=True)
    finally:
        eng.set_option("pair_kernel", "auto")
    print(f"{chem} pair_kernel={pair_kernel}: thr {thr}, conflicts {cnt}, handed on {handed_on} of {n * n}, "
          f"needed f64 {stats['needed_f64']}, list stage {stats['list']}")
    np.testing.assert_array_equal(bits(fast["bitmap"], n), cf.astype(bool))
    np.testing.assert_array_equal(fast["row_conflicts"], cf.sum(1).astype(np.uint32))
    np.testing.assert_array_equal(out["dg"], dg)
    np.testing.assert_array_equal(out["tm"], tt)
    np.testing.assert_array_equal(bits(out["bitmap"], n), cf.astype(bool))
    np.testing.assert_array_equal(out["row_conflicts"], cf.sum(1).astype(np.uint32))
    assert handed_on >= n * n // 2               # the first stage handed at least half of the pairs on ...
    assert stats["needed_f64"] < 0.05 * n * n    # ... and the list stage answered them: few went to the f64 kernels
    assert stats["list"]["replay_mismatch"] == 0
