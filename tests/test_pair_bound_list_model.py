"""The bound list stage's lower-bound argument without a GPU: for the pairs that stage exists for -- 53..63 stored
cells, which the bound first stage hands on without a bound of their own -- pair_bound_model.bound_pair, the integer
k_pairs_bound_list must report (tests/test_gpu_pair_bound_list.py), never exceeds the oracle's dG.  Large tables are
where a chain has the most terms to round down and the most loop shapes to choose from.

13 bases and the two shorter lengths whose tables reach 53 cells (9 and 11), under the stock tables, a 37 C high-salt
chemistry (a negative per-pair salt step) and the long_loops_cheap bundle (long loops win the minimum).  Also here: the
rule of pair_bound_list_model.py that says which pairs that stage bounds, and that the pools hold every class."""
import numpy as np
import pytest

import param_variants as pv
from pair_bound_model import SLOTS, bound_pair, long_loops_cheap_sections, rc, stored_cells
from pair_bound_list_model import LIST_SLOTS, class_plane, n_cells, pair_class, skewed_pool

THR = -9000.0
N_RANDOM = 100
MAX_PAIRS = 250       # pairs of class 'u' the Python model is run on, per case
CHEMS = {"stock": {}, "t37_high_salt": {"temp_c": 37.0, "mv": 600.0, "dv": 20.0}}


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


def test_pair_classes():
    assert pair_class("A" * 13, "T" * 13) == "over" and stored_cells("A" * 13, "T" * 13) == 156
    assert pair_class("A" * 13, "A" * 13) == "none"
    assert pair_class("ATATATATATAT", "GCGCGCGCGCGC") == "sym" and pair_class("ATATATATATAT", "ATATATATATAT") == "sym"
    # 7 A x 8 T + 6 T x 5 A = 86 cells, the last row (T) finds 5 A: 81 stored; 8 A x 8 T = 64, last row A: 56 stored
    a, b = "AAAAAAATTTTTT", "TTTTTTTTAAAAA"
    assert n_cells(a, b) == 86 and stored_cells(a, b) == 81 and pair_class(a, b) == "over" and rc(a) == "AAAAAATTTTTTT"
    assert stored_cells("CAAAAAAACCCCA", "TTTTTTTTCCCCC") == 64 - 8 and pair_class("CAAAAAAACCCCA", "TTTTTTTTCCCCC") == "u"
    assert pair_class("CAAAAAAACCCCA", "TTTTTTTCCCCCC") == "row"   # 56 cells, 49 stored
    assert SLOTS == 52 and LIST_SLOTS == 63


def test_the_two_stem_family_never_reaches_the_list_stage():
    """The constructed two-stem pairs (pair_bound_model.two_stem_family) are stems in a filler of A, which pairs with
    nothing: no a against any b has more than 52 stored cells, so none is bounded by the list stage for its size."""
    from pair_bound_model import two_stem_family
    fam = two_stem_family()
    A, B = sorted({a for a, _ in fam}), sorted({b for _, b in fam})
    assert max(stored_cells(a, b) for a in A for b in B) <= SLOTS


def test_the_skewed_pool_is_what_the_issue_measured():
    """600 seeded 13-mers with P(A) = P(T) = 0.35: about a sixth of the ordered pairs at 53..63 stored cells, a few per
    cent beyond, four fifths at 52 or fewer (16.4 % / 2.6 % / 81 % for the seed the stage was sized with)."""
    pool = skewed_pool(13, 600, seed=8113, n_rich=0)[:600]
    c = class_plane(pool, pool)
    share = {x: float((c == x).mean()) for x in ("u", "over", "row")}
    print(share)
    assert 0.12 < share["u"] < 0.21 and 0.01 < share["over"] < 0.05 and 0.74 < share["row"] < 0.87


@pytest.mark.parametrize("k", [13, 11, 9])
@pytest.mark.parametrize("case", ["stock", "t37_high_salt", "long_loops_cheap"])
def test_model_bound_is_below_the_oracle_for_list_sized_pairs(m, oracle, oracle_tables, tmp_path, k, case):
    pool = skewed_pool(k, N_RANDOM, seed=8100 + k)
    cls = class_plane(pool, pool)
    idx = np.argwhere(cls == "u")
    assert len(idx) >= 20, f"k={k}: {len(idx)} pairs with 53..63 stored cells"
    if len(idx) > MAX_PAIRS:
        idx = idx[np.random.default_rng(k).choice(len(idx), MAX_PAIRS, replace=False)]
    path, tables, kw = None, oracle_tables, CHEMS.get(case, {})
    if case == "long_loops_cheap":
        path = pv.write_bundle(long_loops_cheap_sections(), tmp_path / "long_loops_cheap.bundle")
        tables = oracle.Tables(path)
    bt = m.capi.host_bound_tables(path, m.Chem.ntthal(**kw), THR)
    assert bt["usable"] == 1
    _, dg, _, _ = oracle.pool_pairs(tables, pool, oracle.ntthal_args(**kw), THR)
    gaps = []
    for i, j in idx:
        lb = bound_pair(bt, pool[i], pool[j])
        assert lb is not None and np.isfinite(dg[i, j]), (pool[i], pool[j])
        assert lb <= dg[i, j], (pool[i], pool[j], lb, dg[i, j])
        gaps.append(dg[i, j] - lb)
    gaps = np.array(gaps)
    culled = float(np.mean([dg[i, j] - g > bt["cut"] / bt["unit_inv"] for (i, j), g in zip(idx, gaps)]))
    print(f"k={k} {case}: {len(idx)} pairs with 53..63 stored cells, smallest gap {gaps.min():.4f} cal/mol, mean {gaps.mean():.1f}; "
          f"{culled:.3f} of them have a bound above the cut plus margin")
    assert gaps.min() >= 0.0
