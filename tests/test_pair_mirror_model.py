"""The mirrored bound first stage without a GPU (option pair_mirror; csrc/nn_params.cpp bound_mirror_ok through
msspe_host_bound_mirror_ok, tests/pair_bound_model.py for the recurrence).

A square same-pool screen fills each unordered pair once and uses the bound of (a, b) for (b, a) as well.  That is sound
where every real-valued term of the bound tables equals its strand-swapped partner: the flag must be set for the stock
tables and a loop variant of them, and clear for a bundle with one stacked pair changed and its partner left alone.
The model then checks what the flag promises on a seeded pool: the bound of (a, b) never exceeds the oracle's dG of
(b, a) by more than the margin, the two orders' bounds differ by rounding only, and "no chain" is common to both."""
import numpy as np
import pytest

import param_variants as pv
from pair_bound_model import bound_pair
from pair_mirror_model import broken_sections

THR = -9000.0
E = 1.0                      # cal/mol: fast_tables.hpp BoundTables::kMargin
# two valid lower bounds of one real-number minimum, each a sum of at most 27 terms rounded down to 1/64 cal/mol
MAX_ASYM = 27 / 64
CHEMS = {"ntthal25": {}, "hot_salty": {"temp_c": 37.0, "mv": 600.0, "dv": 20.0}}


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.mark.parametrize("variant", ["stock", "loops_and_bonuses"])
def test_mirror_flag_on_sound_tables(m, tmp_path, variant):
    path = None if variant == "stock" else pv.write_bundle(pv.variant_sections(variant), tmp_path / "v.bundle")
    chems = [m.Chem.ntthal()] if variant != "stock" else [
        m.Chem.ntthal(), m.Chem.ntthal(temp_c=37.0, mv=600.0, dv=20.0), m.Chem.primer3()]
    for chem in chems:
        assert m.capi.host_bound_tables(path, chem, THR)["usable"] == 1
        assert m.capi.host_bound_mirror_ok(path, chem, THR) is True


def test_mirror_flag_on_a_broken_bundle(m, tmp_path):
    path = pv.write_bundle(broken_sections(), tmp_path / "broken.bundle")
    # the bound stage itself still applies: such a bundle runs it un-mirrored
    assert m.capi.host_bound_tables(path, m.Chem.ntthal(), THR)["usable"] == 1
    assert m.capi.host_bound_mirror_ok(path, m.Chem.ntthal(), THR) is False


def test_no_flag_without_usable_tables(m):
    assert m.capi.host_bound_mirror_ok(None, m.Chem.ntthal(), 500.0) is False   # a cut above 0: no bound stage at all


@pytest.mark.parametrize("chem_name", list(CHEMS))
def test_model_mirror_against_the_oracle(m, oracle, oracle_tables, chem_name):
    kw = CHEMS[chem_name]
    pool = m.synth.pool_strings(m.synth.random_pool(150, 13, seed=11))
    pool += ["GCCAGTTCGGATA", oracle.reverse_complement("GCCAGTTCGGATA"), "GGGGGGGCCCCCC", "GCGCGCGCGCGCG"]
    n = len(pool)
    bt = m.capi.host_bound_tables(None, m.Chem.ntthal(**kw), THR)
    _, dg, _, _ = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(**kw), THR)
    lb = np.full((n, n), np.nan)      # nan: no chain
    for i, a in enumerate(pool):
        for j, b in enumerate(pool):
            v = bound_pair(bt, a, b)
            if v is not None:
                lb[i, j] = v
    none = np.isnan(lb)
    # "no chain" holds in both orders or in neither
    np.testing.assert_array_equal(none, none.T)
    # the bound of (a, b) against the oracle's dG of (b, a)
    has = np.isfinite(dg.T) & ~none
    gap = dg.T[has] - lb[has]
    asym = np.abs(lb - lb.T)[~none]
    print(f"{chem_name}: LB(a,b) below dG(b,a) by {gap.min():.4f} at least; |LB(a,b) - LB(b,a)| <= {asym.max() * 64:.0f}/64 "
          f"in {np.mean(asym > 0) * 100:.1f} % of the pairs")
    assert has.sum() > n * n // 2
    assert (lb[has] <= dg.T[has] + E).all(), f"worst {-gap.min()}"
    assert (asym <= MAX_ASYM).all()
