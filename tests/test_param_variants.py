"""Tables other than the shipped ones, without a GPU: which kernels the engine opens for each variant of
tests/param_variants.py (msspe_host_table_routes makes the calls chem_entry() makes), what the loader refuses, and
that every variant moves the oracle's numbers, so that the GPU comparisons under it (test_gpu_param_variants.py) are
about something."""
import numpy as np
import pytest

import param_variants as pv
from helpers import stage_b_pool


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def bundles(tmp_path_factory):
    d = tmp_path_factory.mktemp("variants")
    return {name: pv.write_bundle(pv.variant_sections(name), d / (name + ".bundle")) for name in pv.VARIANTS}


@pytest.mark.parametrize("chem", ["ntthal", "primer3"])
@pytest.mark.parametrize("variant", list(pv.VARIANTS))
def test_routes_of_every_variant(m, bundles, variant, chem):
    """fast_ok / int_ok / row_ok / split_max_k / wave_max_k decide which kernel answers a pair; a change to a builder
    of csrc/nn_params.cpp that moves one of them shows up here."""
    routes = m.capi.host_table_routes(bundles[variant], getattr(m.Chem, chem)())
    assert pv.routes_tuple(routes) == pv.EXPECTED_ROUTES[variant]
    assert routes["split_ok"] == (routes["split_max_k"] > 0)


def test_routes_of_the_shipped_bundle_and_of_a_directory(m, tmp_path):
    assert pv.routes_tuple(m.capi.host_table_routes(None)) == (1, 1, 1, 1, 32, 32)
    d = pv.write_directory(pv.variant_sections("wc_missing"), tmp_path / "primer3_config")
    assert pv.routes_tuple(m.capi.host_table_routes(d)) == pv.EXPECTED_ROUTES["wc_missing"]
    with pytest.raises(m.MsspeError) as e:
        m.capi.host_table_routes(tmp_path / "nowhere")
    assert e.value.code == 3


# Which stages the templates of a flanked site pass take, by variant and (k, flank): a template of k + fl + fr bases with
# fl + fr > 0 is a rectangle without a split-table kernel.  stack_x3 at (24, 4) is the one call whose classes part ways.
EXPECTED_FLANK_STAGES = {
    "wc_missing": {(13, 2): {"dense"}, (17, 1): {"dense"}, (24, 4): {"dense"}},
    "dangle_holes": {(13, 2): {"wave"}, (17, 1): {"wave"}, (24, 4): {"wave"}},
    "stack_x1.5": {(13, 2): {"wave"}, (17, 1): {"wave"}, (24, 4): {"wave"}},
    "stack_x3": {(13, 2): {"wave"}, (17, 1): {"wave"}, (24, 4): {"wave", "dense"}},
    "h_mod10": {(13, 2): {"dense"}, (17, 1): {"dense"}, (24, 4): {"dense"}},
}


@pytest.mark.parametrize("variant", pv.COMPUTED)
def test_rectangle_lengths_on_either_side_of_the_bounds(m, bundles, variant):
    """The rectangles and flanked templates of test_gpu_param_variants.py (g to i) and of the stack_x3 reach cases go
    by the longer oligo against split_max_k and wave_max_k.  Pinned here per variant: the stage each of those lengths
    takes, and that the lengths chosen to sit on a bound and one above it still do -- a builder change that moves a
    bound shows here first, not as a GPU case that silently stopped straddling."""
    routes = m.capi.host_table_routes(bundles[variant])
    split, wave = routes["split_max_k"], routes["wave_max_k"]
    any_want, end_want = pv.EXPECTED_RECT_STAGE[variant]
    any_kmax = {max(a, b) for v, a, b in pv.RECT_ANY_CASES if v == variant}
    assert any_kmax == set(any_want)
    assert {kmax: pv.rect_stage(routes, kmax) for kmax in any_kmax} == any_want
    for (v, a, b), (bound, above) in pv.RECT_ANY_ON_BOUND.items():
        if v == variant:
            assert max(a, b) == routes[bound] + above, (v, a, b)
    end_kmax = {max(a, b) for a, b in pv.RECT_END_SHAPES}
    assert {kmax: pv.rect_stage(routes, kmax, end=True) for kmax in end_kmax} == end_want
    # a bound that binds (0 < bound < 32) has a rectangle on it and one a base above it
    for bound in {split, wave} - {0, 32}:
        assert {bound, bound + 1} <= any_kmax, (variant, bound)
    if 0 < wave < 32:
        assert {wave, wave + 1} <= end_kmax
    if variant in pv.FLANK_VARIANTS:
        got = {(k, f): {pv.rect_stage(routes, n, end=True) for n in range(k + 1, k + 2 * f + 1)} for k, f in pv.FLANK_GRID}
        assert got == EXPECTED_FLANK_STAGES[variant]
        if 0 < wave < 32:                        # one call with templates on both sides of wave_max_k
            assert any(k <= wave < k + 2 * f for k, f in pv.FLANK_GRID)
    # without a wave kernel (wave_max_k 0) the route options have nothing to switch, and the GPU cases skip them
    assert (wave == 0) == (variant in ("wc_missing", "h_mod10"))


def _refused(m, sections, tmp_path, as_text=None):
    """The engine's loader on these sections: (status of msspe_host_table_routes, msspe_create's message).  A
    malformed table stops msspe_create before it looks for a device."""
    path = tmp_path / "broken.bundle"
    path.write_text(as_text if as_text is not None else pv.bundle_text(sections))
    with pytest.raises(m.MsspeError) as routes:
        m.capi.host_table_routes(path)
    with pytest.raises(m.MsspeError) as create:
        m.Engine(0, params_path=str(path))
    assert create.value.code == 3
    return routes.value.code, str(create.value)


def test_bonus_tables_at_their_caps_load(m, tmp_path):
    """32 triloop and 128 tetraloop keys are the most the device tables hold; keys of .ds and .dh are merged, so the
    count is that of their union."""
    s = pv.stock_sections()
    tri = ["A" + "".join("ACGT"[(q >> s_) & 3] for s_ in (4, 2, 0)) + "T" for q in range(32)]
    tet = ["C" + "".join("ACGT"[(q >> s_) & 3] for s_ in (6, 4, 2, 0)) + "G" for q in range(128)]
    s["triloop.ds"] = [f"{k}\t0.5" for k in tri[:20]]
    s["triloop.dh"] = [f"{k}\t-100" for k in tri[12:]]
    s["tetraloop.ds"] = [f"{k}\t0.5" for k in tet]
    s["tetraloop.dh"] = [f"{k}\t-100" for k in reversed(tet)]
    path = pv.write_bundle(s, tmp_path / "caps.bundle")
    assert m.capi.host_table_routes(path)["pair_tables"] == 1


@pytest.mark.parametrize("case", ["33_triloops", "33_triloops_in_the_union", "129_tetraloops", "short_key", "long_key",
                                  "odd_token_count", "missing_section"])
def test_bonus_tables_the_loader_refuses(m, tmp_path, case):
    s = pv.stock_sections()
    tri = ["A" + "".join("ACGT"[(q >> s_) & 3] for s_ in (4, 2, 0)) + "T" for q in range(33)]
    tet = ["C" + "".join("ACGT"[(q >> s_) & 3] for s_ in (6, 4, 2, 0)) + "G" for q in range(129)]
    if case == "33_triloops":
        s["triloop.ds"] = [f"{k}\t0" for k in tri]
        s["triloop.dh"] = [f"{k}\t-100" for k in tri]
    elif case == "33_triloops_in_the_union":
        s["triloop.ds"] = [f"{k}\t0" for k in tri[:17]]
        s["triloop.dh"] = [f"{k}\t-100" for k in tri[17:]]
    elif case == "129_tetraloops":
        s["tetraloop.ds"] = [f"{k}\t0" for k in tet]
        s["tetraloop.dh"] = [f"{k}\t-100" for k in tet]
    elif case == "short_key":
        s["tetraloop.dh"] = s["tetraloop.dh"] + ["ACGTT\t-100"]
    elif case == "long_key":
        s["triloop.ds"] = s["triloop.ds"] + ["ACGTTT\t0"]
    elif case == "odd_token_count":
        s["triloop.dh"] = s["triloop.dh"] + ["ACGTT"]
    else:
        del s["tetraloop.ds"]
    code, msg = _refused(m, s, tmp_path)
    assert code == 3
    assert ("missing: tetraloop.ds" if case == "missing_section" else "malformed") in msg


def test_a_count_field_beyond_the_file_is_reported_as_truncated(m, tmp_path):
    text = pv.bundle_text(pv.stock_sections()).replace("@ tetraloop.dh 154", "@ tetraloop.dh 156")
    assert "@ tetraloop.dh 156" in text
    code, msg = _refused(m, None, tmp_path, as_text=text)
    assert code == 3 and "truncated in section tetraloop.dh" in msg


# The share of the ANY dG plane that differs from the stock plane, as the oracle gave it when the variants were drawn
# up (120 random 13-mers / 60 random 20-mers, ntthal's defaults); the tests ask for a tenth of it.
ANY_SHARE = {"wc_missing": (0.16, 0.24), "h_mod10": (0.16, 0.24), "dangle_holes": (0.70, 0.73),
             "stack_x1.5": (0.99, 0.99), "stack_x3": (0.99, 0.99), "loops_and_bonuses": (0.03, 0.12)}


@pytest.fixture(scope="module")
def any_pools(m):
    return {13: m.synth.pool_strings(m.synth.random_pool(120, 13, seed=13)),
            20: m.synth.pool_strings(m.synth.random_pool(60, 20, seed=20))}


@pytest.fixture(scope="module")
def stock_any(oracle, oracle_tables, any_pools):
    return {k: oracle.pool_pairs(oracle_tables, pool)[1] for k, pool in any_pools.items()}


@pytest.mark.parametrize("variant", list(ANY_SHARE))
def test_the_oracle_moves_under_every_variant(oracle, bundles, any_pools, stock_any, variant):
    tables = oracle.Tables(bundles[variant])
    for k, quoted in zip((13, 20), ANY_SHARE[variant]):
        dg = oracle.pool_pairs(tables, any_pools[k])[1]
        share = float((dg != stock_any[k]).mean())
        print(f"{variant} k={k}: {share:.3f} of the ANY dG plane differs from stock")
        assert share >= quoted / 10


def test_the_oracle_loads_the_refused_tables(oracle, bundles, any_pools, stock_any):
    """ntthal computes with a fractional enthalpy; the engine refuses (test_gpu_param_variants.py pins that)."""
    dg = oracle.pool_pairs(oracle.Tables(bundles["h_frac"]), any_pools[13])[1]
    assert (dg != stock_any[13]).any()


@pytest.mark.parametrize("variant", [v for v in pv.VARIANTS if v != "stock"])
def test_hairpins_fold_under_every_variant(oracle, oracle_tables, bundles, variant):
    pool = stage_b_pool(16, 1016)
    assert len(pool) == 98
    got = oracle.check_primers(oracle.Tables(bundles[variant]), pool)["hairpin_th"]
    folded = int((got > 0).sum())
    print(f"{variant}: {folded} of 98 fold")
    assert folded >= 4.8                         # 48 to 83 of 98 when the variants were drawn up
    if variant == "loops_and_bonuses":
        stock = oracle.check_primers(oracle_tables, pool)["hairpin_th"]
        assert int((got != stock).sum()) >= 5.6  # 56 of 98


def test_every_bonus_oligo_feels_its_key(oracle, oracle_tables, bundles):
    """GCGC + key + GCGC under loops_and_bonuses against loops_only, which differs in the four bonus sections alone:
    a kept key has another value, a dropped key has gone, an added key is new (CAAAG in the enthalpy file alone), and
    the triloop entropies, all zero in the shipped file, are part of it.  Every triloop oligo and every dropped or
    added tetraloop oligo has another HAIRPIN_TH than under the control.  Of the 62 kept tetraloops, about half do
    not: the shipped entropy term of most A.T-closed keys is +1610 cal/K/mol (-650 or -970 next to a positive
    enthalpy for a few others), that closure loses to GCGC around a loop of six under either table, and no value of
    the key is read.  The 27 kept keys whose shipped entropy term is zero (all closed by C.G or G.C) are the ones
    that must move.  Against the shipped tables all 96 differ."""
    with_bonus, control = oracle.Tables(bundles["loops_and_bonuses"]), oracle.Tables(bundles["loops_only"])
    shipped_ds = dict(pv._bonus_pairs(pv.stock_sections()["tetraloop.ds"]))
    pool = pv.bonus_pool()
    assert [len(pool[c][13]) for c in ("kept", "dropped", "added")] == [13, 3, 2]
    assert [len(pool[c][14]) for c in ("kept", "dropped", "added")] == [62, 15, 1]
    hairpin = lambda tables, oligos: oracle.check_primers(tables, oligos)["hairpin_th"]
    for k in (13, 14):
        for cls in ("kept", "dropped", "added"):
            oligos = pool[cls][k]
            a, b, stock = hairpin(with_bonus, oligos), hairpin(control, oligos), hairpin(oracle_tables, oligos)
            assert (a > 0).all() and (stock > 0).all()
            assert (a != stock).all()
            if (k, cls) == (14, "kept"):
                reads_the_key = np.array([float(shipped_ds[o[4:10]]) == 0.0 for o in oligos])
                assert reads_the_key.sum() == 27 and (a != b)[reads_the_key].all()
            else:
                assert (a != b).all(), (k, cls)


def test_keys_at_the_caps_move_the_oracle(oracle, bundles):
    """bonus_caps fills the bonus tables to 32 and 128 keys; every oligo built on a key it adds folds otherwise than
    under loops_only, its control, and no two of them alike -- so the device test on them reads every added slot."""
    caps, control = oracle.Tables(bundles["bonus_caps"]), oracle.Tables(bundles["loops_only"])
    for k, n in ((13, 16), (14, 51)):
        oligos = pv.caps_oligos(k)
        a = oracle.check_primers(caps, oligos)["hairpin_th"]
        b = oracle.check_primers(control, oligos)["hairpin_th"]
        assert len(oligos) == n and (a != b).all() and len(set(a.tolist())) == n
