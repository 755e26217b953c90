"""The windowed packed bound first stage without a GPU (option pair_bound_window; csrc/nn_params.cpp build_bound_window
through msspe_host_bound_window; tests/pair_bound_window_model.py).

Constants: ifar / bfar are the minima over the exported coarse table's rows l1 >= F.  Argument: the windowed model <=
the packed model <= the exact-unit model <= the oracle's dG (+ the margin), pair for pair -- on mixed pools, on the
two-stem family, whose long loops are where the relaxation acts, on a bundle whose far entries are negative and in
every corner of the chemistry domain; and every cell value the windowed model produces lies inside the packed
instance's exported range [lo, hi].  Where the packed instance is unusable, so is this one."""
import subprocess
import sys
from pathlib import Path

import pytest

import param_variants as pv
from pair_bound_model import EDGE_CHEMS, bound_pair, long_loops_cheap_sections, mixed_pool, two_stem_family
from pair_bound_packed_model import NONE, packed_bound_pair, unpackable_sections
from pair_bound_window_model import cells_and_pick, far_constants, plane_model, window_bound_pair, window_tables
from test_pair_bound_packed_model import EXTREMES

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "open-msspe-design_amd" / "csrc"
THR = -9000.0


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.mark.parametrize("tool, args, inc", [
    ("gen_row_bound_packed_asm.py", ["--ring"], "row_bound_ring_pinned.inc"),
    ("gen_row_bound_packed_asm.py", [], "row_bound_packed_pinned.inc"),
    ("gen_row_bound_asm.py", [], "row_bound_pinned.inc"),
    ("gen_row_scan_asm.py", [], "row_scan_pinned.inc"),
])
def test_generated_scans_are_what_the_generators_write(tool, args, inc):
    """The committed .inc files are their generators' output: the single-cell ring scan the windowed kernel runs (both
    ring files: tests/test_pair_bound_ring_model.py), and the three older ones as before."""
    out = subprocess.run([sys.executable, str(ROOT / "tools" / tool), *args], capture_output=True, text=True, check=True)
    assert out.stdout == (CSRC / inc).read_text()


def chem_cases(tmp_path):
    cases = [("stock", None, {})] + [(name, None, kw) for name, kw in EDGE_CHEMS.items()]
    cases.append(("long_loops_cheap", pv.write_bundle(long_loops_cheap_sections(), tmp_path / "long_loops_cheap.bundle"), {}))
    return cases


def test_constants_are_the_minima_over_the_coarse_tables(m, tmp_path):
    for name, path, kw in chem_cases(tmp_path):
        pk = window_tables(m, path, m.Chem.ntthal(**kw), THR)
        w = pk["window"]
        assert pk["usable"] == 1 and w["usable"] == 1 and w["F"] in (2, 3), name
        ifar, bfar = far_constants(pk, w["F"])
        assert w["ifar"] == (w["void"] if ifar is None else ifar), name
        assert w["bfar"] == (w["void"] if bfar is None else bfar), name
        assert w["void"] == 1 << 26 and pk["hi"] + pk["bias"] < pk["field_max"]      # no real field is farmin's "no cell"
        print(f"{name}: F {w['F']}, ifar {w['ifar']}, bfar {w['bfar']} (unit {pk['unit']} cal/mol)")
    stock = window_tables(m)
    assert stock["window"]["ifar"] < stock["window"]["void"] and stock["window"]["bfar"] < stock["window"]["void"]
    cheap = window_tables(m, pv.write_bundle(long_loops_cheap_sections(), tmp_path / "llc.bundle"))
    assert min(cheap["window"]["ifar"], cheap["window"]["bfar"]) < 0      # the bundle whose far entries are negative


def check_pairs(bt, pk, pairs, dg_of=None):
    """windowed <= packed <= exact (<= dG + margin) for every pair, chains exactly where the exact model has them, every
    cell value inside [lo, hi]; returns (pairs with a chain, pairs the window lowered, largest packed - windowed in cal/mol)."""
    n_chain, n_lower, gap = 0, 0, 0.0
    for a, b in pairs:
        values, _ = cells_and_pick(pk, a, b)
        assert all(pk["lo"] <= v <= pk["hi"] for v in values), (a, b, min(values), max(values), pk["lo"], pk["hi"])
        lbw, lbq, lb = window_bound_pair(pk, a, b), packed_bound_pair(pk, a, b), bound_pair(bt, a, b)
        assert (lbw is None) == (lbq is None) == (lb is None), (a, b)
        if lb is None:
            continue
        assert lbw <= lbq <= lb, (a, b, lbw, lbq, lb)
        if dg_of is not None:
            assert lb <= dg_of(a, b) + 1.0, (a, b, lb)
        n_chain, n_lower, gap = n_chain + 1, n_lower + (lbw < lbq), max(gap, lbq - lbw)
    return n_chain, n_lower, gap


def test_windowed_is_below_packed_is_below_exact_is_below_the_oracle(m, oracle, tmp_path):
    for name, path, kw in chem_cases(tmp_path):
        chem = m.Chem.ntthal(**kw)
        bt, pk = m.capi.host_bound_tables(path, chem, THR), window_tables(m, path, chem, THR)
        tables = oracle.Tables(path) if path else oracle.Tables()
        pool = mixed_pool(13, 40, seed=5100)
        _, dg, _, _ = oracle.pool_pairs(tables, pool, oracle.ntthal_args(**kw), THR)
        at = {p: i for i, p in enumerate(pool)}
        n, low, gap = check_pairs(bt, pk, [(a, b) for a in pool for b in pool], lambda a, b: dg[at[a], at[b]])
        n2, _, _ = check_pairs(bt, pk, EXTREMES)
        print(f"{name}: {n} + {n2} pairs with a chain, {low} lowered by the window, by at most {gap:.0f} cal/mol")
        assert n > 0 and n2 == len(EXTREMES)


def test_two_stem_family_and_shorter_oligos(m, oracle, oracle_tables, tmp_path):
    bt, pk = m.capi.host_bound_tables(None, m.Chem.ntthal(), THR), window_tables(m)
    n, low, gap = check_pairs(bt, pk, two_stem_family(), lambda a, b: oracle.thal(oracle_tables, a, b).dG)
    print(f"two-stem family: {low} of {n} lowered by the window, by at most {gap:.0f} cal/mol")
    assert n == 536
    path = pv.write_bundle(long_loops_cheap_sections(), tmp_path / "long_loops_cheap.bundle")
    btc, pkc = m.capi.host_bound_tables(path, m.Chem.ntthal(), THR), window_tables(m, path)
    tables = oracle.Tables(path)
    n, low, _ = check_pairs(btc, pkc, two_stem_family(), lambda a, b: oracle.thal(tables, a, b).dG)
    assert n == 536 and low > 0      # negative far entries: the relaxation acts
    F = pk["window"]["F"]
    for k in (9, F + 1):
        pool = mixed_pool(k, 40, seed=5100 + k)
        _, dg, _, _ = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(), THR)
        at = {p: i for i, p in enumerate(pool)}
        n, low, _ = check_pairs(bt, pk, [(a, b) for a in pool for b in pool], lambda a, b: dg[at[a], at[b]])
        assert n > 0
        if k <= F + 1:      # no row above any window
            assert low == 0


def test_plane_model_is_the_pair_model(m, tmp_path):
    """plane_model (what the GPU suite compares whole planes with) against cells_and_pick: pick, no chain, and the
    extremes of the cell values -- stock tables and the bundle with negative far entries."""
    path = pv.write_bundle(long_loops_cheap_sections(), tmp_path / "long_loops_cheap.bundle")
    for pk in (window_tables(m), window_tables(m, path)):
        for k in (13, 9, 3):
            pool = mixed_pool(k, 14, seed=5300 + k)
            got, vmin, vmax = plane_model(pk, pool, pool)
            lo, hi = NONE, -NONE
            for i, a in enumerate(pool):
                for j, b in enumerate(pool):
                    values, pick = cells_and_pick(pk, a, b)
                    assert got[i, j] == (NONE if pick is None else pick), (a, b)
                    if values:
                        lo, hi = min(lo, min(values)), max(hi, max(values))
            assert (vmin, vmax) == (lo, hi)


def test_unusable_where_the_packed_instance_is(m, tmp_path):
    path = pv.write_bundle(unpackable_sections(), tmp_path / "unpackable.bundle")
    chem = m.Chem.ntthal()
    assert m.capi.host_bound_tables(path, chem, THR)["usable"] == 1 and m.capi.host_bound_packed(path, chem, THR)["usable"] == 0
    w = m.capi.host_bound_window(path, chem, THR)
    assert w["usable"] == 0 and w["ifar"] == w["bfar"] == w["void"]
    assert m.capi.host_bound_window(None, chem, 500.0)["usable"] == 0
    assert m.capi.host_bound_window(None, m.Chem.ntthal(temp_c=-1.0), THR)["usable"] == 0
