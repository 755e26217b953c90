"""The packed bound first stage without a GPU (option pair_bound_packed; csrc/nn_params.cpp build_bound_packed through
msspe_host_bound_packed; tests/pair_bound_packed_model.py).

Tables: every coarse entry is floor(exact-unit entry / 2^shift), void mirrors void, the cut is floored likewise, and
shift is the smallest whose proven range fits the slot word's field.  Argument: the model on the coarse tables <= the
model on the exact-unit tables <= the oracle's dG (+ the margin), pair for pair; and every cell value the coarse model
produces lies inside the exported range [lo, hi], which fits the 15-bit field with the bias -- GC-rich extremes
included.  A bundle whose range fits no shift reports usable = 0."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import param_variants as pv
from pair_bound_model import EDGE_CHEMS, bound_pair, long_loops_cheap_sections, mixed_pool, rc, two_stem_family
from pair_bound_packed_model import NONE, cells_and_pick, packed_bound_pair, packed_tables, plane_model, unpackable_sections

ROOT = Path(__file__).resolve().parent.parent
THR = -9000.0
PK_REACH, PK_OFF, PK_YVOID = 1 << 20, 1 << 28, 1 << 26   # fast_tables.hpp BoundPacked::kReach; thal_pairs_row.hip kPkOff, kPkYVoid


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


def test_generated_packed_scan_is_what_the_generator_writes():
    """open-msspe-design_amd/csrc/row_bound_packed_pinned.inc is generated: the committed file is the generator's output."""
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_row_bound_packed_asm.py")], capture_output=True, text=True,
                         check=True)
    assert out.stdout == (ROOT / "open-msspe-design_amd" / "csrc" / "row_bound_packed_pinned.inc").read_text()


def chem_cases(m, tmp_path):
    """(name, bundle path | None, Chem keywords): stock, every corner of the chemistry domain, long loops made cheap."""
    cases = [("stock", None, {})] + [(name, None, kw) for name, kw in EDGE_CHEMS.items()]
    cases.append(("long_loops_cheap", pv.write_bundle(long_loops_cheap_sections(), tmp_path / "long_loops_cheap.bundle"), {}))
    return cases


def check_tables(bt, pk):
    assert bt["usable"] == 1 and pk["usable"] == 1
    s, void = pk["shift"], bt["void"]
    assert 6 <= s <= 8
    for name in ("g", "T"):
        ex, co = bt[name].astype(np.int64), pk[name].astype(np.int64)
        fin = ex < void
        np.testing.assert_array_equal(co[fin], ex[fin] >> s)          # floor: numpy's >> on negative int64 is arithmetic
        np.testing.assert_array_equal(co[~fin], ex[~fin])             # void mirrors void
        assert (np.abs(co[fin]) < PK_REACH).all()
    assert pk["init"] == bt["init"] >> s and pk["cut"] == bt["cut"] >> s
    # the cull rule lbq > cutq implies lbq * 2^s > cut: the margin is spent exactly as before
    assert (pk["cut"] + 1) << s > bt["cut"]
    # the field: [lo, hi] + bias inside 0 .. field_max, and the kernel's "not available" arithmetic
    assert pk["field_max"] == (1 << 15) - 1
    assert 0 <= pk["lo"] + pk["bias"] and pk["hi"] + pk["bias"] <= pk["field_max"] and 0 <= pk["bias"] < PK_REACH
    assert PK_OFF - 3 * PK_REACH - PK_YVOID > 0x7fff + PK_REACH and PK_OFF + 3 * PK_REACH + PK_YVOID + 0x7fff + PK_REACH < 2**31


def proven_range(pk, k=13):
    """build_bound_packed's range, restated: the most negative left end term + (k - 1) x the most negative step (a table
    entry or stacked pair, plus the most negative cell-side term); the largest finite left end term."""
    import int_dp_model as im
    g, T, void = pk["g"].astype(np.int64), pk["T"].astype(np.int64), pk["void"]
    fmin = lambda a: int(a[a < void].min()) if (a < void).any() else 0
    step = min(0, fmin(T), fmin(g[im.K_WC:im.K_WC + 16]))
    side = min(0, fmin(g[im.K_TSC:im.K_ZERO]))
    endl = g[im.K_ENDL:im.K_ENDL + 100]
    return fmin(endl) + (k - 1) * (step + side), int(endl[endl < void].max())


def test_coarse_tables_are_the_floored_exact_ones(m, tmp_path):
    for name, path, kw in chem_cases(m, tmp_path):
        chem = m.Chem.ntthal(**kw)
        bt, pk = m.capi.host_bound_tables(path, chem, THR), packed_tables(m, path, chem, THR)
        check_tables(bt, pk)
        lo, hi = proven_range(pk)
        assert (pk["lo"], pk["hi"]) == (lo, hi), name
        # the smallest shift that fits: the range of the next finer unit must not
        if pk["shift"] > 6:
            finer = {"g": np.where(bt["g"] < bt["void"], bt["g"] >> (pk["shift"] - 1), bt["g"]),
                     "T": np.where(bt["T"] < bt["void"], bt["T"] >> (pk["shift"] - 1), bt["T"]), "void": bt["void"]}
            flo, fhi = proven_range(finer)
            assert fhi - flo > pk["field_max"], name
        print(f"{name}: shift {pk['shift']}, range [{lo}, {hi}], bias {pk['bias']}")


def check_pairs(bt, pk, pairs, dg_of=None):
    """coarse <= exact (<= dG + margin) for every pair, chains exactly where the exact model has them, every cell value
    inside [lo, hi]; returns (pairs with a chain, largest exact - coarse in cal/mol)."""
    n_chain, gap = 0, 0.0
    for a, b in pairs:
        values, _ = cells_and_pick(pk, a, b)
        assert all(pk["lo"] <= v <= pk["hi"] for v in values), (a, b, min(values), max(values), pk["lo"], pk["hi"])
        lbq, lb = packed_bound_pair(pk, a, b), bound_pair(bt, a, b)
        assert (lbq is None) == (lb is None), (a, b)
        if lb is None:
            continue
        assert lbq <= lb, (a, b, lbq, lb)
        if dg_of is not None:
            assert lb <= dg_of(a, b) + 1.0, (a, b, lb)
        n_chain, gap = n_chain + 1, max(gap, lb - lbq)
    return n_chain, gap


EXTREMES = [(("GC" * 7)[:13], rc(("GC" * 7)[:13])), ("G" * 13, "C" * 13), ("C" * 13, "G" * 13),
            (("CG" * 7)[:13], rc(("CG" * 7)[:13]))]


def test_coarse_bound_is_below_the_exact_bound_is_below_the_oracle(m, oracle, tmp_path):
    for name, path, kw in chem_cases(m, tmp_path):
        chem = m.Chem.ntthal(**kw)
        bt, pk = m.capi.host_bound_tables(path, chem, THR), packed_tables(m, path, chem, THR)
        tables = oracle.Tables(path) if path else oracle.Tables()
        pool = mixed_pool(13, 40, seed=5100)
        _, dg, _, _ = oracle.pool_pairs(tables, pool, oracle.ntthal_args(**kw), THR)
        at = {p: i for i, p in enumerate(pool)}
        n, gap = check_pairs(bt, pk, [(a, b) for a in pool for b in pool], lambda a, b: dg[at[a], at[b]])
        # GC-rich extremes: the most negative chains there are
        n2, gap2 = check_pairs(bt, pk, EXTREMES)
        print(f"{name}: {n} + {n2} pairs with a chain, exact - coarse at most {max(gap, gap2):.3f} cal/mol (unit {pk['unit']})")
        assert n > 0 and n2 == len(EXTREMES)
        # a chain of 13 pairs floors at most 27 terms: 2 end terms, 12 steps of at most 2, the initiation
        assert max(gap, gap2) < 27 * pk["unit"]


def test_two_stem_family_and_shorter_oligos(m, oracle, oracle_tables, tmp_path):
    bt, pk = m.capi.host_bound_tables(None, m.Chem.ntthal(), THR), packed_tables(m)
    n, gap = check_pairs(bt, pk, two_stem_family(), lambda a, b: oracle.thal(oracle_tables, a, b).dG)
    assert n == 536
    path = pv.write_bundle(long_loops_cheap_sections(), tmp_path / "long_loops_cheap.bundle")
    btc, pkc = m.capi.host_bound_tables(path, m.Chem.ntthal(), THR), packed_tables(m, path)
    tables = oracle.Tables(path)
    n, _ = check_pairs(btc, pkc, two_stem_family(), lambda a, b: oracle.thal(tables, a, b).dG)
    assert n == 536
    for k in (9, 12):
        pool = mixed_pool(k, 40, seed=5100 + k)
        _, dg, _, _ = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(), THR)
        at = {p: i for i, p in enumerate(pool)}
        n, gap = check_pairs(bt, pk, [(a, b) for a in pool for b in pool], lambda a, b: dg[at[a], at[b]])
        print(f"k = {k}: {n} pairs with a chain, exact - coarse at most {gap:.3f} cal/mol")
        assert n > 0


def test_plane_model_is_the_pair_model(m):
    """plane_model (numpy over the pairs; what the GPU suite compares whole planes with) against cells_and_pick, on
    the coarse and on the exact-unit tables: pick, no chain, and the extremes of the cell values."""
    bt, pk = m.capi.host_bound_tables(None, m.Chem.ntthal(), THR), packed_tables(m)
    for k in (13, 9):
        pool = mixed_pool(k, 14, seed=5300 + k)
        for tables in (pk, bt):
            got, vmin, vmax = plane_model(tables, pool, pool)
            lo, hi = NONE, -NONE
            for i, a in enumerate(pool):
                for j, b in enumerate(pool):
                    values, pick = cells_and_pick(tables, a, b)
                    assert got[i, j] == (NONE if pick is None else pick), (a, b)
                    if values:
                        lo, hi = min(lo, min(values)), max(hi, max(values))
            assert (vmin, vmax) == (lo, hi)


def test_unusable_where_no_shift_holds_the_range(m, tmp_path):
    path = pv.write_bundle(unpackable_sections(), tmp_path / "unpackable.bundle")
    chem = m.Chem.ntthal()
    bt, pk = m.capi.host_bound_tables(path, chem, THR), m.capi.host_bound_packed(path, chem, THR)
    assert bt["usable"] == 1 and pv.routes_tuple(m.capi.host_table_routes(path))[:4] == (1, 1, 1, 1)
    assert pk["usable"] == 0 and pk["shift"] == 0 and not pk["g"].any() and not pk["T"].any()
    coarsest = {"g": np.where(bt["g"] < bt["void"], bt["g"] >> 8, bt["g"]), "T": np.where(bt["T"] < bt["void"], bt["T"] >> 8, bt["T"]),
                "void": bt["void"]}
    lo, hi = proven_range(coarsest)
    assert hi - lo > (1 << 15) - 1
    # 4000 instead of 6000: the coarsest unit holds it
    path4 = pv.write_bundle(pv._mapped(pv.stock_sections(), {"tstack.dh": lambda i, v: v - 4000}), tmp_path / "unit4.bundle")
    pk4 = packed_tables(m, path4)
    assert pk4["usable"] == 1 and pk4["shift"] == 8
    check_tables(m.capi.host_bound_tables(path4, chem, THR), pk4)
    # where the bound stage itself does not apply, neither does this
    assert m.capi.host_bound_packed(None, chem, 500.0)["usable"] == 0
    assert m.capi.host_bound_packed(None, m.Chem.ntthal(temp_c=-1.0), THR)["usable"] == 0
