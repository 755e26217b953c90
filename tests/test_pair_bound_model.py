"""The bound first stage's tables and its lower-bound argument, without a GPU (csrc/nn_params.cpp build_bound_tables
through msspe_host_bound_tables; tests/pair_bound_model.py restates the kernel's min-plus recurrence).

Tables: every integer entry times the unit is at most the exact double H - temp_k (S [+ salt]); void stays void; every
entry and every reachable sum fits the kernel's int32 arithmetic with its zero offset.  Argument: on a seeded pool the
model's bound never exceeds the oracle's dG, and stays close to it -- at every length the stage runs for (2 .. 13) and at
the corners of the chemistry domain build_bound_tables admits, where `usable` must flip.  Inputs of the GPU value tests
(tests/test_gpu_pair_bound_values.py): the sizing helpers, and the loop shapes the two-stem family's winning chains use."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import int_dp_model as im
import param_variants as pv
from pair_bound_model import (EDGE_CHEMS, UNUSABLE_CHEMS, bound_pair, bound_pair_trace, bounded_in_uniform_wave,
                              long_loops_cheap_sections, mixed_pool, rc, stored_cells, two_stem_family)

ROOT = Path(__file__).resolve().parent.parent
H_INF = 1 << 28                    # nn_params.hpp kHInf
BND_ZERO, BND_YVOID = 1 << 29, 1 << 28   # thal_pairs_row.hip kBndZero, kBndYVoid


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


def test_generated_bound_scan_is_what_the_generator_writes():
    """open-msspe-design_amd/csrc/row_bound_pinned.inc is generated: the committed file is the generator's output."""
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_row_bound_asm.py")], capture_output=True, text=True, check=True)
    assert out.stdout == (ROOT / "open-msspe-design_amd" / "csrc" / "row_bound_pinned.inc").read_text()


def exact_terms(tb, chem_salt_steps):
    """H - temp_k (S + steps * salt) of every FastTables entry; +inf: not available."""
    g = tb.H.astype(np.float64) - tb.temp_k * (tb.S + chem_salt_steps * tb.salt)
    g[tb.H >= H_INF] = np.inf
    return g


@pytest.mark.parametrize("variant", ["stock", "loops_and_bonuses"])
@pytest.mark.parametrize("chem_kw", [{}, {"temp_c": 37.0}, {"mv": 600.0, "dv": 20.0}])
def test_bound_tables_round_down_and_fit(m, tmp_path, variant, chem_kw):
    path = None if variant == "stock" else pv.write_bundle(pv.variant_sections(variant), tmp_path / "v.bundle")
    chem = m.Chem.ntthal(**chem_kw)
    bt = m.capi.host_bound_tables(path, chem, -9000.0)
    tb = im.load_tables(m, -9000.0, path) if not chem_kw else None
    if tb is None:   # load_tables() reads ntthal's defaults: restate it for this chemistry
        import ctypes as C
        S, H = np.zeros(im.K_COUNT), np.zeros(im.K_COUNT, dtype=np.int32)
        g, T = np.zeros(im.K_COUNT, dtype=np.int32), np.zeros(im.K_ROWS * 64, dtype=np.int32)
        consts = (C.c_double * 8)()
        L = m.capi.load_library()
        L.msspe_host_pair_tables.argtypes = [C.c_char_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.POINTER(C.c_double)]
        assert L.msspe_host_pair_tables(str(path).encode() if path else None, C.byref(chem), C.c_float(-9000.0),
                                        S.ctypes.data, H.ctypes.data, g.ctypes.data, T.ctypes.data, consts) == 0
        tb = im.PairTables(S, H, g, T, consts[0], consts[1], consts[2], consts[3], consts[4], True, True)
    assert bt["usable"] == 1 and bt["unit_inv"] == 64 and bt["margin"] == 64
    if "mv" in chem_kw:
        assert tb.salt > 0      # the per-pair step - temp_k * salt is negative
    u, void, reach = bt["unit_inv"], bt["void"], bt["reach"]
    plain, step = exact_terms(tb, 0), exact_terms(tb, 1)
    # ---- the flat entries: stacked pairs carry the step's salt term, everything else is as it is
    for e in range(im.K_COUNT):
        want = step[e] if im.K_WC <= e < im.K_WC + 16 else plain[e]
        if not np.isfinite(want):
            assert bt["g"][e] >= void, e
            continue
        assert bt["g"][e] < void
        assert bt["g"][e] / u <= want < (bt["g"][e] + 1) / u + 1e-9, e
    # ---- the loop table
    n_valid = 0
    for d in range(1, im.K_ROWS):
        l1, l2 = d >> 4, d & 15
        sz = l1 + l2
        for pe in range(64):
            got = int(bt["T"][d * 64 + pe])
            want = np.inf
            if l1 <= 14 and l2 <= 14 and sz <= im.K_MAXSZ:
                if l1 == 0 or l2 == 0:
                    if pe < 16:
                        want = step[im.K_BU + (pe >> 2) * im.K_BUSTRIDE + sz * 4 + (pe & 3)]
                else:
                    want = step[im.K_NB + (sz - 2) * 64 + pe]
                    if d != 0x11 and np.isfinite(want):
                        want -= tb.temp_k * tb.S[im.K_ZT + 32 + (l1 - l2)]
            if not np.isfinite(want):
                assert got >= void, (d, pe)
                continue
            n_valid += 1
            assert got < void and got / u <= want + 1e-9 and want < (got + 1) / u + 1e-9, (d, pe, got, want)
    assert n_valid > 5000 and int(bt["T"][0]) >= void    # d = 0: the stacked pair is no loop entry of this table
    assert bt["init"] / u <= 200.0 - tb.temp_k * tb.init_S < (bt["init"] + 1) / u
    assert bt["cut"] == int(np.floor((tb.g_cut + bt["margin"] / u) * u))
    # ---- int32 with the zero offset: a chain of 13 pairs takes a loop or stack term and at most one cell-side term per
    #      step, two end terms and the initiation
    mag = lambda a: np.abs(a[a < void]).max()
    step_max = max(mag(bt["T"]), mag(bt["g"][im.K_WC:im.K_WC + 16]))
    mm = mag(bt["g"][im.K_TSC:im.K_ZERO])
    en = mag(bt["g"][im.K_ENDL:im.K_WC])
    assert 13 * (step_max + mm) + 2 * en + abs(bt["init"]) < reach
    # the kernel's stored forms: entries - kBndZero (a folded-out void cell-side term included), slot values + kBndZero,
    # and the largest candidate
    assert -reach - BND_YVOID - BND_ZERO > -2**31 and reach + BND_ZERO < 2**31 and BND_ZERO + BND_YVOID + reach < 2**31


def test_a_cut_above_zero_is_not_usable(m):
    assert m.capi.host_bound_tables(None, m.Chem.ntthal(), 500.0)["usable"] == 0
    assert m.capi.host_bound_tables(None, m.Chem.ntthal(), 0.0)["usable"] == 1


@pytest.mark.parametrize("chem_kw", [{}, {"temp_c": 37.0, "mv": 600.0, "dv": 20.0}])
def test_model_bound_is_below_the_oracle(m, oracle, oracle_tables, chem_kw):
    """50 seeded 13-mers plus a perfect duplex: bound <= dG for every pair with a structure (E = 1 cal/mol is not even
    needed here), no chain exactly where the oracle finds no structure's cells, and a mean distance of tens of cal/mol."""
    pool = m.synth.pool_strings(m.synth.random_pool(50, 13, seed=77))
    pool += ["GCCAGTTCGGATA", oracle.reverse_complement("GCCAGTTCGGATA")]
    bt = m.capi.host_bound_tables(None, m.Chem.ntthal(**chem_kw), -9000.0)
    _, dg, _, _ = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(**chem_kw), -9000.0)
    gaps = []
    for i, a in enumerate(pool):
        for j, b in enumerate(pool):
            lb = bound_pair(bt, a, b)
            if lb is None:
                assert not np.isfinite(dg[i, j])
            elif np.isfinite(dg[i, j]):
                assert lb <= dg[i, j] + 1.0, (a, b, lb, dg[i, j])
                gaps.append(dg[i, j] - lb)
    gaps = np.array(gaps)
    print(f"bound below dG by {gaps.mean():.2f} on average, {gaps.min():.4f} at least")
    assert gaps.min() > -1.0 and gaps.mean() < 100.0


# ---- the model against the oracle at every length and at the corners of the chemistry domain ---------------------------
def check_model_below_oracle(m, oracle, oracle_tables, k, chem_kw):
    pool = mixed_pool(k, 40, seed=4200 + k)
    bt = m.capi.host_bound_tables(None, m.Chem.ntthal(**chem_kw), -9000.0)
    assert bt["usable"] == 1
    _, dg, _, _ = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(**chem_kw), -9000.0)
    worst, n_chain = -np.inf, 0
    for i, a in enumerate(pool):
        for j, b in enumerate(pool):
            lb = bound_pair(bt, a, b)
            # no chain exactly where the oracle finds no structure
            assert (lb is None) == (not np.isfinite(dg[i, j])), (a, b, lb, dg[i, j])
            if lb is not None:
                assert lb <= dg[i, j] + 1.0, (a, b, lb, dg[i, j])
                worst, n_chain = max(worst, lb - dg[i, j]), n_chain + 1
    print(f"k={k} {chem_kw}: {n_chain} of {len(pool) ** 2} pairs with a chain, worst lb - dG = {worst:.4f} cal/mol")
    assert n_chain > 0


@pytest.mark.parametrize("k", range(2, 14))
def test_model_bound_is_below_the_oracle_at_every_length(m, oracle, oracle_tables, k):
    check_model_below_oracle(m, oracle, oracle_tables, k, {})


@pytest.mark.parametrize("k", [7, 13])
@pytest.mark.parametrize("chem_name", list(EDGE_CHEMS))
def test_model_bound_is_below_the_oracle_at_the_chemistry_edges(m, oracle, oracle_tables, k, chem_name):
    check_model_below_oracle(m, oracle, oracle_tables, k, EDGE_CHEMS[chem_name])


def test_usable_flips_where_build_bound_tables_says(m):
    """273.15 K <= temp_k <= 373.15 K and a finite salt term (mv = dv = 0: the logarithm of no salt at all)."""
    usable = lambda **kw: m.capi.host_bound_tables(None, m.Chem.ntthal(**kw), -9000.0)["usable"]
    assert usable(temp_c=0.0) == 1 and usable(temp_c=100.0) == 1
    assert usable(temp_c=-1.0) == 0 and usable(temp_c=100.5) == 0
    assert usable(mv=0.0, dv=0.0) == 0
    for name, kw in EDGE_CHEMS.items():
        assert usable(**kw) == 1, name
    for name, kw in UNUSABLE_CHEMS.items():
        assert usable(**kw) == 0, name


def test_trace_and_sizing_helpers():
    # one pair of the family by hand: GCC AAA CGC against rc(CGC) AA rc(GCC) -> the loop (3, 2)
    fam = dict(((a, b), None) for a, b in two_stem_family())
    assert len(fam) == 536 and ("GCCAAACGCAAAA", "AAAAAGCGAAGGC") in fam
    assert all(len(a) == 13 and len(b) == 13 for a, b in fam)
    assert len(two_stem_family(5)) == sum(1 for sA, sB in (("GC", "CG"), ("G", "C"), ("GC", "C"))
                                          for l1 in range(12) for l2 in range(12)
                                          if (l1, l2) != (0, 0) and len(sA) + len(sB) + max(l1, l2) <= 5)
    # A*13 x T*13: 169 cells, 13 of them in the last row; the perfect duplex of a mixed oligo is far smaller
    assert stored_cells("A" * 13, "T" * 13) == 156 and not bounded_in_uniform_wave("A" * 13, "T" * 13)
    assert stored_cells("A" * 13, "A" * 13) == 0 and bounded_in_uniform_wave("A" * 13, "A" * 13)
    assert stored_cells("ACGT", "ACGT") == 4 - 1 and not bounded_in_uniform_wave("ACGT", "ACGT")   # both self-complementary
    assert bounded_in_uniform_wave("ACGT", "ACGA") and rc("AACG") == "CGTT"
    # 4 C x 4 G + 2 G x 2 C cells, the last row (A) finds no T; with a fifth C as the last row, its 4 cells are not stored
    assert stored_cells("GCCAAACGCAAAA", "AAAAAGCGAAGGC") == 20 and stored_cells("GCCAAACGCAAAC", "AAAAAGCGAAGGC") == 24 - 4


def family_shapes(bt):
    shapes = set()
    for a, b in two_stem_family():
        lb, tr = bound_pair_trace(bt, a, b)
        assert lb == bound_pair(bt, a, b) and lb is not None
        shapes.update(tr)
    return shapes


def test_the_family_covers_the_loop_shapes(m, tmp_path):
    """Conditions on the inputs of tests/test_gpu_pair_bound_values.py, not on the kernel: the winning chains of the
    two-stem family must use many loop shapes, long ones included.  A table change that breaks this calls for another
    family, not for a lower cap."""
    stock = family_shapes(m.capi.host_bound_tables(None, m.Chem.ntthal(), -9000.0))
    path = pv.write_bundle(long_loops_cheap_sections(), tmp_path / "long_loops_cheap.bundle")
    cheap = family_shapes(m.capi.host_bound_tables(path, m.Chem.ntthal(), -9000.0))
    print(f"stock: {len(stock)} shapes, longest side {max(max(s) for s in stock)}; "
          f"long_loops_cheap: {len(cheap)} shapes, longest side {max(max(s) for s in cheap)}")
    assert len(stock) >= 40
    assert len(cheap) >= 95 and max(max(s) for s in cheap) >= 9


def test_long_loops_cheap_keeps_every_route(m, oracle, tmp_path):
    path = pv.write_bundle(long_loops_cheap_sections(), tmp_path / "long_loops_cheap.bundle")
    assert pv.routes_tuple(m.capi.host_table_routes(path)) == (1, 1, 1, 1, 32, 32)
    assert m.capi.host_bound_tables(path, m.Chem.ntthal(), -9000.0)["usable"] == 1
    assert m.capi.host_bound_mirror_ok(path)
    # the bound stays a bound under it: the family and 60 random 13-mers against the oracle on the same file
    tables = oracle.Tables(path)
    bt = m.capi.host_bound_tables(path, m.Chem.ntthal(), -9000.0)
    worst = -np.inf
    for a, b in two_stem_family():
        worst = max(worst, bound_pair(bt, a, b) - oracle.thal(tables, a, b).dG)
    pool = mixed_pool(13, 60, seed=4300)[:60]
    _, dg, _, _ = oracle.pool_pairs(tables, pool, oracle.ntthal_args(), -9000.0)
    for i, a in enumerate(pool[:20]):
        for j, b in enumerate(pool):
            lb = bound_pair(bt, a, b)
            assert (lb is None) == (not np.isfinite(dg[i, j]))
            if lb is not None:
                worst = max(worst, lb - dg[i, j])
    print(f"long_loops_cheap: worst lb - dG = {worst:.4f} cal/mol")
    assert worst <= 1.0
