"""The oracle's primer3_core view (check_primers) at chemistries other than Primer3's defaults, checked on its own:
the default entry points are unchanged, oligotm() equals an independent restatement of Primer3 2.6.1 bit for bit on
every branch of its salt handling, thal's temperature and maxLoop leave Tm alone, and every chemistry of the GPU
parity matrix (tests/test_gpu_stage_b_chemistry.py) moves the statistics it is there for."""
import json
import math

import numpy as np
import pytest

from helpers import (STAGE_B_CHEMS, STAGE_B_FAMILY_KS, reverse_complement, stage_b_pool)

FIELDS = ("tm", "gc", "self_any_th", "self_end_th", "hairpin_th")

# SantaLucia (1998) unified nearest-neighbour parameters, the ten distinct Watson-Crick stacks (5'->3' / 3'->5'):
# dH in kcal/mol, dS in cal/(K mol).  The other six follow from reading the duplex from the other strand.
UNIFIED = {"AA": (-7.9, -22.2), "AT": (-7.2, -20.4), "TA": (-7.2, -21.3), "CA": (-8.5, -22.7),
           "GT": (-8.4, -22.4), "CT": (-7.8, -21.0), "GA": (-8.2, -22.2), "CG": (-10.6, -27.2),
           "GC": (-9.8, -24.4), "GG": (-8.0, -19.9)}
# initiation with a terminal A.T / G.C pair and the symmetry correction, same units
INIT_AT, INIT_GC, SYMMETRY_DS = (2.3, 4.1), (0.1, -2.8), -1.4


def _nn_tenths():
    """dH in 100 cal/mol and dS in 0.1 cal/(K mol) as exact integers, the way oligotm.c sums them."""
    nn = {}
    for pair, (h, s) in UNIFIED.items():
        for key in (pair, reverse_complement(pair)):
            nn[key] = (round(h * 10), round(s * 10))
    assert len(nn) == 16
    return nn


NN = _nn_tenths()


def oligotm(s, dna_conc, mv, dv, dntp, sym=None):
    """Primer3 2.6.1 oligotm(), tm_method santalucia, salt_corrections santalucia; None = OLIGOTM_ERROR."""
    n = len(s)
    if sym is None:
        sym = n % 2 == 0 and s == reverse_complement(s)
    dh, ds = 0, round(SYMMETRY_DS * 10) if sym else 0
    for end in (s[0], s[-1]):
        h, e = INIT_AT if end in "AT" else INIT_GC
        dh += round(h * 10)
        ds += round(e * 10)
    for a, b in zip(s, s[1:]):
        dh += NN[a + b][0]
        ds += NN[a + b][1]
    delta_h = dh * 100.0
    delta_s = ds * 0.1
    # divalent_to_monovalent()
    if dv == 0:
        dntp = 0
    if dv < 0 or dntp < 0:
        return None
    if dv < dntp:
        dv = dntp
    k_mm = mv + 120 * math.sqrt(dv - dntp)
    delta_s = delta_s + 0.368 * (n - 1) * math.log(k_mm / 1000.0)
    return delta_h / (delta_s + 1.987 * math.log(dna_conc / (1e9 if sym else 4e9))) - 273.15


def _tm_pool():
    rng = np.random.default_rng(17)
    pool = []
    for k in range(2, 33):
        pool += ["".join("ACGT"[x] for x in rng.integers(0, 4, k)) for _ in range(6)]
        if k % 2 == 0:
            for _ in range(4):
                half = "".join("ACGT"[x] for x in rng.integers(0, 4, k // 2))
                pool.append(half + reverse_complement(half))
        pool += [b * k for b in "ACGT"]
    return pool


def _check(oracle, oracle_tables, pool, **kw):
    return oracle.check_primers(oracle_tables, pool, oracle.p3_args(**kw))


def test_default_chemistry_entry_points_are_unchanged(oracle, oracle_tables, golden_dir):
    """check_primers without a chemistry = at p3_args() = the old C entry point, byte for byte, and the golden."""
    g = json.loads((golden_dir / "primer3_check_primers.json").read_text())["check_primers"][0]
    for k in (13, 20):
        pool = stage_b_pool(k, 1000 + k)
        if k == 13:
            pool.append(g["primer"])
        got = oracle.check_primers(oracle_tables, pool)
        at = oracle.check_primers(oracle_tables, pool, oracle.p3_args())
        old = np.zeros_like(got)
        assert oracle.lib().orc_check_primers(oracle_tables.ptr, "".join(pool).encode(), len(pool), k,
                                              old.ctypes.data) == 0
        assert got.tobytes() == at.tobytes() == old.tobytes()
        one = oracle.check_primer(oracle_tables, pool[-1])
        assert [getattr(one, f) for f in FIELDS] == [got[f][-1] for f in FIELDS]
        if k == 13:
            assert (got["tm_f32"][-1], got["gc_f32"][-1]) == (np.float32(g["tm"]), np.float32(g["gc"]))
            assert got["self_any_th"][-1] == got["self_end_th"][-1] == got["hairpin_th"][-1] == 0.0


@pytest.mark.parametrize("kw", [
    dict(),                                                     # Primer3's defaults
    dict(mv=50.0, dv=3.0, dntp=0.0, dna_conc=250.0),            # ntthal's
    dict(dv=0.0, dntp=0.6), dict(dv=0.0, dntp=-0.5),            # dv == 0: dNTP ignored, even a negative one
    dict(dv=0.3, dntp=0.6), dict(dv=0.6, dntp=0.6),             # dNTP >= dv: no divalent term
    dict(dv=2.5, dntp=0.6),
    dict(mv=0.5), dict(mv=10.0), dict(mv=200.0), dict(mv=1000.0, dv=0.0),
    dict(dna_conc=0.5), dict(dna_conc=5.0), dict(dna_conc=5000.0), dict(dna_conc=1e5)])
def test_oligotm_equals_a_restatement_of_primer3(oracle, oracle_tables, kw):
    pool = _tm_pool()
    a = oracle.p3_args(**kw)
    got = np.concatenate([oracle.check_primers(oracle_tables, [s for s in pool if len(s) == k], a)["tm"]
                          for k in range(2, 33)])
    want = [oligotm(s, a.dna_conc, a.mv, a.dv, a.dntp) for s in pool]
    assert got.tolist() == want
    assert [oracle.lib().orc_oligotm(s.encode(), a.dna_conc, a.mv, a.dv, a.dntp) for s in pool] == want
    # the self-complementary branch is taken (+1.4 e.u. ... 1 instead of 4 in the concentration term)
    sym = [i for i, s in enumerate(pool) if len(s) % 2 == 0 and s == reverse_complement(s)]
    assert len(sym) > 60
    assert all(oligotm(pool[i], a.dna_conc, a.mv, a.dv, a.dntp, sym=False) != got[i] for i in sym)


def test_oligotm_salt_branches_are_distinct(oracle):
    """The cases above are not one case: each rule of divalent_to_monovalent moves the Tm it produces."""
    s = "ACGTTGCAAGGCTTAC"
    tm = lambda **kw: oracle.lib().orc_oligotm(s.encode(), 50.0, kw.get("mv", 50.0), kw["dv"], kw["dntp"])
    assert tm(dv=0.0, dntp=0.6) == tm(dv=0.0, dntp=0.0) == tm(dv=0.0, dntp=-0.5)
    # without the "dv == 0 -> dntp = 0" rule a negative dNTP would count as divalent salt
    assert tm(dv=0.0, dntp=-0.5) != tm(dv=0.5, dntp=0.0)
    assert tm(dv=0.3, dntp=0.6) == tm(dv=0.6, dntp=0.6) == tm(dv=0.0, dntp=0.0)
    assert tm(dv=1.5, dntp=0.6) != tm(dv=0.0, dntp=0.0)
    for dv, dntp in ((-1.0, 0.0), (1.5, -0.1), (-0.5, -0.5)):
        assert tm(dv=dv, dntp=dntp) == -999999.9999
        assert oligotm(s, 50.0, 50.0, dv, dntp) is None


def test_temperature_and_loop_limit_change_no_tm(oracle, oracle_tables):
    """oligotm has neither: Tm and GC stay put whatever thal's temperature and maxLoop."""
    pool = stage_b_pool(16, 7)
    ref = _check(oracle, oracle_tables, pool)
    for kw in (dict(temp_c=10.0), dict(temp_c=60.0), dict(max_loop=0), dict(max_loop=3), dict(max_loop=7),
               dict(max_loop=20)):
        got = _check(oracle, oracle_tables, pool, **kw)
        assert got["tm"].tobytes() == ref["tm"].tobytes() and got["gc"].tobytes() == ref["gc"].tobytes()


@pytest.fixture(scope="module")
def family_pools(oracle, oracle_tables):
    pools = {k: stage_b_pool(k, 1000 + k) for k in STAGE_B_FAMILY_KS}
    return pools, {k: _check(oracle, oracle_tables, p) for k, p in pools.items()}


@pytest.mark.parametrize("name", [c for c in STAGE_B_CHEMS if STAGE_B_CHEMS[c][1]])
def test_every_gpu_chemistry_moves_what_it_targets(oracle, oracle_tables, family_pools, name):
    """Guard against a vacuous matrix: on the pools every chemistry meets on the GPU, each one changes some values
    of each statistic it is there for, compared with Primer3's defaults."""
    kw, targets = STAGE_B_CHEMS[name]
    pools, ref = family_pools
    changed = dict.fromkeys(targets, 0)
    for k, pool in pools.items():
        got = _check(oracle, oracle_tables, pool, **kw)
        for f in targets:
            changed[f] += int((got[f] != ref[k][f]).sum())
    assert all(v > 0 for v in changed.values()), changed


def test_the_pools_fold(family_pools):
    """The designed parts of the pools give non-zero SELF_ANY, SELF_END and HAIRPIN values to compare."""
    _, ref = family_pools
    for k in (13, 20, 32):
        for f in ("self_any_th", "self_end_th", "hairpin_th"):
            assert (ref[k][f] > 0).sum() >= 10, (k, f)

