"""Stage B (msspe_oligo_stats, _dev, _group and the primer3_core shim) at chemistries other than Primer3's defaults:
Tm, GC %, SELF_ANY_TH, SELF_END_TH and HAIRPIN_TH bit-exact against the oracle's check_primers at the same chemistry,
over every kernel family (k 2..32), through every route the engine can take, and with each statistic asked for alone.

The matrix (tests/helpers.py STAGE_B_CHEMS, stage_b_cases) crosses the salt rules of oligotm's divalent_to_monovalent,
the oligo concentration, thal's temperature and maxLoop (0, 3, 7 cut loops; 20 is below 2k - 4 for 13-mers, so the
self-dimers leave the one-lane-per-oligo kernels) with pools of random oligos, designed stem-loops, palindromes,
homopolymers and END1 corner cases.  tests/test_oracle_stage_b_chemistry.py checks that each chemistry moves the
statistics it is there for."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import STAGE_B_CHEMS, stage_b_cases, stage_b_pool

pytestmark = pytest.mark.gpu
BIN = Path(__file__).resolve().parent.parent / "open-msspe-design_amd" / "bin"
STATS = (("tm", "tm"), ("gc", "gc"), ("self_any", "self_any_th"), ("self_end", "self_end_th"),
         ("hairpin", "hairpin_th"))
# engine options of each route, and the values they return to
ROUTES = {"default": {}, "force_generic": {"force_generic": 1}, "self_lane_from=0": {"self_lane_from": 0},
          "self_lane_from=2^30": {"self_lane_from": 1 << 30}}
RESET = {"force_generic": 0, "self_lane_from": 81920}


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


def assert_stats(got, ref, what):
    for a, b in STATS:
        np.testing.assert_array_equal(got[a], ref[b], err_msg=f"{what}: {a}")


def routes(eng, pool, chem):
    """{route: oligo_stats} over the routes of ROUTES."""
    out = {}
    for route, opts in ROUTES.items():
        try:
            for key, v in opts.items():
                eng.set_option(key, v)
            out[route] = eng.oligo_stats(pool, chem)
        finally:
            for key in opts:
                eng.set_option(key, RESET[key])
    return out


def stats_alone(eng, m, pool, chem):
    """Each of the five statistics asked for alone through msspe_oligo_stats_dev (the other four pointers null)."""
    import torch
    n, k = len(pool), len(pool[0])
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    d_out = torch.full((5, n), -1.0, dtype=torch.float64, device="cuda")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for q, (name, _) in enumerate(STATS):
            eng.oligo_stats_dev(d_pool.data_ptr(), n, k, chem, **{"d_" + name: d_out[q].data_ptr()})
        torch.cuda.synchronize()
    finally:
        eng.reset_stream()
    host = d_out.cpu().numpy()
    return {name: host[q] for q, (name, _) in enumerate(STATS)}


@pytest.mark.parametrize("name,k", stage_b_cases())
def test_oligo_stats_bit_exact_at_chemistry(eng, m, oracle, oracle_tables, name, k):
    """All five statistics equal the oracle's at the chemistry, through the default route, the one-lane kernels over
    a global workspace (force_generic), self-dimers one lane per oligo where the chemistry allows it
    (self_lane_from 0) and one wave per oligo (self_lane_from 2^30); and each statistic alone on the device."""
    kw, _ = STAGE_B_CHEMS[name]
    pool = stage_b_pool(k, 1000 + k)
    chem = m.Chem.primer3(**kw)
    ref = oracle.check_primers(oracle_tables, pool, oracle.p3_args(**kw))
    for route, got in routes(eng, pool, chem).items():
        assert_stats(got, ref, f"{name} k={k} {route}")
    assert_stats(stats_alone(eng, m, pool, chem), ref, f"{name} k={k} alone")


def test_large_pool_at_a_chemistry(eng, m, oracle, oracle_tables):
    """From 8,192 oligos per call HAIRPIN_TH runs one lane per oligo by default: a pool above that, at a chemistry
    that moves every statistic (dv below dNTP, another temperature, a loop limit still >= 2k - 4), on every route."""
    kw = dict(mv=200.0, dv=0.5, dntp=0.6, dna_conc=500.0, temp_c=50.0, max_loop=25)
    pool = stage_b_pool(13, 4242, n_random=6000, n_stem_loops=3000)
    assert len(pool) >= 8192
    chem = m.Chem.primer3(**kw)
    ref = oracle.check_primers(oracle_tables, pool, oracle.p3_args(**kw))
    base = oracle.check_primers(oracle_tables, pool)
    for _, b in STATS:
        assert (ref[b] != base[b]).any() or b == "gc", b
    assert (ref["hairpin_th"] > 0).sum() > 1000 and (ref["self_any_th"] > 0).sum() > 500
    for route, got in routes(eng, pool, chem).items():
        assert_stats(got, ref, route)
    assert_stats(stats_alone(eng, m, pool, chem), ref, "alone")


@pytest.mark.parametrize("name,k", [("ntthal", 20), ("loop3", 13)])
def test_group_oligo_stats_at_chemistry(m, oracle, oracle_tables, name, k):
    kw, _ = STAGE_B_CHEMS[name]
    pool = stage_b_pool(k, 1000 + k)
    g = m.Group([0])
    try:
        got = g.oligo_stats(pool, m.Chem.primer3(**kw))
        with pytest.raises(m.MsspeError) as e:
            g.oligo_stats(pool, m.Chem.primer3(dv=-1.0))
        assert e.value.code == 1
    finally:
        g.close()
    assert_stats(got, oracle.check_primers(oracle_tables, pool, oracle.p3_args(**kw)), name)


def test_negative_salts_are_refused(eng, m, oracle, oracle_tables):
    """oligotm returns OLIGOTM_ERROR for a negative divalent or dNTP concentration (the dNTP one only when dv != 0,
    as it zeroes dNTP first); the engine refuses those and a negative monovalent one rather than give a finite Tm.
    The cross-dimer screen keeps thal's own rule, which clamps."""
    import torch
    pool = stage_b_pool(13, 5)
    for kw in (dict(dv=-1.0), dict(dntp=-0.1), dict(dv=-0.5, dntp=-0.5), dict(mv=-1.0), dict(mv=-1.0, dv=0.0)):
        with pytest.raises(m.MsspeError) as e:
            eng.oligo_stats(pool, m.Chem.primer3(**kw))
        assert e.value.code == 1, kw
        d_pool = torch.zeros(len(pool), dtype=torch.int64, device="cuda")
        d_out = torch.zeros(len(pool), dtype=torch.float64, device="cuda")
        with pytest.raises(m.MsspeError):
            eng.oligo_stats_dev(d_pool.data_ptr(), len(pool), 13, m.Chem.primer3(**kw), d_tm=d_out.data_ptr())
    got = eng.oligo_stats(pool, m.Chem.primer3(dv=0.0, dntp=-0.5))
    assert_stats(got, oracle.check_primers(oracle_tables, pool, oracle.p3_args(dv=0.0, dntp=-0.5)), "dv 0, dntp < 0")
    out = eng.cross_dimer(pool[:16], m.Chem.ntthal(dv=-1.0), -9000.0, want_dg=True)
    _, dg, _, _ = oracle.pool_pairs(oracle_tables, pool[:16], oracle.ntthal_args(dv=-1.0), -9000.0)
    np.testing.assert_array_equal(out["dg"], dg)


def test_primer3_shim_reads_the_chemistry_of_each_record(oracle, oracle_tables):
    """primer3_core-hip: a record's PRIMER_SALT_MONOVALENT / _DIVALENT / PRIMER_DNTP_CONC / PRIMER_DNA_CONC hold for
    that record only; a record without them is at Primer3's defaults.  Every printed value equals the oracle's at the
    record's chemistry, printed the same way; a negative salt is a PRIMER_ERROR line for its record alone."""
    primer = "GGGGCCCTTTTGGGCCCCAA"
    tags = [dict(PRIMER_SALT_MONOVALENT="120", PRIMER_SALT_DIVALENT="2.5", PRIMER_DNTP_CONC="0.8",
                 PRIMER_DNA_CONC="300"),
            {},
            dict(PRIMER_DNA_CONC="900"),
            dict(PRIMER_SALT_DIVALENT="-1"),
            {}]
    chems = [oracle.p3_args(mv=120.0, dv=2.5, dntp=0.8, dna_conc=300.0), oracle.p3_args(),
             oracle.p3_args(dna_conc=900.0), None, oracle.p3_args()]
    text = "".join(f"SEQUENCE_ID=r{q}\nSEQUENCE_PRIMER={primer}\nPRIMER_TASK=check_primers\n"
                   + "".join(f"{a}={b}\n" for a, b in t.items()) + "=\n" for q, t in enumerate(tags))
    res = subprocess.run([str(BIN / "primer3_core-hip")], input=text, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    records = res.stdout.split("\n=\n")
    assert records[-1].strip() == "" and len(records) == len(tags) + 1
    printed = set()
    for q, (rec, a) in enumerate(zip(records, chems)):
        kv = dict(line.split("=", 1) for line in rec.splitlines())
        assert kv["SEQUENCE_ID"] == f"r{q}"
        if a is None:
            assert "PRIMER_ERROR" in kv and "PRIMER_LEFT_0_TM" not in kv
            continue
        assert "PRIMER_ERROR" not in kv
        ref = oracle.check_primers(oracle_tables, [primer], a)[0]
        want = ("%.3f" % ref["tm"], "%.3f" % ref["gc"], "%.2f" % ref["self_any_th"], "%.2f" % ref["self_end_th"],
                "%.2f" % ref["hairpin_th"])
        got = tuple(kv["PRIMER_LEFT_0_" + t] for t in ("TM", "GC_PERCENT", "SELF_ANY_TH", "SELF_END_TH",
                                                       "HAIRPIN_TH"))
        assert got == want, q
        printed.add(got)
    assert len(printed) == 3            # the three chemistries print three different records
