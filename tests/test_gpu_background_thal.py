"""msspe_background_thal* on the device against the model (tests/background_thal_model.py: the site model plus the CPU
oracle's thal): dg and t of every site bit for bit, the stable counts, both modes and chemistries, oligo lengths on
both routing branches, odd primers and records, the routes, the work-list split, the caller's capacity, a 2^24-column
stream, isolation from the END and ANY screens' cuts, argument errors and the CLI's --background-tm block."""
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import background_model as bm
import background_thal_model as btm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "open-msspe-design_amd" / "od-msspe-hip"


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


def random_seq(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def chems(m, oracle):
    return {"ntthal": (m.Chem.ntthal(), oracle.ntthal_args()), "primer3": (m.Chem.primer3(), oracle.p3_args())}


def plant(rng, records, primers, copies, max_subs, keep_3p):
    """Writes `copies` near-copies of every primer (0 .. max_subs substitutions outside its last keep_3p bases, every
    other one as its reverse complement) into the records at random places."""
    recs = [list(r) for r in records]
    k = len(primers[0])
    for i, p in enumerate(primers):
        for c in range(copies):
            w = list(p)
            for q in rng.choice(k - keep_3p, int(rng.integers(0, max_subs + 1)), replace=False):
                w[q] = "ACGT"[int(rng.integers(0, 4))]
            w = "".join(w)
            if (i + c) % 2:
                w = bm.revcomp(w)
            r = recs[int(rng.integers(0, len(recs)))]
            a = int(rng.integers(0, len(r) - k + 1))
            r[a:a + k] = w
    return ["".join(r) for r in recs]


def check_against_model(eng, tables, records, primers, M, E, chem, args, mode, thr, want=None):
    """One host call with the list against the model; returns the model's (counts, stable, records)."""
    if want is None:
        want = btm.scored_sites(tables, records, primers, M, E, mode, thr, args)
    w_counts, w_stable, w_recs = want
    counts, stable, starts, recs = eng.background_thal(records, primers, M, E, chem, thr, mode,
                                                       capacity=len(w_recs) + 16)
    np.testing.assert_array_equal(counts, w_counts)
    for f in ("primer", "pos", "mismatches", "strand"):
        np.testing.assert_array_equal(recs[f], w_recs[f])
    np.testing.assert_array_equal(recs["dg"], w_recs["dg"])      # doubles, bit for bit (inf == inf)
    np.testing.assert_array_equal(recs["t"], w_recs["t"])
    np.testing.assert_array_equal(recs["stable"], w_recs["stable"])
    np.testing.assert_array_equal(stable, w_stable)
    np.testing.assert_array_equal(starts, bm.record_starts(records)[0])
    return want


def restable(want, n, thr):
    """The model's answer at another threshold from the same oracle doubles."""
    counts, _stable, recs = want
    recs = recs.copy()
    recs["stable"] = [btm.is_stable(float(t), thr) for t in recs["t"]]
    return counts, btm.stable_counts(n, recs), recs


# ---- the probe ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    rng = np.random.default_rng(5)
    primers = [random_seq(rng, 13) for _ in range(24)]
    records = [random_seq(rng, 200000) for _ in range(3)]
    recs = [list(r) for r in records]
    for j in range(24):   # 12 one-mismatch copies and 12 exact copies, every other one on the minus strand
        w = list(primers[j])
        if j < 12:
            q = int(rng.integers(0, 11))
            w[q] = "ACGT"[("ACGT".index(w[q]) + 1 + int(rng.integers(0, 3))) % 4]
        w = "".join(w)
        if j % 2:
            w = bm.revcomp(w)
        r = recs[j % 3]
        a = 1000 + 7919 * j
        r[a:a + 13] = w
    return ["".join(r) for r in recs], primers


@pytest.mark.parametrize("chem_name", ["ntthal", "primer3"])
@pytest.mark.parametrize("mode", ["any", "end1"])
def test_probe_every_site_bit_equal(m, eng, oracle, oracle_tables, probe, mode, chem_name):
    records, primers = probe
    chem, args = chems(m, oracle)[chem_name]
    want = check_against_model(eng, oracle_tables, records, primers, 3, 2, chem, args, mode, 30.0)
    counts, _stable, recs = want
    n = len(primers)
    by_mm = [int((recs["mismatches"] == q).sum()) for q in range(4)]
    print(f"probe {mode} {chem_name}: {len(recs)} sites, by mismatches {by_mm}, t max {recs['t'].max():.2f}")
    assert len(recs) > 1500 and by_mm[0] >= 12 and by_mm[1] >= 12
    np.testing.assert_array_equal(eng.background_sites(records, primers, 3, 2)[0], counts)   # the existing call
    for thr in (10.0, 40.0):
        check_against_model(eng, oracle_tables, records, primers, 3, 2, chem, args, mode, thr,
                            want=restable(want, n, thr))
    # a site's own rounded t as the threshold: that site is stable; at the next float32 above, it is not
    pick = recs[np.argsort(recs["t"])[len(recs) * 9 // 10]]
    assert pick["t"] > 0
    own = np.float32(oracle.round_fixed_f32(float(pick["t"]), 2))
    for thr, is_stable in ((own, 1), (np.nextafter(own, np.float32(np.inf)), 0)):
        w = restable(want, n, float(thr))
        at = np.flatnonzero((w[2]["primer"] == pick["primer"]) & (w[2]["pos"] == pick["pos"]) &
                            (w[2]["strand"] == pick["strand"]))[0]
        assert w[2]["stable"][at] == is_stable
        check_against_model(eng, oracle_tables, records, primers, 3, 2, chem, args, mode, float(thr), want=w)


# ---- lengths: both routing branches (k <= 16 / above) and both word widths of the site kernel -------------------------
@pytest.mark.parametrize("mode", ["any", "end1"])
@pytest.mark.parametrize("k", [8, 13, 16, 17, 20, 24, 31])
def test_lengths(m, eng, oracle, oracle_tables, k, mode):
    rng = np.random.default_rng(100 + k)
    M, E = max(1, k // 6), min(3, k // 4)
    primers = [random_seq(rng, k) for _ in range(24)]
    records = plant(rng, [random_seq(rng, 30000), random_seq(rng, 20011)], primers, 16, M, E)
    chem, args = chems(m, oracle)["ntthal"]
    want = check_against_model(eng, oracle_tables, records, primers, M, E, chem, args, mode, 30.0)
    # long near-copies all melt far above 30 C: a second threshold from the oracle's own doubles, the median t_site
    # as its "%.2f" float32, has sites on both sides at every length
    t_site = np.maximum(want[2]["t"], 0.0)
    mid = float(np.float32(oracle.round_fixed_f32(float(np.median(t_site)), 2)))
    _c, _s, recs = check_against_model(eng, oracle_tables, records, primers, M, E, chem, args, mode, mid,
                                       want=restable(want, len(primers), mid))
    print(f"k={k} M={M} E={E} {mode}: {len(recs)} sites, {int(want[2]['stable'].sum())} stable at 30 C, "
          f"{int(recs['stable'].sum())} at {mid:.2f} C")
    assert len(recs) >= 300 and 0 < recs["stable"].sum() < len(recs)


# ---- edges ----------------------------------------------------------------------------------------------------------
def test_edges(m, eng, oracle, oracle_tables):
    rng = np.random.default_rng(77)
    pal, homo = "ACGTACGTACGT", "A" * 12
    other = random_seq(rng, 12)
    primers = [pal, homo, other, other]                                       # a duplicate primer
    body = random_seq(rng, 3000)
    records = [pal + body[:500] + "N" + other + "NN" + bm.revcomp(other)[:11] + "N" + body[500:1500] + homo,
               "", other, body[1500:] + "T" * 12 + "N" * 5 + bm.revcomp(other), ""]
    starts, _total = bm.record_starts(records)
    for (chem, args), mode in itertools.product(
            [(m.Chem.ntthal(), oracle.ntthal_args()), (m.Chem.ntthal(max_loop=5), oracle.ntthal_args(max_loop=5))],
            ["any", "end1"]):
        _c, _s, recs = check_against_model(eng, oracle_tables, records, primers, 2, 2, chem, args, mode, 20.0)
        at0 = recs[(recs["primer"] == 0) & (recs["pos"] == 0)]
        assert len(at0) == 2 and (at0["mismatches"] == 0).all()               # the palindrome: a site on both strands
        assert (at0["dg"] == at0["dg"][0]).all() and np.isfinite(at0["dg"]).all()
        a, b = recs[recs["primer"] == 2], recs[recs["primer"] == 3]
        assert len(a) >= 3
        for f in ("pos", "strand", "mismatches", "dg", "t", "stable"):
            np.testing.assert_array_equal(a[f], b[f])
        # flush with record ends: a record of exactly k columns, and the last k columns of records 0 and 3
        pos = {(int(r["primer"]), int(r["pos"])) for r in recs}
        assert (2, int(starts[2])) in pos and (1, int(starts[0]) + len(records[0]) - 12) in pos
        assert (2, int(starts[3]) + len(records[3]) - 12) in pos
    # No structure at all: a homopolymer primer against windows that hold none of its complement (every window is a
    # site at M = k, E = 0).  At its exact site the template is the full complement, a duplex like any other.
    records = ["CCGGCGCGGCCGCGCGCCGGCC" + "ACGT" * 6 + "G" * 15 + "T" * 14]
    chem, args = chems(m, oracle)["ntthal"]
    for mode in ("any", "end1"):
        for thr, all_stable in ((0.0, True), (-1.0, True), (0.01, False)):
            _c, _s, recs = check_against_model(eng, oracle_tables, records, [homo], 12, 0, chem, args, mode, thr)
            none = recs[np.isinf(recs["dg"])]
            assert len(none) >= 10 and (none["t"] == 0).all() and (none["dg"] > 0).all()
            assert recs["stable"].all() == all_stable and none["stable"].all() == all_stable
            assert np.isfinite(recs["dg"]).any()


# ---- routes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [13, 20])
def test_routes_give_the_same_bits(m, oracle, oracle_tables, probe, k):
    rng = np.random.default_rng(k)
    primers = [random_seq(rng, k) for _ in range(16)] + (["ACGTACGTACGT" + "A" * (k - 12)] if k == 13 else [])
    records = plant(rng, [random_seq(rng, 40000)], primers, 12, 2, 2)
    chem, args = chems(m, oracle)["ntthal"]
    for mode in ("any", "end1"):
        want = btm.scored_sites(oracle_tables, records, primers, 2, 2, mode, 25.0, args)
        for options in ({}, {"force_generic": 1}, {"wave_kernel": 0}, {"list_cap_log2": 20}):
            e = m.Engine(0)
            try:
                for key, value in options.items():
                    e.set_option(key, value)
                check_against_model(e, oracle_tables, records, primers, 2, 2, chem, args, mode, 25.0, want=want)
            finally:
                e.close()


# ---- the work list --------------------------------------------------------------------------------------------------
def test_work_list_split(m, eng, probe):
    records, primers = probe
    chem = m.Chem.ntthal()
    assert eng.info("site_list_cap_log2") == 22
    counts, stable, _starts, recs = eng.background_thal(records, primers, 4, 0, chem, 20.0, "any", capacity=1 << 16)
    assert len(recs) > 5 * 4096 and eng.info("background_thal_slabs") == 1 and eng.info("background_thal_redone") == 0
    small = m.Engine(0)
    try:
        small.set_option("site_list_cap_log2", 12)
        assert small.info("site_list_cap_log2") == 12
        c2, s2, _starts, r2 = small.background_thal(records, primers, 4, 0, chem, 20.0, "any", capacity=1 << 16)
        print(f"{len(recs)} sites through a work list of 4096: {small.info('background_thal_slabs')} slabs, "
              f"{small.info('background_thal_redone')} split")
        assert small.info("background_thal_slabs") > 5 and small.info("background_thal_redone") >= 1
        c3, s3, _starts = small.background_thal(records, primers, 4, 0, chem, 20.0, "any")   # counts only
        with pytest.raises(m.MsspeError):
            small.set_option("site_list_cap_log2", 11)
    finally:
        small.close()
    for c, s in ((c2, s2), (c3, s3)):
        np.testing.assert_array_equal(c, counts)
        np.testing.assert_array_equal(s, stable)
    np.testing.assert_array_equal(r2, recs)
    np.testing.assert_array_equal(eng.background_sites(records, primers, 4, 0)[0], counts)


def test_one_primer_more_sites_than_the_work_list(m):
    """One run of 2048 positions holds more sites than the work list: the slab is split by primers."""
    records = ["A" * 2000]
    primers = ["A" * 13, "T" * 13, "A" * 12 + "C", "ACGTTGCAACGTA"]
    e = m.Engine(0)
    try:
        want = e.background_thal(records, primers, 1, 0, m.Chem.ntthal(), 0.0, "any", capacity=1 << 14)
        e.set_option("site_list_cap_log2", 12)
        got = e.background_thal(records, primers, 1, 0, m.Chem.ntthal(), 0.0, "any", capacity=1 << 14)
        assert e.info("background_thal_redone") >= 1
    finally:
        e.close()
    assert want[0].sum() == 3 * 1988 > 4096
    for a, b in zip(want, got):
        np.testing.assert_array_equal(a, b)


def test_callers_capacity(m, eng, probe):
    import torch
    records, primers = probe
    chem = m.Chem.ntthal()
    counts, stable, _starts, recs = eng.background_thal(records, primers, 3, 2, chem, 30.0, "any", capacity=1 << 13)
    n_sites, cap = len(recs), len(recs) // 3
    with pytest.raises(m.MsspeError) as e:
        eng.background_thal(records, primers, 3, 2, chem, 30.0, "any", capacity=cap)
    assert e.value.code == 5 and e.value.count == n_sites and len(e.value.sites) == cap
    np.testing.assert_array_equal(e.value.counts, counts)
    np.testing.assert_array_equal(e.value.stable, stable)
    every = {tuple(r) for r in recs.tolist()}
    assert len({tuple(r) for r in e.value.sites.tolist()}) == cap and {tuple(r) for r in e.value.sites.tolist()} <= every
    d, total, _ = eng.put_stream_packed(records)
    try:
        guard = 64
        buf = torch.full(((cap + guard) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        c, s = eng.background_thal_packed(d, total, primers, 3, 2, chem, 30.0, "any", d_sites=buf.data_ptr(),
                                          capacity=cap, d_count=d_count.data_ptr())
        raw = buf.cpu().numpy()
        assert int(d_count.item()) == n_sites and (raw[cap * 32:] == 0xA5).all()
        kept = raw[:cap * 32].view(btm.SCORED_SITE_DTYPE)
        assert len({tuple(r) for r in kept.tolist()}) == cap and {tuple(r) for r in kept.tolist()} <= every
        np.testing.assert_array_equal(c, counts)
        np.testing.assert_array_equal(s, stable)
        c, s = eng.background_thal_packed(d, total, primers, 3, 2, chem, 30.0, "any")   # no list
        np.testing.assert_array_equal(c, counts)
        np.testing.assert_array_equal(s, stable)
    finally:
        eng.device_free(d)


# ---- a larger stream ------------------------------------------------------------------------------------------------
def test_larger_stream(m, eng, oracle, oracle_tables):
    rng = np.random.default_rng(2400)
    records = [random_seq(rng, (1 << 23) + 5), random_seq(rng, (1 << 23) - 40000), random_seq(rng, 50000)]
    assert sum(map(len, records)) >= 1 << 24
    primers = [random_seq(rng, 13) for _ in range(200)]
    chem, args = chems(m, oracle)["ntthal"]
    counts, stable, _starts, recs = eng.background_thal(records, primers, 2, 3, chem, 25.0, "any", capacity=1 << 17)
    d, total, _ = eng.put_stream_packed(records)
    try:
        np.testing.assert_array_equal(eng.background_sites_packed(d, total, primers, 2, 3), counts)
    finally:
        eng.device_free(d)
    assert 20000 < len(recs) == int(counts.sum()) <= 60000          # the oracle's share: a few seconds
    stream = btm.stream_text(records)
    o2 = [btm.template_oligo(stream, 13, int(r["pos"]), int(r["strand"])) for r in recs]
    dg, t = btm.score(oracle_tables, primers, recs, o2, "any", args)
    want = btm.records_of(recs, dg, t, 25.0)
    np.testing.assert_array_equal(stable, btm.stable_counts(len(primers), want))
    sample = np.random.default_rng(1).choice(len(recs), 2000, replace=False)
    for f in ("dg", "t", "stable"):
        np.testing.assert_array_equal(recs[f][sample], want[f][sample])
    np.testing.assert_array_equal(recs["dg"], want["dg"])
    np.testing.assert_array_equal(recs["t"], want["t"])
    print(f"{len(recs)} sites on 2^24 columns, {int(stable.sum())} stable at 25 C")
    assert 0 < stable.sum() < counts.sum()


# ---- isolation ------------------------------------------------------------------------------------------------------
def test_cuts_of_three_kinds_never_mix(m, probe):
    """An END screen, an ANY screen and a background-thal call at the same numeric threshold share no cut."""
    rng = np.random.default_rng(3)
    pool = [random_seq(rng, 13) for _ in range(64)]
    records, primers = probe
    records = [records[0][:60000]]
    chem, thr = m.Chem.ntthal(), 20.0

    def calls(e):
        return {"end": lambda: e.cross_dimer_end(pool, chem, thr)["bitmap"],
                "any": lambda: e.cross_dimer(pool, chem, thr, want_dg=False)["bitmap"],
                "bg_any": lambda: e.background_thal(records, primers, 3, 2, chem, thr, "any")[1],
                "bg_end": lambda: e.background_thal(records, primers, 3, 2, chem, thr, "end1")[1]}

    alone = {}
    for name in ("end", "any", "bg_any", "bg_end"):
        e = m.Engine(0)
        try:
            alone[name] = calls(e)[name]()
        finally:
            e.close()
    assert alone["bg_any"].sum() > 0 and alone["any"].any() and alone["end"].any()
    for order in itertools.permutations(("end", "any", "bg_any", "bg_end")):
        e = m.Engine(0)
        try:
            for name in order + order[:1]:
                np.testing.assert_array_equal(calls(e)[name](), alone[name], err_msg=f"{name} in {order}")
        finally:
            e.close()


# ---- argument errors ------------------------------------------------------------------------------------------------
def test_argument_errors(m, eng):
    import ctypes as C
    records, chem = ["ACGTACGTACGTACGTACGTACGT"], m.Chem.ntthal()
    for bad_m, bad_e in ((14, 0), (0, 14), (-1, 0), (0, -1)):
        with pytest.raises(m.MsspeError) as e:
            eng.background_thal(records, ["ACGTACGTACGTA"], bad_m, bad_e, chem, 30.0)
        assert e.value.code == 1
    for k in (0, 1, 32):
        with pytest.raises(m.MsspeError) as e:
            eng.background_thal(records, np.zeros(1, dtype=np.uint64), 0, 0, chem, 30.0, k=k)
        assert e.value.code == 2
    for mode in (0, 3, 4):
        with pytest.raises(m.MsspeError) as e:
            eng.background_thal(records, ["ACGTACGTACGTA"], 1, 1, chem, 30.0, mode)
        assert e.value.code == 1
    with pytest.raises(m.MsspeError) as e:
        eng.background_thal(records, np.array([1 << 26], dtype=np.uint64), 0, 0, chem, 30.0, k=13)
    assert e.value.code == 1 and "bits above" in str(e.value)
    from msspe_amd.capi import MismatchOpt
    mm, out, words, count = MismatchOpt(1, 1), (C.c_uint64 * 2)(), (C.c_uint64 * 1)(0), C.c_uint64()
    L = eng.L
    assert L.msspe_background_thal(eng.ptr, None, None, 0, 13, C.byref(mm), words, 1, None, 1, 30.0, out, out, None, 0,
                                   C.byref(count), None) == 1                                   # chem
    assert L.msspe_background_thal(eng.ptr, None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1, 30.0, out, None,
                                   None, 0, C.byref(count), None) == 1                          # stable_out
    # n == 0, and a stream shorter than k: MSSPE_OK with zeroed outputs
    counts, stable, _starts, recs = eng.background_thal(records, [], 1, 1, chem, 30.0, k=13, capacity=4)
    assert counts.shape == stable.shape == (0, 2) and len(recs) == 0
    counts, stable, _starts, recs = eng.background_thal(["ACGTACGTACGT"], ["ACGTACGTACGTA"], 1, 1, chem, 30.0, capacity=4)
    assert counts.sum() == stable.sum() == 0 and len(recs) == 0


# ---- the CLI --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_inputs(m, tmp_path_factory):
    rng = np.random.default_rng(2025)
    g = np.concatenate([m.synth.aligned_genomes(30, 9000, seed=600 + j) for j in range(2)])
    d = tmp_path_factory.mktemp("bg_thal_cli")
    fa = d / "in.fa"
    fa.write_text("".join(f">g{i} synthetic\n{bytes(r).decode()}\n" for i, r in enumerate(g)))
    t0 = bytes(g[0]).decode().replace("-", "")
    records = [random_seq(rng, 30000) + t0[:3000] + random_seq(rng, 500), bm.revcomp(t0[3000:6000]) + random_seq(rng, 12000)]
    bg = d / "background.fa"
    bg.write_text("".join(f">b{i} background\n" + "\n".join(r[a:a + 70] for a in range(0, len(r), 70)) + "\n"
                          for i, r in enumerate(records)))
    return fa, bg, records


def run_cli(fa, csv, *extra):
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(csv), "--do-align", "false", *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout, Path(csv).read_bytes()


def csv_primers(csv):
    rows = [l.split(",") for l in csv.decode().splitlines()[1:] if l]
    return [r[1] for r in rows], [r[2] for r in rows]


def cli_chem(oracle):
    # the cross-dimer screen's chemistry: od-msspe's defaults as the "{:.2}" texts ntthal is called with
    return oracle.ntthal_args(mv=50.0, dv=3.0, dntp=0.0, dna_conc=250.0, temp_c=25.0)


def test_cli_block_drop_rule_and_modes(cli_inputs, tmp_path, oracle, oracle_tables, m):
    fa, bg, records = cli_inputs
    base_out, base_csv = run_cli(fa, tmp_path / "a.csv")
    # without --background-tm: every byte is the parent's (the model of the unscored block)
    out0, csv0 = run_cli(fa, tmp_path / "b.csv", "--background", str(bg))
    names, words = csv_primers(csv0)
    assert csv0 == base_csv and out0 == base_out + bm.render(names, bm.sites(records, words, 2, 3)[0], 2, 3)
    args = cli_chem(oracle)
    for mode, flags in (("any", ()), ("any", ("--background-thal", "any")), ("end1", ("--background-thal", "end1"))):
        out, csv = run_cli(fa, tmp_path / "c.csv", "--background", str(bg), "--background-tm", "30", *flags)
        assert csv == base_csv and out.startswith(base_out)
        counts, stable, _recs = btm.scored_sites(oracle_tables, records, words, 2, 3, mode, 30.0, args)
        assert out[len(base_out):] == btm.render(names, counts, stable, 2, 3, mode, 30.0)
        assert 0 < stable.sum() < counts.sum()
    # the drop rule counts stable sites: seen without the vertex cover in the way
    quiet = ("--delta-g-threshold", "-1000000")
    _, all_csv = run_cli(fa, tmp_path / "d.csv", *quiet)
    all_names, all_words = csv_primers(all_csv)
    counts, stable, _recs = btm.scored_sites(oracle_tables, records, all_words, 2, 3, "any", 25.0, args)
    per, per_all = stable.sum(1), counts.sum(1)
    limit = int(np.sort(per)[len(per) * 3 // 4])
    assert (per > limit).any() and (per <= limit).any() and ((per <= limit) & (per_all > limit)).any()
    f_out, f_csv = run_cli(fa, tmp_path / "e.csv", *quiet, "--background", str(bg), "--background-tm", "25",
                           "--max-background-sites", str(limit))
    f_names, f_words = csv_primers(f_csv)
    assert f_words == [w for w, c in zip(all_words, per) if c <= limit]
    fc, fs, _recs = btm.scored_sites(oracle_tables, records, f_words, 2, 3, "any", 25.0, args)
    assert f_out.endswith(btm.render(f_names, fc, fs, 2, 3, "any", 25.0))
    r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(tmp_path / "x.csv"), "--background-tm", "30"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "'--background-tm' needs '--background <FASTA>'" in r.stderr
