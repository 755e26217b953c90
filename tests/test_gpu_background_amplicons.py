"""msspe_background_amplicons* on the device against the model (tests/background_amplicon_model.py: the scored-site
model's stable records paired by brute force): counts, total and the sorted list, exactly; planted facing pairs in both
modes and chemistries on both routing branches, every site stable, record boundaries, a dense tandem repeat, the
plumbing options, the caller's capacity, a 2^24-column stream, argument errors and the CLI's amplicon block."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import background_amplicon_model as bam
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


def near_copy(rng, p, max_subs, keep_3p):
    w = list(p)
    for q in rng.choice(len(p) - keep_3p, int(rng.integers(0, max_subs + 1)), replace=False):
        w[q] = "ACGT"[int(rng.integers(0, 4))]
    return "".join(w)


def plant(rng, records, primers, copies, max_subs, keep_3p):
    """The idiom of tests/test_gpu_background_thal.py: `copies` near-copies of every primer, every other one as its
    reverse complement, at random places."""
    recs = [list(r) for r in records]
    k = len(primers[0])
    for i, p in enumerate(primers):
        for c in range(copies):
            w = near_copy(rng, p, max_subs, keep_3p)
            if (i + c) % 2:
                w = bm.revcomp(w)
            r = recs[int(rng.integers(0, len(recs)))]
            a = int(rng.integers(0, len(r) - k + 1))
            r[a:a + k] = w
    return ["".join(r) for r in recs]


def plant_pairs(rng, records, primers, pairs, lengths, max_subs, keep_3p):
    """`pairs` facing pairs: a near-copy of one primer (a plus-strand site) and, `length - k` columns on, the reverse
    complement of a near-copy of another (a minus-strand site), in slots of their own so that none overwrites another."""
    recs = [list(r) for r in records]
    k = len(primers[0])
    slot = max(lengths) + 8
    free = [(ri, a) for ri, r in enumerate(recs) for a in range(0, len(r) - slot, slot)]
    for c, at in enumerate(rng.choice(len(free), pairs, replace=False)):
        ri, a = free[int(at)]
        f, v = primers[int(rng.integers(0, len(primers)))], primers[int(rng.integers(0, len(primers)))]
        length = lengths[c % len(lengths)]
        subs = max_subs if c % 2 else 0                     # every other pair exact: stable at any sensible threshold
        recs[ri][a:a + k] = near_copy(rng, f, subs, keep_3p)
        recs[ri][a + length - k:a + length] = bm.revcomp(near_copy(rng, v, subs, keep_3p))
    return ["".join(r) for r in recs]


def restable(scored, n, thr):
    """The scored model's answer at another threshold from the same oracle doubles."""
    counts, _stable, recs = scored
    recs = recs.copy()
    recs["stable"] = [btm.is_stable(float(t), thr) for t in recs["t"]]
    return counts, btm.stable_counts(n, recs), recs


def check_against_model(eng, records, primers, M, E, chem, mode, thr, lo, hi, want):
    """One host call with the list against the model's (counts, stable, amplicon counts, total, list)."""
    w_counts, w_stable, w_amp, w_total, w_list = want
    counts, stable, amp, total, starts, lst = eng.background_amplicons(records, primers, M, E, chem, thr, mode, lo, hi,
                                                                       capacity=w_total + 16)
    print(f"{mode} thr {thr} len {lo}..{hi}: {int(w_counts.sum())} sites, {int(w_stable.sum())} stable, "
          f"{w_total} amplicons (device {total})")
    np.testing.assert_array_equal(counts, w_counts)
    np.testing.assert_array_equal(stable, w_stable)
    np.testing.assert_array_equal(amp, w_amp)
    assert total == w_total == len(lst)
    np.testing.assert_array_equal(lst, w_list)
    np.testing.assert_array_equal(starts, bm.record_starts(records)[0])
    t_counts, t_stable, _starts = eng.background_thal(records, primers, M, E, chem, thr, mode)
    np.testing.assert_array_equal(counts, t_counts)
    np.testing.assert_array_equal(stable, t_stable)
    assert eng.info("amplicon_keys") == int(w_stable.sum())
    return counts, stable, amp, total, lst


def unscored(records, primers, M, E, lo, hi):
    """The model with every site of the string rule stable (tm_threshold <= 0): no thal needed."""
    counts, sites = bm.sites(records, primers, M, E)
    amp, total, lst = bam.pair_sites(len(primers), len(primers[0]), sites, records, lo, hi)
    return counts, counts, amp, total, lst


# ---- planted facing pairs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chem_name", ["ntthal", "primer3"])
@pytest.mark.parametrize("mode", ["any", "end1"])
@pytest.mark.parametrize("k", [13, 20])
def test_planted_pairs(m, eng, oracle, oracle_tables, k, mode, chem_name):
    rng = np.random.default_rng(1000 + k)
    M, E = 2, 2
    primers = [random_seq(rng, k) for _ in range(24)]
    records = plant(rng, [random_seq(rng, 30000), random_seq(rng, 20011)], primers, 8, M, E)
    records = plant_pairs(rng, records, primers, 60, [60, 61, 120, 299, 300, 301, 59], M, E)
    chem, args = chems(m, oracle)[chem_name]
    scored = btm.scored_sites(oracle_tables, records, primers, M, E, mode, 30.0, args)
    n = len(primers)
    # a threshold from the oracle's own doubles with sites on both sides: the median t_site as its "%.2f" float32
    mid = float(np.float32(oracle.round_fixed_f32(float(np.median(np.maximum(scored[2]["t"], 0.0))), 2)))
    for thr in (30.0, mid):
        s = restable(scored, n, thr)
        amp, total, lst = bam.amplicons_of(n, k, s[2], records, 60, 300)
        check_against_model(eng, records, primers, M, E, chem, mode, thr, 60, 300, (s[0], s[1], amp, total, lst))
        assert total >= 12        # the exact planted pairs of lengths 60, 61, 120, 299, 300 at the least
        assert set(lst["len"].tolist()) >= {60, 300} and lst["len"].min() >= 60 and lst["len"].max() <= 300
    assert 0 < s[1].sum() < s[0].sum()     # at the median some planted sites are unstable


# ---- every site stable ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.0, -5.0])
def test_threshold_zero_pairs_the_site_list(m, eng, thr):
    rng = np.random.default_rng(7)
    pal = "ACGTACAGTACGT"      # its reverse complement differs in the middle base only: a site on both strands
    primers = [random_seq(rng, 13) for _ in range(16)] + [pal, pal]
    records = plant(rng, [random_seq(rng, 60000), random_seq(rng, 5000)], primers, 10, 3, 1)
    records[1] = pal + records[1] + pal
    chem = m.Chem.ntthal()
    want = unscored(records, primers, 3, 1, 13, 500)
    *_rest, lst = check_against_model(eng, records, primers, 3, 1, chem, "any", thr, 13, 500, want)
    assert want[3] >= 100 and (lst["len"] == 13).any() and (lst["fwd"] == lst["rev"]).any()
    # the same pairing from the device's own site list
    _counts, _starts, sites = eng.background_sites(records, primers, 3, 1, capacity=int(want[0].sum()) + 16)
    amp, total, lst2 = bam.pair_sites(len(primers), 13, sites, records, 13, 500)
    np.testing.assert_array_equal(lst2, lst)
    np.testing.assert_array_equal(amp, want[2])


# ---- record boundaries ----------------------------------------------------------------------------------------------
def test_record_boundaries(m, eng):
    rng = np.random.default_rng(11)
    k, chem = 13, m.Chem.ntthal()
    f, v = random_seq(rng, k), random_seq(rng, k)
    primers = [f, v]
    rv, rf = bm.revcomp(v), bm.revcomp(f)
    body = lambda n: random_seq(rng, n)
    records = [
        f + body(74) + rv,                      # first and last window of a record: len 100
        f + body(30),                           # a plus site whose partner ...
        rv + body(20),                          # ... lies in the next record: none
        "",
        body(10) + f + "N" * 7 + "R" + body(5) + rv,   # invalid columns between the two: one amplicon
        "", "",
        rv + body(40) + f,                      # facing away from each other: none
        f, rv,                                  # records of exactly k columns, a separator between them: none
        v + body(3) + rf,                       # the other way round: primer 1 forward, primer 0 reverse
    ] + [f + body(int(rng.integers(0, 9))) + rv for _ in range(300)] + [""]     # many short records
    want = unscored(records, primers, 0, 0, k, 150)
    *_rest, lst = check_against_model(eng, records, primers, 0, 0, chem, "any", 0.0, k, 150, want)
    starts = bm.record_starts(records)[0]
    pos = {(int(a["pos"]), int(a["len"])) for a in lst}
    assert (0, 100) in pos and (int(starts[4]) + 10, 10 + k + 13 + k - 10) in pos
    assert not any(int(starts[1]) <= p < int(starts[4]) for p, _l in pos)       # nothing out of records 1 .. 3
    assert not any(int(starts[7]) <= p < int(starts[10]) for p, _l in pos)      # ... or 7 .. 9
    assert want[3] >= 302
    # the same stream as ONE record (record_start NULL): the separators are invalid columns and break nothing
    d, total_len, d_starts = eng.put_stream_packed(records)
    try:
        np.testing.assert_array_equal(d_starts, starts)
        c, s, amp, total = eng.background_amplicons_packed(d, total_len, primers, 0, 0, chem, 0.0, "any", k, 150,
                                                           record_start=d_starts)
        np.testing.assert_array_equal(amp, want[2])
        assert total == want[3]
        c1, s1, amp1, total1 = eng.background_amplicons_packed(d, total_len, primers, 0, 0, chem, 0.0, "any", k, 150)
    finally:
        eng.device_free(d)
    one = ["-".join(records)]
    w1 = unscored(one, primers, 0, 0, k, 150)
    np.testing.assert_array_equal(amp1, w1[2])
    assert total1 == w1[3] > want[3]
    check_against_model(eng, one, primers, 0, 0, chem, "any", 0.0, k, 150, w1)


# ---- a dense region -------------------------------------------------------------------------------------------------
def test_tandem_repeat(m, eng):
    rng = np.random.default_rng(13)
    p = "GATTACAGATTCC"
    unit = p + bm.revcomp(p) + "TT"
    copies = 3000
    records = [random_seq(rng, 777) + unit * copies + random_seq(rng, 500), unit * 40]
    primers = [p, random_seq(rng, 13)]
    assert len(unit) == 28
    # 900 units on: a tile of 256 sorted keys (two per unit) and its window of 1800 keys span three staged chunks of
    # 1024 keys, so partners are found in the second and third chunk as well; 300 units on: one chunk
    for units in (900, 300):
        lo, hi = 13, len(unit) * units
        want = unscored(records, primers, 0, 0, lo, hi)
        assert want[0][0].tolist() == [copies + 40, copies + 40]
        # every plus site but the last ones pairs with `units` minus sites
        assert want[3] > units * (copies - units) and want[2][0, 0] == want[2][0, 1] == want[3]
        check_against_model(eng, records, primers, 0, 0, m.Chem.ntthal(), "any", 0.0, lo, hi, want)


# ---- independence from the plumbing ---------------------------------------------------------------------------------
def test_plumbing_options_change_nothing(m, eng, oracle, oracle_tables):
    rng = np.random.default_rng(17)
    primers = [random_seq(rng, 13) for _ in range(24)]
    records = plant(rng, [random_seq(rng, 200000) for _ in range(3)], primers, 6, 3, 2)
    records = plant_pairs(rng, records, primers, 80, [80, 200, 400], 2, 2)
    chem, args = chems(m, oracle)["ntthal"]
    M, E, thr = 4, 0, 20.0
    want = bam.amplicons(oracle_tables, records, primers, M, E, "any", thr, 40, 400, args)
    assert want[0].sum() > 5 * 4096 and want[1].sum() > 2048 and want[3] >= 40
    check_against_model(eng, records, primers, M, E, chem, "any", thr, 40, 400, want)
    assert eng.info("amplicon_keys_cap_log2") == 20 and eng.info("amplicon_key_grows") == 0
    for options in ({"site_list_cap_log2": 12}, {"amplicon_keys_cap_log2": 10}, {"force_generic": 1},
                    {"site_list_cap_log2": 12, "amplicon_keys_cap_log2": 10}):
        e = m.Engine(0)
        try:
            for key, value in options.items():
                e.set_option(key, value)
            check_against_model(e, records, primers, M, E, chem, "any", thr, 40, 400, want)
            if "site_list_cap_log2" in options:
                assert e.info("background_thal_slabs") > 5 and e.info("background_thal_redone") >= 1
            if "amplicon_keys_cap_log2" in options:
                assert e.info("amplicon_key_grows") > 0
            # a second call on the same engine keeps the grown buffer and answers the same
            check_against_model(e, records, primers, M, E, chem, "any", thr, 40, 400, want)
            assert e.info("amplicon_key_grows") == 0
        finally:
            e.close()
    for bad in (9, 29):
        with pytest.raises(m.MsspeError):
            eng.set_option("amplicon_keys_cap_log2", bad)


# ---- the caller's capacity ------------------------------------------------------------------------------------------
def test_callers_capacity(m, eng):
    import torch
    rng = np.random.default_rng(19)
    primers = [random_seq(rng, 13) for _ in range(12)]
    records = plant_pairs(rng, [random_seq(rng, 50000)], primers, 200, [50, 90, 140], 0, 0)
    chem = m.Chem.ntthal()
    want = unscored(records, primers, 1, 2, 13, 200)
    n_amp, cap = want[3], want[3] // 3
    assert n_amp >= 200
    every = {tuple(r) for r in want[4].tolist()}
    with pytest.raises(m.MsspeError) as e:
        eng.background_amplicons(records, primers, 1, 2, chem, 0.0, "any", 13, 200, capacity=cap)
    assert e.value.code == 5 and e.value.count == n_amp == e.value.total and len(e.value.list) == cap
    np.testing.assert_array_equal(e.value.counts, want[0])
    np.testing.assert_array_equal(e.value.stable, want[1])
    np.testing.assert_array_equal(e.value.amplicons, want[2])
    kept = {tuple(r) for r in e.value.list.tolist()}
    assert len(kept) == cap and kept <= every
    *_rest, lst = eng.background_amplicons(records, primers, 1, 2, chem, 0.0, "any", 13, 200, capacity=e.value.count)
    np.testing.assert_array_equal(lst, want[4])                                  # the retry with count_out
    counts_only = eng.background_amplicons(records, primers, 1, 2, chem, 0.0, "any", 13, 200)      # no list
    assert len(counts_only) == 5 and counts_only[3] == n_amp
    np.testing.assert_array_equal(counts_only[2], want[2])
    d, total_len, starts = eng.put_stream_packed(records)
    try:
        guard = 64
        buf = torch.full(((cap + guard) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        _c, _s, amp, total = eng.background_amplicons_packed(d, total_len, primers, 1, 2, chem, 0.0, "any", 13, 200,
                                                             record_start=starts, d_amplicons=buf.data_ptr(),
                                                             capacity=cap, d_count=d_count.data_ptr())
        raw = buf.cpu().numpy()
        assert int(d_count.item()) == n_amp == total and (raw[cap * 16:] == 0xA5).all()
        kept = {tuple(r) for r in raw[:cap * 16].view(bam.AMPLICON_DTYPE).tolist()}
        assert len(kept) == cap and kept <= every
        np.testing.assert_array_equal(amp, want[2])
    finally:
        eng.device_free(d)


# ---- a larger stream ------------------------------------------------------------------------------------------------
def test_larger_stream(m, eng, oracle, oracle_tables):
    rng = np.random.default_rng(2424)
    primers = [random_seq(rng, 13) for _ in range(64)]
    records = [random_seq(rng, (1 << 23) + 5), random_seq(rng, (1 << 23) - 40000), random_seq(rng, 50000)]
    assert sum(map(len, records)) >= 1 << 24
    records = plant_pairs(rng, records, primers, 120, [100, 333, 1000], 2, 3)
    chem, args = chems(m, oracle)["ntthal"]
    want = bam.amplicons(oracle_tables, records, primers, 2, 3, "any", 25.0, 50, 1000, args)
    assert 5000 < want[0].sum() and 0 < want[1].sum() < want[0].sum() and want[3] >= 60
    check_against_model(eng, records, primers, 2, 3, chem, "any", 25.0, 50, 1000, want)


# ---- argument errors ------------------------------------------------------------------------------------------------
def test_argument_errors(m, eng):
    import ctypes as C
    from msspe_amd.capi import AmpliconOpt, MismatchOpt
    records, chem, primers = ["ACGTACGTACGTACGTACGTACGT"], m.Chem.ntthal(), ["ACGTACGTACGTA"]
    for lo, hi in ((12, 100), (0, 100), (101, 100)):                              # min_len < k, min_len > max_len
        with pytest.raises(m.MsspeError) as e:
            eng.background_amplicons(records, primers, 1, 1, chem, 30.0, "any", lo, hi)
        assert e.value.code == 1
    # the scored call's errors
    for bad_m, bad_e in ((14, 0), (0, 14)):
        with pytest.raises(m.MsspeError) as e:
            eng.background_amplicons(records, primers, bad_m, bad_e, chem, 30.0, "any", 13, 100)
        assert e.value.code == 1
    for k in (1, 32):
        with pytest.raises(m.MsspeError) as e:
            eng.background_amplicons(records, np.zeros(1, dtype=np.uint64), 0, 0, chem, 30.0, "any", 40, 100, k=k)
        assert e.value.code == 2
    with pytest.raises(m.MsspeError) as e:
        eng.background_amplicons(records, primers, 1, 1, chem, 30.0, 3, 13, 100)
    assert e.value.code == 1
    mm, opt = MismatchOpt(1, 1), AmpliconOpt(13, 100)
    out, words, count, total = (C.c_uint64 * 2)(), (C.c_uint64 * 1)(0), C.c_uint64(), C.c_uint64()
    L = eng.L
    assert L.msspe_background_amplicons(eng.ptr, None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1, 30.0, None,
                                        out, out, out, C.byref(total), None, 0, C.byref(count), None) == 1    # amp
    assert L.msspe_background_amplicons(eng.ptr, None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1, 30.0,
                                        C.byref(opt), out, out, None, C.byref(total), None, 0, C.byref(count),
                                        None) == 1                                                  # amplicons_out
    d, total_len, _starts = eng.put_stream_packed(["ACGTACGTACGTACGTACGT", "ACGTACGTACGTACGT"])
    try:
        for bad in ([0, 21, 21], [5, 3], [1, 21], [0, total_len + 1]):    # not ascending / not from 0 / beyond the stream
            with pytest.raises(m.MsspeError) as e:
                eng.background_amplicons_packed(d, total_len, primers, 1, 1, chem, 30.0, "any", 13, 100,
                                                record_start=np.array(bad, dtype=np.uint64))
            assert e.value.code == 1
        for lo, hi in ((12, 100), (101, 100)):
            with pytest.raises(m.MsspeError) as e:
                eng.background_amplicons_packed(d, total_len, primers, 1, 1, chem, 30.0, "any", lo, hi)
            assert e.value.code == 1
        eng.background_amplicons_packed(d, total_len, primers, 1, 1, chem, 30.0, "any", 13, 100,
                                        record_start=np.array([0, total_len], dtype=np.uint64))   # an empty last record
    finally:
        eng.device_free(d)
    # n == 0, and a stream shorter than k: MSSPE_OK with zeroed outputs
    counts, stable, amp, total, _starts, lst = eng.background_amplicons(records, [], 1, 1, chem, 30.0, "any", 13, 100,
                                                                        k=13, capacity=4)
    assert counts.shape == stable.shape == amp.shape == (0, 2) and total == 0 and len(lst) == 0
    counts, stable, amp, total, _starts, lst = eng.background_amplicons(["ACGTACGTACGT"], primers, 1, 1, chem, 30.0,
                                                                        "any", 13, 100, capacity=4)
    assert counts.sum() == stable.sum() == amp.sum() == total == 0 and len(lst) == 0


# ---- the CLI --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_inputs(m, tmp_path_factory):
    rng = np.random.default_rng(2026)
    g = np.concatenate([m.synth.aligned_genomes(30, 9000, seed=600 + j) for j in range(2)])
    d = tmp_path_factory.mktemp("bg_amplicon_cli")
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


def test_cli_block(cli_inputs, tmp_path, oracle, oracle_tables):
    fa, bg, records = cli_inputs
    scored_flags = ("--background", str(bg), "--background-tm", "30")
    base_out, base_csv = run_cli(fa, tmp_path / "a.csv", *scored_flags)
    names, words = csv_primers(base_csv)
    args = oracle.ntthal_args(mv=50.0, dv=3.0, dntp=0.0, dna_conc=250.0, temp_c=25.0)   # the screen's chemistry
    scored = btm.scored_sites(oracle_tables, records, words, 2, 3, "any", 30.0, args)
    assert base_out.endswith(btm.render(names, scored[0], scored[1], 2, 3, "any", 30.0))
    for lo, flags in ((13, ()), (200, ("--background-amplicon-min", "200"))):
        out, csv = run_cli(fa, tmp_path / "b.csv", *scored_flags, "--background-amplicon-max", "1500", *flags)
        # report only: without the block the run is the run without the new options, byte for byte
        assert csv == base_csv and out.startswith(base_out)
        amp, total, lst = bam.amplicons_of(len(words), 13, scored[2], records, lo, 1500)
        assert out[len(base_out):] == bam.render(names, ["b0", "b1"], records, amp, lst, lo, 1500)
        print(out[len(base_out):])
        assert total > 20
    for flags, why in ((("--background-amplicon-max", "500"), "'--background-amplicon-max' needs '--background <FASTA>'"),
                       (("--background", str(bg), "--background-amplicon-max", "500"),
                        "'--background-amplicon-max' needs '--background-tm <C>'"),
                       (("--background", str(bg), "--background-amplicon-min", "50"),
                        "'--background-amplicon-min' needs '--background-tm <C>'"),
                       ((*scored_flags, "--background-amplicon-min", "50"),
                        "'--background-amplicon-min' needs '--background-amplicon-max <LEN>'"),
                       ((*scored_flags, "--background-amplicon-max", "500", "--background-amplicon-min", "12"),
                        "is smaller than '--kmer-size 13'"),
                       ((*scored_flags, "--background-amplicon-max", "500", "--background-amplicon-min", "501"),
                        "is larger than '--background-amplicon-max 500'")):
        r = subprocess.run([str(CLI), "-i", str(fa), "-o", str(tmp_path / "x.csv"), *flags],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and why in r.stderr, r.stderr
