"""The model of msspe_background_thal* (tests/background_thal_model.py) against first principles, the C ABI's new
symbols and the CLI's two new flags; no GPU."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import background_model as bm
import background_thal_model as btm

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def host():
    p = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
    if not p.exists():
        pytest.fail(f"{p} is missing: run open-msspe-design_amd/build.sh")
    return C.CDLL(str(p))


def random_seq(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def small_case(seed=3, k=9):
    rng = np.random.default_rng(seed)
    records = [random_seq(rng, 700), "ACGTN" + random_seq(rng, 300), "", random_seq(rng, k)]
    primers = [records[0][50:50 + k], bm.revcomp(records[0][300:300 + k]), random_seq(rng, k), records[3]]
    return records, primers


def test_template_oligo_against_a_string_rule():
    records, primers = small_case()
    k = len(primers[0])
    stream = "-".join(records)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    _counts, sites = bm.naive_sites(records, primers, 2, 1)
    assert len(sites) > 8 and {0, 1} <= set(sites["strand"].tolist())
    got = btm.template_oligos(records, primers, sites)
    for r, o2 in zip(sites, got):
        w = stream[int(r["pos"]):int(r["pos"]) + k]
        want = w if r["strand"] else "".join(comp[c] for c in reversed(w))
        assert o2 == want and len(o2) == k
        # the primer's near-copy is the reverse complement of the strand it anneals to
        near = "".join(comp[c] for c in reversed(o2))
        assert sum(a != b for a, b in zip(near, primers[int(r["primer"])])) == int(r["mismatches"])


def test_an_exact_site_gives_the_reverse_complement_of_the_primer():
    records, primers = small_case()
    _counts, sites = bm.sites(records, primers, 0, 0)
    assert {0, 1} <= set(sites["strand"].tolist())
    for r, o2 in zip(sites, btm.template_oligos(records, primers, sites)):
        assert o2 == bm.revcomp(primers[int(r["primer"])])


def test_minus_sites_are_the_plus_sites_of_the_reversed_stream(oracle_tables):
    records, primers = small_case(seed=8)
    k = len(primers[0])
    flipped = [bm.revcomp(r.replace("N", "A")) for r in reversed(records)]
    straight = [r.replace("N", "A") for r in records]
    total = len("-".join(straight))
    _c, a = bm.sites(straight, primers, 3, 0)
    _c, b = bm.sites(flipped, primers, 3, 0)
    minus = a[a["strand"] == 1]
    plus = b[b["strand"] == 0]
    assert len(minus) == len(plus) > 4
    o2_minus = dict(zip(((int(r["primer"]), total - k - int(r["pos"])) for r in minus),
                        btm.template_oligos(straight, primers, minus)))
    o2_plus = dict(zip(((int(r["primer"]), int(r["pos"])) for r in plus), btm.template_oligos(flipped, primers, plus)))
    assert o2_minus == o2_plus
    for mode in ("any", "end1"):
        dg_m, t_m = btm.score(oracle_tables, primers, minus, btm.template_oligos(straight, primers, minus), mode)
        by = {(int(r["primer"]), total - k - int(r["pos"])): (g, t) for r, g, t in zip(minus, dg_m, t_m)}
        dg_p, t_p = btm.score(oracle_tables, primers, plus, btm.template_oligos(flipped, primers, plus), mode)
        for r, g, t in zip(plus, dg_p, t_p):
            assert by[(int(r["primer"]), int(r["pos"]))] == (g, t)


@pytest.mark.parametrize("thr", [30.0, 47.0, 12.345, 0.01, 0.0, -5.0, 99.99])
def test_the_stable_rule_and_its_cut(oracle, thr):
    import msspe_amd
    cut = msspe_amd.t_cut(thr)
    thr32 = float(np.float32(thr))
    rng = np.random.default_rng(5)
    probes = [cut, float(np.nextafter(cut, np.inf)), float(np.nextafter(cut, -np.inf)), 0.0, -3.0, thr32, thr32 - 0.005,
              thr32 + 0.005] + list(thr32 + rng.normal(0, 0.01, 300)) + list(rng.uniform(-90, 90, 300))
    for t in probes:
        t_site = max(0.0, float(t))
        want = not (oracle.round_fixed_f32(t_site, 2) < thr32)
        assert btm.is_stable(float(t), thr) == want
        assert (t_site > cut) == want          # what the kernels test
    if thr <= 0:
        assert btm.is_stable(0.0, thr) and btm.is_stable(-50.0, thr) and cut < 0


def test_render():
    text = btm.render(["Primer_0_F", "Primer_0_R"], [[7, 5], [0, 1]], [[2, 1], [0, 0]], 2, 3, "any", 30.0)
    assert text == ("\nBackground sites (up to 2 mismatches, last 3 bases exact; stable: thal ANY t >= 30.00 C):\n"
                    "  Primer_0_F: plus 7, minus 5, stable plus 2, minus 1\n"
                    "  Primer_0_R: plus 0, minus 1, stable plus 0, minus 0\n"
                    "  Total: 2 primers, plus 7, minus 6, stable plus 2, minus 1\n")
    assert "thal END1 t >= 47.50 C" in btm.render([], np.zeros((0, 2)), np.zeros((0, 2)), 1, 0, "end1", 47.5)


def test_symbols_dtype_and_null_context():
    import msspe_amd
    from msspe_amd import capi
    lib = msspe_amd.load_library()
    for name in ("msspe_background_thal_packed_dev", "msspe_background_thal"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    assert capi.SCORED_SITE_DTYPE.itemsize == 32 and capi.SCORED_SITE_DTYPE == btm.SCORED_SITE_DTYPE
    for method in ("background_thal", "background_thal_packed"):
        assert hasattr(capi.Engine, method)
    mm = capi.MismatchOpt(2, 3)
    chem = capi.Chem.ntthal()
    out = (C.c_uint64 * 2)()
    words = (C.c_uint64 * 1)(0)
    count = C.c_uint64()
    assert lib.msspe_background_thal_packed_dev(None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1, 30.0, out,
                                                out, None, 0, None) == 1
    assert lib.msspe_background_thal(None, None, None, 0, 13, C.byref(mm), words, 1, C.byref(chem), 1, 30.0, out, out,
                                     None, 0, C.byref(count), None) == 1


def parse(host, *a):
    argv = (C.c_char_p * (len(a) + 1))(b"od-msspe-hip", *[x.encode() for x in a])
    buf = C.create_string_buffer(1 << 16)
    rc = host.odm_parse_args(len(a) + 1, argv, buf, 1 << 16)
    out = buf.value.decode()
    return rc, (dict(l.split("=", 1) for l in out.splitlines()) if rc == 0 else out)


ENV = ["BACKGROUND", "BACKGROUND_MISMATCHES", "BACKGROUND_3P_EXACT", "MAX_BACKGROUND_SITES", "BACKGROUND_TM",
       "BACKGROUND_THAL"]


def test_cli_flags_need_a_background(host, monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for flag, value in (("--background-tm", "30"), ("--background-thal", "end1")):
        rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", flag, value)
        assert rc == 2 and f"'{flag}' needs '--background <FASTA>'" in out
    rc, kv = parse(host, "-i", "a.fa", "-o", "b.csv", "--background", "h.fa")
    assert rc == 0 and kv["background_tm"] == "" and kv["background_thal"] == "any"
    rc, kv = parse(host, "-i", "a.fa", "-o", "b.csv", "--background", "h.fa", "--background-tm", "30.5",
                   "--background-thal", "end1")
    assert rc == 0 and kv["background_tm"] == "30.5" and kv["background_thal"] == "end1"
    monkeypatch.setenv("BACKGROUND", "env.fa")
    monkeypatch.setenv("BACKGROUND_TM", "25")
    monkeypatch.setenv("BACKGROUND_THAL", "end1")
    rc, kv = parse(host, "-i", "a.fa", "-o", "b.csv")
    assert rc == 0 and (kv["background_tm"], kv["background_thal"]) == ("25", "end1")
    rc, kv = parse(host, "-i", "a.fa", "-o", "b.csv", "--background-thal", "any")   # the command line wins
    assert rc == 0 and kv["background_thal"] == "any"
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--background-tm", "warm")
    assert rc == 2 and "invalid value 'warm' for '--background-tm'" in out
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--background-thal", "end2")
    assert rc == 2 and "invalid value 'end2' for '--background-thal" in out
    rc, out = parse(host, "-i", "a.fa", "-o", "b.csv", "--help")
    assert rc == 2 and "--background-tm <...>  [env: BACKGROUND_TM=]" in out
    assert "--background-thal <...>  [env: BACKGROUND_THAL=]" in out
