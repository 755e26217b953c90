"""The tolerant seeded stage A's interface without a GPU: the header declares the three entry points with the _sets
siblings' arguments, the rule behind the sets and the two state outputs at the end; the library exports them; the
binding lists them and has the three Engine methods; a NULL context is an argument error; the CLI reads --seed-*
only when a round can seed and reports the usage errors; the host layer renders the seeding block as the model does."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from stage_a_tolerant_model import render_block
from test_coverage_mm_model import parse

ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
NAMES = ["msspe_kmer_candidates_tolerant", "msspe_kmer_candidates_tolerant_packed_dev",
         "msspe_kmer_candidates_both_tolerant_packed_dev"]
SIBLINGS = ["msspe_kmer_candidates_sets", "msspe_kmer_candidates_sets_packed_dev",
            "msspe_kmer_candidates_both_sets_packed_dev"]
ENV = ("SEED_MISMATCHES", "SEED_3P_EXACT", "SEED_TM", "SEED_THAL", "EXISTING_PRIMERS", "REPICK_ROUNDS", "KMER_SIZE",
       "MSSPE_DEVICES", "TUBES")


@pytest.fixture(scope="module")
def lib():
    import msspe_amd
    return msspe_amd.load_library()


@pytest.fixture(scope="module")
def host():
    import msspe_amd
    msspe_amd.load_library()
    return C.CDLL(str(HOST_LIB))


def declared_args(header, name):
    decl = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
    return [" ".join(a.split()) for a in decl.split(",")]


def test_header_library_and_binding_agree(lib):
    from msspe_amd import capi
    header = (ROOT / "include" / "msspe_hip.h").read_text()
    for name, sibling in zip(NAMES, SIBLINGS):
        assert hasattr(lib, name) and name in capi.EXPORTS, name
        args, sib = declared_args(header, name), declared_args(header, sibling)
        both = "both" in name
        at = 7                                      # behind the sets (one list, or one per direction)
        assert args[:at] == sib[:at] and args[at] == "const msspe_seed_rule *rule", name
        assert args[at + 1:len(sib) + 1] == sib[at:], name
        tail = args[len(sib) + 1:]
        assert tail == (["uint8_t *seed_covered_fwd", "uint32_t *seed_partitions_fwd", "uint8_t *seed_covered_rev",
                         "uint32_t *seed_partitions_rev"] if both else
                        ["uint8_t *seed_covered_out", "uint32_t *seed_partitions_out"]), name
        assert len(getattr(lib, name).argtypes) == len(args) == (19 if both else 14), name
    for field in ("int max_mismatches, exact_3p;", "int mode;", "const msspe_chem *chem;", "float tm_threshold;"):
        assert field in header
    assert "} msspe_seed_rule;" in header
    for key in ("tiles", "segments", "incidence_us", "seed_us"):
        assert f'"stage_a_tolerant_{key}"' in header, key
    assert [f[0] for f in capi.SeedRule._fields_] == ["max_mismatches", "exact_3p", "mode", "chem", "tm_threshold"]


def test_binding_has_the_three_methods():
    from msspe_amd import Engine, seed_rule, Chem
    for name in ("kmer_candidates_tolerant", "kmer_candidates_tolerant_packed", "kmer_candidates_tolerant_both_packed"):
        params = list(inspect.signature(getattr(Engine, name)).parameters)
        assert "rule" in params and "capacity" in params, name
    assert list(inspect.signature(Engine.kmer_candidates_tolerant).parameters)[:6] == [
        "self", "seqs", "opt", "direction", "seed", "rule"]
    assert list(inspect.signature(Engine.kmer_candidates_tolerant_packed).parameters)[:8] == [
        "self", "d_packed", "n_seq", "seq_len", "opt", "direction", "seed", "rule"]
    # existing signatures are untouched
    assert list(inspect.signature(Engine.kmer_candidates_packed).parameters) == [
        "self", "d_packed", "n_seq", "seq_len", "opt", "direction", "capacity", "seed", "exclude"]
    r = seed_rule(2, 3, "end1", Chem.ntthal(), 30.0)
    assert (r.max_mismatches, r.exact_3p, r.mode, r.tm_threshold) == (2, 3, 2, 30.0) and r.chem.contents.mv == 50.0
    assert seed_rule(1, 0).mode == 0 and not seed_rule(1, 0).chem


def test_null_context_is_an_argument_error(lib):
    from msspe_amd import KmerOpt, capi, seed_rule
    g = np.full((2, 600), ord("A"), dtype=np.uint8)
    w, f = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint32)
    n = C.c_int(-1)
    opt, sets, rule = KmerOpt(500, 250, 50, 13, 4, 1), capi.KmerSets(None, 0, None, 0), seed_rule(1, 3)
    for name in NAMES[:2]:
        assert getattr(lib, name)(None, g.ctypes.data, 2, 600, C.byref(opt), 0, C.byref(sets), C.byref(rule),
                                  w.ctypes.data, f.ctypes.data, 4, C.byref(n), None, None) == 1, name
    assert lib.msspe_kmer_candidates_both_tolerant_packed_dev(
        None, g.ctypes.data, 2, 600, C.byref(opt), C.byref(sets), C.byref(sets), C.byref(rule), w.ctypes.data,
        f.ctypes.data, C.byref(n), w.ctypes.data, f.ctypes.data, C.byref(n), 4, None, None, None, None) == 1


def kv(out):
    return dict(l.split("=", 1) for l in out.splitlines())


def test_cli_flags(host, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    base = ("-i", "a", "-o", "b")
    got = kv(parse(host, *base)[1])
    assert (got["seed_mismatches"], got["seed_tm"], got["seed_thal"], got["seed_tolerant"]) == ("-1", "", "", "false")
    # read whenever a round can seed: with a panel, or with re-pick rounds
    for seeds in (("--existing-primers", "p.csv"), ("--repick-rounds", "2")):
        rc_, out = parse(host, *base, *seeds, "--seed-mismatches", "1")
        got = kv(out)
        assert rc_ == 0 and (got["seed_mismatches"], got["seed_3p_exact"], got["seed_tolerant"]) == ("1", "3", "true")
        rc_, out = parse(host, *base, *seeds, "--seed-mismatches", "2", "--seed-3p-exact", "0", "--seed-tm", "-2.5",
                         "--seed-thal", "end1")
        got = kv(out)
        assert rc_ == 0 and (got["seed_mismatches"], got["seed_3p_exact"], got["seed_tm"], got["seed_thal"]) == (
            "2", "0", "-2.5", "end1")
        rc_, out = parse(host, *base, *seeds, "--seed-tm", "30")          # thal alone: exact matches, scored
        got = kv(out)
        assert rc_ == 0 and (got["seed_mismatches"], got["seed_thal"], got["seed_tolerant"]) == ("0", "any", "true")
        assert kv(parse(host, *base, *seeds)[1])["seed_tolerant"] == "false"   # unset: today's exact seeding
        for bad in (("--seed-mismatches", "14"), ("--seed-mismatches", "1", "--seed-3p-exact", "14"),
                    ("--seed-mismatches", "1", "--seed-3p-exact", "x"), ("--seed-tm", "warm"), ("--seed-tm", "nan"),
                    ("--seed-tm", "30", "--seed-thal", "end2"), ("--seed-tm", "30", "--kmer-size", "1")):
            rc_, out = parse(host, *base, *seeds, *bad)
            assert rc_ == 2 and "--seed-" in out, (bad, out)
    # otherwise the values are ignored, whatever they say
    rc_, out = parse(host, *base, "--seed-mismatches", "99", "--seed-3p-exact", "x", "--seed-tm", "warm")
    assert rc_ == 0 and kv(out)["seed_tolerant"] == "false"
    # --seed-thal without --seed-tm, and any of them with --devices, are usage errors wherever they stand
    for seeds in ((), ("--existing-primers", "p.csv")):
        rc_, out = parse(host, *base, *seeds, "--seed-thal", "any")
        assert rc_ == 2 and "'--seed-thal' needs '--seed-tm <C>'" in out
        for flag in (("--seed-mismatches", "1"), ("--seed-3p-exact", "3"), ("--seed-tm", "30"),
                     ("--seed-tm", "30", "--seed-thal", "any")):
            rc_, out = parse(host, *base, *seeds, *flag, "--devices", "0,1")
            assert rc_ == 2 and "--seed-mismatches" in out and "--devices" in out, flag
    monkeypatch.setenv("SEED_MISMATCHES", "2")
    monkeypatch.setenv("SEED_3P_EXACT", "4")
    monkeypatch.setenv("EXISTING_PRIMERS", "p.csv")
    got = kv(parse(host, *base)[1])
    assert (got["seed_mismatches"], got["seed_3p_exact"], got["seed_tolerant"]) == ("2", "4", "true")
    rc_, out = parse(host, "--help")
    assert rc_ == 2
    for flag, env in (("--seed-mismatches", "SEED_MISMATCHES"), ("--seed-3p-exact", "SEED_3P_EXACT"),
                      ("--seed-tm", "SEED_TM"), ("--seed-thal", "SEED_THAL")):
        assert f"{flag} <...>  [env: {env}=]" in out


def test_the_host_text_is_the_models_render(host):
    host.odm_seed_block.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float] + [C.c_longlong] * 5 + [C.c_char_p, C.c_size_t]
    for M, E, mode, thr, (af, cf, ar, cr, b) in ((1, 3, 0, 0.0, (120, 7, 0, 0, 400)),
                                                   (2, 0, 2, 41.256, (1, 3, 4, 6, 1000000)),
                                                   (0, 13, 1, -5.0, (0, 0, 9, 2, 9))):
        buf = C.create_string_buffer(1 << 12)
        n = host.odm_seed_block(M, E, mode, thr, af, cf, ar, cr, b, buf, 1 << 12)
        assert n > 0 and buf.value.decode() == render_block(M, E, (af, b, cf), (ar, b, cr), mode, thr)
    assert render_block(1, 3, (120, 400, 7), (5, 400, 2), "any", 30.0) == (
        "\nSeeding (up to 1 mismatches, last 3 bases exact; thal ANY, t >= 30.00 C):\n"
        "  Forward: 120 of 400 segments covered by 7 panel primers; Reverse: 5 of 400 segments covered by 2 panel primers\n")
