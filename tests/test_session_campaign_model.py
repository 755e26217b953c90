"""The session campaign's generators and expected values without a GPU (tests/session_campaign_model.py): schedules are
deterministic per seed and keep the schedule rules, the committed seeds together hold every family, k, option and chain
order, and every session's expected values are not vacuous.  Conditions on the generators, not measurements: a seed that
fails one needs another generator or another seed."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import background_model as bgm
import panel_thin_model as ptm
import session_campaign_model as scm

ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"


def test_eight_committed_seeds():
    assert len(scm.SEEDS) == 8 == len(set(scm.SEEDS))


@pytest.mark.parametrize("seed", scm.SEEDS)
def test_schedule_is_deterministic(seed):
    a, b = scm.schedule(seed), scm.schedule(seed)
    assert [c.describe() for c in a] == [c.describe() for c in b]
    for x, y in zip(a, b):
        if x.kind in ("any", "end", "ab", "detail", "sites"):      # inputs held as lists of strings
            assert x.data() == y.data()


@pytest.mark.parametrize("seed", scm.SEEDS)
def test_schedule_rules(seed):
    calls = scm.schedule(seed)
    assert len(calls) == 20 and [c.index for c in calls] == list(range(20))
    # shrink after grow: every family of the session at both ends of its range, with another k where it has one
    for family in {c.family for c in calls}:
        mine = [c for c in calls if c.family == family and c.kind != "tubes"]
        assert {c.size for c in mine} == {"large", "small"}, family
        if family in scm.KS:
            assert len({c.p["k"] for c in mine}) >= 2, family
    first = {c.family: c.size for c in reversed(calls) if c.kind != "tubes"}
    assert len(set(first.values())) == 1            # a session grows first or shrinks first, as a whole
    # neighbours follow each other, forwards or reversed
    kinds = [c.kind for c in calls]
    text = " ".join(kinds)
    for chain in scm.CHAINS.values():
        names = [kind for _, kind in chain]
        assert " ".join(names) in text or " ".join(names[::-1]) in text, names
    chem = [c for c in calls if c.block.startswith("chem:")]
    assert len({(c.p["chem"], c.p["thr"]) for c in chem}) == 1 and {c.kind for c in chem} == {"any", "end", "thal_any"}
    assert next(c for c in chem if c.kind == "thal_any").p["mode"] == "any"
    bg = [c for c in calls if c.block.startswith("background:")]
    assert len(bg) == 5 and all(c.data()["records"] is bg[0].data()["records"] for c in bg)
    assert len({(c.p["k"], c.p["M"], c.p["E"], c.p["chem"], c.p["thr"], c.p["mode"]) for c in bg}) == 1
    assert bg[[c.kind for c in bg].index("flank0")].p["flank"] == 0
    # the boundary sizes of the table
    ns = [c.p["n"] for c in calls if c.kind == "any"]
    assert any(n in (63, 64, 65) for n in ns) and any(n % 24 for n in ns if n > 65)
    for c in calls:
        if c.kind in ("stage_a", "coverage", "thin"):
            L = c.data()["g"].shape[1]
            assert (L - c.p["seg"]) % c.p["stride"], "a trailing partial segment"
            assert (c.data()["g"] == ord("-")).any() and (c.data()["g"] == ord("N")).any()
        if c.kind in ("sites", "thal", "thal_any", "flank", "flank0", "amplicons"):
            lens = [len(r) for r in c.data()["records"]]
            assert min(lens) < c.p["k"] and (c.size == "small" or max(lens) > 2 * 2048)
        if c.option:
            assert scm.OPTIONS[c.option[0]][0] == c.option[1] != scm.OPTIONS[c.option[0]][1]


def test_committed_seeds_cover_every_item():
    have, large_first = set(), 0
    for seed in scm.SEEDS:
        calls = scm.schedule(seed)
        have |= scm.covered(calls)
        large_first += calls[0].size == "large"
    assert not scm.required() - have, sorted(scm.required() - have, key=repr)
    assert 2 * large_first >= len(scm.SEEDS)


@pytest.fixture(scope="module")
def session_counters():
    """Every expected value of every committed session, once: counters per seed (and the calls, for the cross-checks)."""
    out = {}
    for seed in scm.SEEDS:
        calls = scm.schedule(seed)
        for c in calls:
            scm.expect(c)
        out[seed] = (scm.counters(calls), calls)
    return out


@pytest.mark.parametrize("seed", scm.SEEDS)
def test_expected_values_are_not_vacuous(session_counters, seed):
    n, _calls = session_counters[seed]
    assert n["any_some_conflicts"] and n["end_some_conflicts"]
    assert n["background_sites"] > 0 and n["background_stable"] > 0 and n["background_truncated"] > 0
    assert n["thin_dropped"] >= 1 and n["thin_kept"] >= 1
    assert n["tubes_used"] > 1 and n["tubes_unplaced"] >= 1
    assert n["cover_rounds"] > 1


def test_an_amplicon_exists_across_the_seeds(session_counters):
    assert sum(n["amplicons"] for n, _ in session_counters.values()) >= 1


@pytest.mark.parametrize("seed", scm.SEEDS)
def test_second_models_agree_on_a_small_case(session_counters, seed):
    _n, calls = session_counters[seed]
    # the string-compare triple loop against the bit-plane site model, on the head of the session's small streams
    c = next(c for c in calls if c.kind == "sites" and c.size == "small")
    records = [r[:160] for r in c.data()["records"]]
    primers = c.data()["primers"][:8] + [records[-1][5:5 + c.p["k"]].upper().replace("N", "A").replace("R", "A")]
    primers = [p for p in primers if len(p) == c.p["k"]]
    counts, sites = bgm.sites(records, primers, c.p["M"], c.p["E"])
    n_counts, n_sites = bgm.naive_sites(records, primers, c.p["M"], c.p["E"])
    np.testing.assert_array_equal(counts, n_counts)
    order = np.lexsort((n_sites["pos"], n_sites["strand"], n_sites["primer"]))
    np.testing.assert_array_equal(sites, n_sites[order])
    # the host layer's sequential thinning rule against the greedy model, on the session's small incidence matrix
    c = next(c for c in calls if c.kind == "thin" and c.size == "small")
    I, want = c.incidence, scm.expect(c)
    host = C.CDLL(str(HOST_LIB))
    host.odm_thin_panel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
    rows = ptm.pack_rows(I)
    n = I.shape[0]
    order, gains = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    keep, cov = np.full(n, 9, dtype=np.uint8), np.zeros(2, dtype=np.int64)
    forced = c.data()["forced"]
    picks = host.odm_thin_panel(rows.ctypes.data, n, rows.shape[1], c.p["min_gain"],
                                forced.ctypes.data if forced is not None else None, order.ctypes.data, gains.ctypes.data,
                                keep.ctypes.data, cov.ctypes.data)
    np.testing.assert_array_equal(order[:picks], want["order"])
    np.testing.assert_array_equal(gains[:picks], want["gains"])
    np.testing.assert_array_equal(keep, want["keep"])
    assert (int(cov[0]), int(cov[1])) == (want["covered_all"], want["covered_kept"])
