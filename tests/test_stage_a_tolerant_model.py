"""The tolerant seeded restatement of stage A (tests/stage_a_tolerant_model.py) on the CPU, on the four alignments of
stage_a_excluding_model.cases in both directions: the identities include/msspe_hip.h states for
msspe_kmer_candidates_tolerant*, and that the rule is not vacuous -- seeds one 5' mismatch away from the unseeded
winners, which exact seeding ignores, keep those winners out.  One input with stable and unstable matches separates
the thal modes from mode 0.  No GPU."""
import numpy as np
import pytest

import coverage_mm_model as cm
import coverage_thal_model as ctm
from stage_a_excluding_model import CachedSegments, ExcludingModel, cases
from stage_a_seeded_model import SeededModel
from stage_a_tolerant_model import TolerantModel, first_base_changed, render_block, seed_incidence
from test_panel_thin_thal_model import grid_input

NAMES = ["synth", "ties-k3", "ties-k5", "wide-k17"]
M_SEEDS = 3   # W[:m]


@pytest.fixture(scope="module")
def built(oracle):
    import msspe_amd
    out = {}
    for name, rows, fields in cases(msspe_amd):
        segs = CachedSegments(oracle.Segments([bytes(x).decode() for x in rows], *fields[:4]))
        out[name] = (segs, rows, fields)
    return out


ABSENT = ("synth", "wide-k17")   # cases whose first winners have 5' variants that occur nowhere in the alignment


def near_seeds(name, model, winners, k):
    """W[:m] with the 5' base changed: to words absent from the index where there are such (ABSENT).  ties-k3 holds all
    64 3-mers and ties-k5 four fifths of the 5-mers, so there the changed words are merely none of W[:m]."""
    w = [x for x, _ in winners[:M_SEEDS]]
    if name not in ABSENT:
        return [next(b + x[1:] for b in "ACGT" if b + x[1:] not in w) for x in w]
    seeds = first_base_changed(w, model.vocab, k)
    assert len(seeds) == M_SEEDS and not set(seeds) & set(model.vocab)
    return seeds


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_identities(built, name, direction):
    segs, rows, fields = built[name]
    k, mi, mms = fields[3], fields[4], fields[5]
    plain = SeededModel(segs, direction)
    winners = plain.candidates(mi, mms)
    model = TolerantModel(segs, direction, rows, fields)
    # no seed: the unseeded run, nothing ignored
    got, covered, parts = model.candidates_tolerant(mi, mms, [], 2, 3)
    assert got == winners and not covered.any() and not parts.any()
    # mode 0, no mismatch, any exact_3p: the exact-seeded run
    seed = [w for w, _ in winners[1:4]] + [winners[1][0]]
    want = plain.candidates(mi, mms, seed=seed)
    assert want != winners
    for E in (0, 3, k):
        got, covered, parts = model.candidates_tolerant(mi, mms, seed, 0, min(E, k))
        assert got == want, (name, direction, E)
        # the state outputs are the exact postings' segments and their partitions, one bump per distinct seed
        segs_of = [set(plain.index[w]) for w in set(seed)]
        flat = covered.reshape(-1)
        assert set(np.flatnonzero(flat).tolist()) == set().union(*segs_of)
        want_parts = np.zeros(model.P, dtype=np.uint32)
        for ss in segs_of:
            for p in {plain.part[s] for s in ss}:
                want_parts[p] += 1
        np.testing.assert_array_equal(parts, want_parts)
    # ... also with exclusions that share no word with the seeds
    exclude = [w for w, _ in winners[5:8]]
    want = ExcludingModel(segs, direction, exclude).candidates(mi, mms, seed=seed)
    got, _, _ = TolerantModel(segs, direction, rows, fields, exclude).candidates_tolerant(mi, mms, seed, 0, 0)
    assert got == want
    # seed_covered is best != 255 of the mismatch coverage with this direction's seeds alone
    near = near_seeds(name, plain, winners, k)
    for M, E in ((1, min(3, k)), (2, 0)):
        got, covered, parts = model.candidates_tolerant(mi, mms, near + seed, M, E)
        fwd, rev = ([], near + seed) if direction else (near + seed, [])
        best, _ = cm.best_matrix(rows, fields[0], fields[1], fields[2], k, fwd, rev, M, E)
        np.testing.assert_array_equal(covered != 0, best != 255)
        # order and duplicates do not matter
        again = model.candidates_tolerant(mi, mms, (seed + near)[::-1] + near, M, E)
        assert again[0] == got and (again[1] == covered).all() and (again[2] == parts).all()
        # exclusions do not change what a seed covers
        ex = TolerantModel(segs, direction, rows, fields, exclude).candidates_tolerant(mi, mms, near + seed, M, E)
        np.testing.assert_array_equal(ex[1], covered)
        np.testing.assert_array_equal(ex[2], parts)
        assert not {w for w, _ in ex[0]} & set(exclude)


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_near_seeds_cover_what_exact_seeding_ignores(built, name, direction):
    segs, rows, fields = built[name]
    k, mi, mms = fields[3], fields[4], fields[5]
    plain = SeededModel(segs, direction)
    winners = plain.candidates(mi, mms)
    assert len(winners) > M_SEEDS + 2
    near = near_seeds(name, plain, winners, k)
    model = TolerantModel(segs, direction, rows, fields)
    exact = plain.candidates(mi, mms, seed=near)
    if name in ABSENT:
        assert exact == winners                          # absent from the index: exact seeding does nothing
    E = 3
    if name == "ties-k3":
        # k = 3: "the last 3 bases exact" is the whole word, so M = 1, E = 3 is exact seeding; the 5' base is free at E = 2
        assert model.candidates_tolerant(mi, mms, near, 1, 3)[0] == exact
        E = 2
    tolerant, covered, parts = model.candidates_tolerant(mi, mms, near, 1, E)
    assert tolerant != exact
    assert not {w for w, _ in tolerant} & {w for w, _ in winners[:M_SEEDS]}
    assert not {w for w, _ in tolerant} & set(near)      # seeds are never winners
    # every posting of W[:m] is covered before the first iteration, and each seed bumped its partitions
    flat = covered.reshape(-1)
    for w, _ in winners[:M_SEEDS]:
        assert flat[plain.index[w]].all()
    assert parts.sum() >= M_SEEDS


@pytest.fixture(scope="module")
def grid(oracle, oracle_tables):
    g, fwd, rev = grid_input()
    fields = (400, 170, 50, 13, 1000, 1)
    segs = CachedSegments(oracle.Segments([bytes(x).decode() for x in g], *fields[:4]))
    return g, fwd, rev, fields, segs, oracle_tables, oracle.ntthal_args()


@pytest.mark.parametrize("direction", [0, 1])
def test_thal_modes_differ_from_mode_0_where_matches_are_unstable(grid, direction):
    g, fwd, rev, fields, segs, tables, args = grid
    seed = rev if direction else fwd
    model = TolerantModel(segs, direction, g, fields)
    cache = {}
    w0, c0, p0 = model.candidates_tolerant(1000, 1, seed, 2, 3)
    results = {}
    for mode in ("any", "end1"):
        results[mode] = model.candidates_tolerant(1000, 1, seed, 2, 3, mode, 40.0, tables, args, cache)
        # a threshold of zero or less is mode 0
        z = model.candidates_tolerant(1000, 1, seed, 2, 3, mode, 0.0, tables, args, cache)
        assert z[0] == w0 and (z[1] == c0).all() and (z[2] == p0).all()
    w2, c2, p2 = results["end1"]
    assert c2.any() and (c0 & ~c2).any() and not (c2 & ~c0).any()   # stable and unstable matches both occur
    assert w2 != w0 and (p2 <= p0).all() and (p2 < p0).any()
    # seed_covered is held == 2 of the scored coverage with this direction's seeds alone
    f, r = ([], seed) if direction else (seed, [])
    res = ctm.coverage_thal(tables, g, 400, 170, 50, 13, f, r, 2, 3, "end1", 40.0, args, cache=cache)
    np.testing.assert_array_equal(c2 != 0, res["held"] == 2)
    # the incidence rows are this direction's alone: the other direction's words change nothing
    words, I = seed_incidence(g, fields, direction, seed, 2, 3)
    assert len(words) == len(set(seed)) and I.shape == (len(words), c0.size)


def test_block_text():
    assert render_block(1, 3, (120, 400, 7), (0, 400, 0)) == (
        "\nSeeding (up to 1 mismatches, last 3 bases exact):\n"
        "  Forward: 120 of 400 segments covered by 7 panel primers; Reverse: 0 of 400 segments covered by 0 panel primers\n")
    assert render_block(2, 0, (1, 2, 3), (4, 5, 6), "end1", 41.256) == (
        "\nSeeding (up to 2 mismatches, last 0 bases exact; thal END1, t >= 41.26 C):\n"
        "  Forward: 1 of 2 segments covered by 3 panel primers; Reverse: 4 of 5 segments covered by 6 panel primers\n")
