"""Stage A seeded on what a panel covers, on the GPU (msspe_kmer_candidates_tolerant*, Engine.kmer_candidates_tolerant*).

The device is held against tests/stage_a_tolerant_model.py exactly -- winners, frequencies, the segments ignored before
the first iteration and coverage[] at that moment -- on the four alignments of stage_a_excluding_model.cases in both
directions, at M in {0, 1, 2} and E in {0, 3}, for seeds one 5' base away from the unseeded winners, seeds far from
everything, repeated and shuffled lists, the whole vocabulary and lists with exclusions; against the device's own
_sets, segment_coverage_mm and segment_coverage_thal calls; at the segment, partition and seed counts where the matrix
and the kernel change shape; in tiles; in the two thal modes; under both loop drivers; and on a context shared with the
calls whose buffers it borrows."""
import ctypes as C

import numpy as np
import pytest

import coverage_thal_model as ctm
import panel_thin_thal_model as pttm
from stage_a_excluding_model import CachedSegments, as_array, cases, mutated
from stage_a_seeded_model import SeededModel
from stage_a_tolerant_model import TolerantModel, first_base_changed
from test_panel_thin_thal_model import grid_input
from test_stage_a_tolerant_model import ABSENT, near_seeds

pytestmark = pytest.mark.gpu

OPTS = [(cand, graph) for cand in (1, 0) for graph in (1, 0)]
ALL_RULES = [(M, E) for M in (0, 1, 2) for E in (0, 3)]
TWO_RULES = [(1, 3), (2, 0)]
ROT = str.maketrans("ACGT", "CGTA")


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


def wl(res):
    return list(zip(res[0], res[1].tolist()))


def check(got, want, tag):
    assert wl(got) == want[0], (tag, wl(got)[:3], want[0][:3])
    np.testing.assert_array_equal(got[2], want[1], err_msg=str(tag))
    np.testing.assert_array_equal(got[3], want[2], err_msg=str(tag))


def rotated(words):
    """Each word with its 5' base replaced by the next one (A -> C -> G -> T -> A)."""
    return [w[0].translate(ROT) + w[1:] for w in words]


def segments_of(oracle, rows, fields):
    return CachedSegments(oracle.Segments([bytes(x).decode() for x in rows], *fields[:4]))


def random_rows(n, L, seed):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, (n, L))]


class Runner:
    """One alignment, resident both as host rows and as a packed device copy; the three entry points."""

    def __init__(self, eng, m, rows, fields):
        self.eng, self.m, self.opt, self.rows = eng, m, m.KmerOpt(*fields), np.ascontiguousarray(rows)
        self.d = eng.put_rows_packed(self.rows)

    def run(self, how, direction, seed, rule, exclude=None):
        n, L = self.rows.shape
        if how == "host":
            return self.eng.kmer_candidates_tolerant(self.rows, self.opt, direction, seed, rule, exclude=exclude)
        if how == "packed":
            return self.eng.kmer_candidates_tolerant_packed(self.d, n, L, self.opt, direction, seed, rule,
                                                            exclude=exclude)
        seeds = [None, None]
        excl = [None, None]
        seeds[direction], excl[direction] = seed, exclude
        return self.eng.kmer_candidates_tolerant_both_packed(self.d, n, L, self.opt, seeds[0], seeds[1], rule,
                                                             exclude_fwd=excl[0], exclude_rev=excl[1])[direction]

    def plain(self, direction, seed=None, exclude=None):
        n, L = self.rows.shape
        return wl(self.eng.kmer_candidates_packed(self.d, n, L, self.opt, direction, seed=seed, exclude=exclude))

    def close(self):
        self.eng.device_free(self.d)


@pytest.fixture(scope="module")
def expected(m, oracle):
    """Per case: rows, fields and per direction the plain winners and [(label, seed, exclude, M, E, want)] from the model,
    computed once and shared by every parametrisation."""
    out = []
    for name, rows, fields in cases(m):
        segs = segments_of(oracle, rows, fields)
        k, mi, mms = fields[3], fields[4], fields[5]
        per_dir = {}
        for direction in (0, 1):
            plain = SeededModel(segs, direction)
            winners = plain.candidates(mi, mms)
            model = TolerantModel(segs, direction, rows, fields)
            near = near_seeds(name, plain, winners, k) + [winners[1][0]]
            exclude = [w for w, _ in winners[5:8]]
            runs = []
            for M, E in ALL_RULES:
                runs.append(("near", near, None, M, min(E, k), model.candidates_tolerant(mi, mms, near, M, min(E, k))))
            rng = np.random.default_rng([len(name), direction, 77])
            far = ["".join("ACGT"[i] for i in rng.integers(0, 4, k)) for _ in range(5)]
            for M, E in TWO_RULES:
                E = min(E, k)
                shuffled = (near + [w for w, _ in winners[2:4]])[::-1] + near[:2]
                runs.append(("shuffled", shuffled, None, M, E, model.candidates_tolerant(mi, mms, shuffled, M, E)))
                with_ex = TolerantModel(segs, direction, rows, fields, exclude)
                runs.append(("excluding", near, exclude, M, E, with_ex.candidates_tolerant(mi, mms, near, M, E)))
                if name in ABSENT:   # random 13- and 17-mers lie farther than two mismatches from every window
                    want = model.candidates_tolerant(mi, mms, far, M, E)
                    assert not want[1].any() and want[0] == winners
                    runs.append(("far", far, None, M, E, want))
            per_dir[direction] = (winners, runs)
        out.append((name, rows, fields, per_dir))
    return out


@pytest.mark.parametrize("cand,graph", OPTS, ids=[f"cand{c}-graph{g}" for c, g in OPTS])
def test_device_equals_the_model(eng, m, expected, cand, graph):
    eng.set_option("stage_a_candidates", cand)
    eng.set_option("stage_a_graph", graph)
    try:
        for name, rows, fields, per_dir in expected:
            r = Runner(eng, m, rows, fields)
            try:
                for direction in (0, 1):
                    winners, runs = per_dir[direction]
                    assert r.plain(direction) == winners, (name, direction)
                    differs = 0
                    for label, seed, exclude, M, E, want in runs:
                        got = r.run("packed", direction, seed, m.seed_rule(M, E), exclude)
                        check(got, want, (name, direction, label, M, E))
                        assert eng.info("stage_a_tolerant_segments") == int(want[1].sum())
                        assert eng.info("stage_a_tolerant_tiles") == 1
                        differs += label == "near" and M == 1 and want[0] != winners
                    assert differs, (name, direction, "the near seeds change nothing")
                    # a plain call after the tolerant ones, on the same context
                    assert r.plain(direction) == winners, (name, direction, "plain after tolerant")
            finally:
                r.close()
    finally:
        eng.set_option("stage_a_candidates", 1)
        eng.set_option("stage_a_graph", 1)


def test_entry_points_agree_and_the_both_call_is_two_single_calls(eng, m, expected):
    for name, rows, fields, per_dir in expected:
        r = Runner(eng, m, rows, fields)
        try:
            n, L = rows.shape
            picked = {}
            for direction in (0, 1):
                for label, seed, exclude, M, E, want in per_dir[direction][1]:
                    if (M, E) != (1, min(3, fields[3])) or label not in ("near", "excluding"):
                        continue
                    for how in ("host", "packed", "both"):
                        check(r.run(how, direction, seed, m.seed_rule(M, E), exclude), want, (name, direction, label, how))
                    if label == "excluding":
                        picked[direction] = (seed, exclude, want)
            (s0, x0, want0), (s1, x1, want1) = picked[0], picked[1]
            got0, got1 = eng.kmer_candidates_tolerant_both_packed(r.d, n, L, r.opt, s0, s1,
                                                                  m.seed_rule(1, min(3, fields[3])), exclude_fwd=x0,
                                                                  exclude_rev=x1)
            check(got0, want0, (name, "both", 0))
            check(got1, want1, (name, "both", 1))
            assert eng.info("stage_a_tolerant_tiles") == 2
            assert eng.info("stage_a_tolerant_segments") == int(want0[1].sum()) + int(want1[1].sum())
            # one direction seeded, the other not: the unseeded one is the plain run
            got0, got1 = eng.kmer_candidates_tolerant_both_packed(r.d, n, L, r.opt, s0, [], m.seed_rule(1, min(3, fields[3])),
                                                                  exclude_fwd=x0)
            check(got0, want0, (name, "fwd only", 0))
            assert wl(got1) == per_dir[1][0] and not got1[2].any() and not got1[3].any()
        finally:
            r.close()


def test_identities_against_the_devices_other_calls(eng, m, expected):
    for name, rows, fields, per_dir in expected:
        r = Runner(eng, m, rows, fields)
        try:
            n, L = rows.shape
            k = fields[3]
            for direction in (0, 1):
                winners, runs = per_dir[direction]
                # no seed: the _sets call, nothing ignored; the tolerant infos say so
                got = r.run("packed", direction, [], m.seed_rule(2, 3 if k >= 3 else 0))
                assert wl(got) == winners and not got[2].any() and not got[3].any()
                assert eng.info("stage_a_tolerant_tiles") == 0 and eng.info("stage_a_tolerant_segments") == 0
                # mode 0 without mismatches, any exact_3p, no word in both lists: the _sets call's winners
                seed = [w for w, _ in winners[1:4]] + [winners[1][0]]
                exclude = [w for w, _ in winners[5:8]]
                for E in (0, min(3, k), k):
                    assert wl(r.run("packed", direction, seed, m.seed_rule(0, E))) == r.plain(direction, seed=seed)
                    assert wl(r.run("packed", direction, seed, m.seed_rule(0, E), exclude)) == \
                        r.plain(direction, seed=seed, exclude=exclude)
                # seed_covered is best != 255 of the mismatch coverage with this direction's seeds alone
                for label, seed, exclude, M, E, want in runs:
                    if label != "near":
                        continue
                    fwd, rev = ([], seed) if direction else (seed, [])
                    best = eng.segment_coverage_mm_packed(r.d, n, L, r.opt, fwd, rev, M, E)
                    np.testing.assert_array_equal(want[1] != 0, best != 255, err_msg=str((name, direction, M, E)))
        finally:
            r.close()


def test_the_whole_vocabulary_at_one_mismatch_leaves_nothing_to_pick(eng, m, oracle, expected):
    for name, rows, fields, per_dir in expected:
        if name not in ("ties-k5", "wide-k17"):
            continue
        segs = segments_of(oracle, rows, fields)
        r = Runner(eng, m, rows, fields)
        try:
            for direction in (0, 1):
                model = TolerantModel(segs, direction, rows, fields)
                want = model.candidates_tolerant(fields[4], fields[5], model.vocab, 1, 3)
                has_word = np.array([len(w) > 0 for w in model.words]).reshape(want[1].shape)
                assert want[0] == [] and (want[1] != 0)[has_word].all()
                check(r.run("packed", direction, model.vocab, m.seed_rule(1, 3)), want, (name, direction))
        finally:
            r.close()


def top_words(model, n):
    return sorted(model.vocab, key=lambda w: (-len(model.index[w]), w))[:n]


def small_case(eng, m, oracle, rows, fields, rules=((1, 3),), n_top=4, extra_seed=()):
    """Both directions of one small alignment against the model, seeds = the most frequent words with the 5' base
    rotated plus one as it is."""
    segs = segments_of(oracle, rows, fields)
    r = Runner(eng, m, rows, fields)
    try:
        for direction in (0, 1):
            model = TolerantModel(segs, direction, rows, fields)
            top = top_words(model, n_top)
            seed = rotated(top) + top[:1] + list(extra_seed)
            for M, E in rules:
                want = model.candidates_tolerant(fields[4], fields[5], seed, M, min(E, fields[3]))
                assert want[1].any() or not model.vocab
                check(r.run("packed", direction, seed, m.seed_rule(M, min(E, fields[3]))), want,
                      (rows.shape, fields, direction, M, E))
    finally:
        r.close()


@pytest.mark.parametrize("n_seq", [1, 63, 64, 65, 129])
def test_segment_counts_around_a_matrix_group(eng, m, oracle, n_seq):
    """P = 1, W - k + 1 = 16 positions: S = min(64, 2048 / 16) = 64 segments per group -- 1, S - 1, S, S + 1, 2 S + 1."""
    small_case(eng, m, oracle, as_array(mutated(n_seq, 40, 0.05, 100 + n_seq)), (40, 20, 20, 5, 1000, 1))


@pytest.mark.parametrize("n_seq", [7, 8, 9, 17])
def test_segment_counts_at_the_widest_window(eng, m, oracle, n_seq):
    """W - k + 1 = 256 positions, the widest window stage A's extraction takes: S = 8 -- S - 1, S, S + 1, 2 S + 1."""
    small_case(eng, m, oracle, as_array(mutated(n_seq, 268, 0.05, 200 + n_seq)), (268, 268, 268, 13, 1000, 1))


def test_a_window_of_more_than_2048_positions_is_stage_as_argument_error(eng, m):
    """S = 1 needs more than 2,048 window positions; stage A's extraction stops at 256, and the tolerant call reports
    what the _sets call reports."""
    rows = random_rows(3, 2200, 5)
    opt = m.KmerOpt(2200, 2200, 2100, 5, 10, 1)
    with pytest.raises(m.MsspeError) as plain:
        eng.kmer_candidates(rows, opt, 0, seed=["ACGTA"])
    with pytest.raises(m.MsspeError) as tolerant:
        eng.kmer_candidates_tolerant(rows, opt, 0, ["ACGTA"], m.seed_rule(1, 3))
    assert plain.value.code == tolerant.value.code == 1 and "too wide" in str(tolerant.value)


@pytest.mark.parametrize("P", [1, 31, 32, 33, 65])
def test_partition_counts_around_a_bitmap_word(eng, m, oracle, P):
    small_case(eng, m, oracle, as_array(mutated(9, 40 + 20 * (P - 1), 0.05, 300 + P)), (40, 20, 12, 5, 1000, 1))


@pytest.mark.parametrize("k", [16, 31])
def test_word_lengths_at_the_plane_form_boundaries(eng, m, oracle, k):
    """13 and 17 are among the four cases; 16 is the longest word of the 32-bit plane form, 31 the longest there is."""
    small_case(eng, m, oracle, as_array(mutated(40, 700, 0.02, 400 + k)), (120, 60, 40, k, 1000, 1), rules=((1, 3), (2, 0)))


@pytest.fixture(scope="module")
def many_seeds(oracle):
    import msspe_amd
    rows = msspe_amd.synth.aligned_genomes(12, 3000, seed=9)
    fields = (500, 250, 50, 13, 200, 1)
    segs = segments_of(oracle, rows, fields)
    rng = np.random.default_rng(2100)
    pool = {}
    for direction in (0, 1):
        model = TolerantModel(segs, direction, rows, fields)
        words = rotated(top_words(model, 1200))
        while len(set(words)) < 2100:
            words.append("".join("ACGT"[i] for i in rng.integers(0, 4, 13)))
        pool[direction] = (model, list(dict.fromkeys(words)))
    return rows, fields, pool


@pytest.mark.parametrize("n_seed", [0, 1, 63, 64, 65, 2100])
def test_seed_counts_around_a_matrix_row_pad(eng, m, many_seeds, n_seed):
    rows, fields, pool = many_seeds
    r = Runner(eng, m, rows, fields)
    try:
        for direction in (0, 1):
            model, words = pool[direction]
            seed = words[:n_seed]
            want = model.candidates_tolerant(fields[4], fields[5], seed, 1, 3)
            assert bool(want[1].any()) == (n_seed > 0)
            check(r.run("packed", direction, seed, m.seed_rule(1, 3)), want, (n_seed, direction))
            assert eng.info("stage_a_tolerant_tiles") == (1 if n_seed else 0)
    finally:
        r.close()


def test_two_seeds_sharing_segments_and_a_seed_matching_a_window_twice(eng, m, oracle):
    rows = as_array(mutated(30, 400, 0.02, 17))
    fields = (100, 50, 40, 13, 1000, 1)
    word = bytes(rows[0, 60:73]).decode()
    rows = rows.copy()
    planted = np.frombuffer(word.encode(), dtype=np.uint8)
    rows[:, 2:15] = planted            # twice in partition 0's head window ...
    rows[:, 22:35] = planted
    rows[:, 362:375] = planted         # ... and twice in the last partition's tail window
    rows[:, 385:398] = planted
    segs = segments_of(oracle, rows, fields)
    r = Runner(eng, m, rows, fields)
    try:
        for direction in (0, 1):
            model = TolerantModel(segs, direction, rows, fields)
            target = word if direction == 0 else ctm.revcomp(word)
            assert target in model.index
            variants = [b + target[1:] for b in "ACGT" if b != target[0]]   # three seeds, the same segments each
            want = model.candidates_tolerant(fields[4], fields[5], variants, 1, 3)
            part = 0 if direction == 0 else model.P - 1
            assert want[2][part] == 3 and want[1][:, part].all()            # claimed once, bumped once per seed
            check(r.run("packed", direction, variants, m.seed_rule(1, 3)), want, ("claims", direction))
    finally:
        r.close()


def test_tiles_of_seeds_add_up_and_the_matrix_cap_is_reported(eng, m):
    """panel_thin_matrix_max_mb = 1 over 1,500 segment groups: 64 seeds fill 768 KB, so 130 seeds take three tiles; the
    result is the one-tile call's.  Over 2,100 groups 64 seeds do not fit."""
    opt = m.KmerOpt(260, 260, 260, 5, 50, 1)             # S = 8 segments per group
    rows = random_rows(12000, 260, 3)
    rng = np.random.default_rng(4)
    words = ["".join("ACGT"[i] for i in w) for w in rng.integers(0, 4, (400, 5))]
    seed = list(dict.fromkeys(words))[:130]
    assert len(seed) == 130
    n, L = rows.shape
    d = eng.put_rows_packed(rows)
    try:
        for direction in (0, 1):
            for rule in (m.seed_rule(0, 0), m.seed_rule(1, 3)):
                one = eng.kmer_candidates_tolerant_packed(d, n, L, opt, direction, seed, rule)
                assert eng.info("stage_a_tolerant_tiles") == 1
                eng.set_option("panel_thin_matrix_max_mb", 1)
                try:
                    tiled = eng.kmer_candidates_tolerant_packed(d, n, L, opt, direction, seed, rule)
                    assert eng.info("stage_a_tolerant_tiles") == 3
                finally:
                    eng.set_option("panel_thin_matrix_max_mb", 8192)
                assert wl(tiled) == wl(one)
                np.testing.assert_array_equal(tiled[2], one[2])
                np.testing.assert_array_equal(tiled[3], one[3])
                fwd, rev = ([], seed) if direction else (seed, [])
                best = eng.segment_coverage_mm_packed(d, n, L, opt, fwd, rev, rule.max_mismatches, rule.exact_3p)
                np.testing.assert_array_equal(tiled[2] != 0, best != 255)
                assert tiled[2].any() and tiled[3].tolist() == [130]     # P = 1: every seed bumped the one partition
    finally:
        eng.device_free(d)
    big = random_rows(16800, 260, 6)
    eng.set_option("panel_thin_matrix_max_mb", 1)
    try:
        with pytest.raises(m.MsspeError) as e:
            eng.kmer_candidates_tolerant(big, opt, 0, seed[:3], m.seed_rule(1, 3))
        assert e.value.code == 5 and "64 seeds" in str(e.value)
    finally:
        eng.set_option("panel_thin_matrix_max_mb", 8192)
    assert eng.kmer_candidates_tolerant(big, opt, 0, seed[:3], m.seed_rule(1, 3))[2].any()   # under the default cap it runs


GRID_FIELDS = (400, 170, 50, 13, 1000, 1)


@pytest.fixture(scope="module")
def grid(m, oracle, oracle_tables):
    """The 10 x 2,600 alignment and 65 + 65 primers of the scored coverage's grid; per chemistry, mode and direction
    the model's scored matches (thresholds are applied to them afterwards)."""
    g, fwd, rev = grid_input()
    segs = segments_of(oracle, g, GRID_FIELDS)
    args = {"ntthal": oracle.ntthal_args(), "primer3": oracle.p3_args()}
    scored, models = {}, {}
    for direction in (0, 1):
        models[direction] = TolerantModel(segs, direction, g, GRID_FIELDS)
        f, r = ([], rev) if direction else (fwd, [])
        for chem in args:
            cache = {}
            for mode in ("any", "end1"):
                scored[chem, mode, direction] = ctm.coverage_thal(oracle_tables, g, 400, 170, 50, 13, sorted(set(f)),
                                                                  sorted(set(r)), 2, 3, mode, 30.0, args[chem], cache=cache)
    return g, fwd, rev, models, scored


def grid_want(grid, chem, mode, direction, thr):
    g, fwd, rev, models, scored = grid
    H = pttm.held_incidence(ctm.rethreshold(scored[chem, mode, direction], thr))
    return models[direction].candidates_from([np.flatnonzero(row).tolist() for row in H], 1000, 1)


@pytest.mark.parametrize("unique", [1, 0])
@pytest.mark.parametrize("chem", ["ntthal", "primer3"])
def test_thal_modes_against_the_model(eng, m, grid, chem, unique):
    g, fwd, rev, models, scored = grid
    c = m.Chem.ntthal() if chem == "ntthal" else m.Chem.primer3()
    r = Runner(eng, m, g, GRID_FIELDS)
    eng.set_option("thin_thal_unique", unique)
    try:
        for direction in (0, 1):
            seed = rev if direction else fwd
            mode0 = models[direction].candidates_tolerant(1000, 1, seed, 2, 3)
            differs = 0
            for mode in ("any", "end1"):
                for thr in (30.0, 40.0):
                    want = grid_want(grid, chem, mode, direction, thr)
                    differs += want[0] != mode0[0] and bool((mode0[1] & ~want[1]).any())
                    for how in ("packed", "host", "both"):
                        check(r.run(how, direction, seed, m.seed_rule(2, 3, mode, c, thr)), want,
                              (chem, mode, direction, thr, how))
                    # seed_covered is held == 2 of the scored coverage with this direction's seeds alone
                    f, rv = ([], seed) if direction else (seed, [])
                    held = eng.segment_coverage_thal(g, r.opt, f, rv, 2, 3, c, mode, thr)["held"]
                    np.testing.assert_array_equal(want[1] != 0, held == 2)
                # a threshold of zero or less is mode 0
                for thr in (0.0, -5.0):
                    check(r.run("packed", direction, seed, m.seed_rule(2, 3, mode, c, thr)), mode0, (chem, mode, thr))
            assert differs >= 2, "no unstable match on this input"
    finally:
        eng.set_option("thin_thal_unique", 1)
        r.close()


def test_a_small_work_list_splits_the_slabs(eng, m, grid):
    g, fwd, rev, models, scored = grid
    r = Runner(eng, m, g, GRID_FIELDS)
    eng.set_option("site_list_cap_log2", 12)
    try:
        for direction in (0, 1):
            seed = rev if direction else fwd
            want = grid_want(grid, "ntthal", "end1", direction, 30.0)
            check(r.run("packed", direction, seed, m.seed_rule(2, 3, "end1", m.Chem.ntthal(), 30.0)), want, direction)
            # the whole vocabulary: every window position matches its own word, more than the list holds at once
            top = models[direction].vocab
            got = r.run("packed", direction, top, m.seed_rule(2, 3, "end1", m.Chem.ntthal(), 30.0))
            assert eng.info("panel_thin_thal_matches") > 4096 and eng.info("panel_thin_thal_redone") >= 1
            eng.set_option("site_list_cap_log2", 22)
            whole = r.run("packed", direction, top, m.seed_rule(2, 3, "end1", m.Chem.ntthal(), 30.0))
            eng.set_option("site_list_cap_log2", 12)
            assert eng.info("panel_thin_thal_redone") == 0
            check(got, (wl(whole), whole[2], whole[3]), ("split slabs", direction))
            f, rv = ([], top) if direction else (top, [])
            held = eng.segment_coverage_thal(g, r.opt, f, rv, 2, 3, m.Chem.ntthal(), "end1", 30.0)["held"]
            np.testing.assert_array_equal(got[2] != 0, held == 2)
    finally:
        eng.set_option("site_list_cap_log2", 22)
        r.close()


def test_a_shared_context_gives_what_a_fresh_one_gives(eng, m, grid, expected):
    """Ten tolerant calls interleaved with the calls whose matrix, work list and tables they share."""
    g, fwd, rev, models, scored = grid
    opt = m.KmerOpt(*GRID_FIELDS)
    c = m.Chem.ntthal()
    pool = m.synth.pool_strings(m.synth.random_pool(64, 13))
    name, rows, fields, per_dir = expected[0]
    near = [x[1] for x in per_dir[0][1] if x[0] == "near"][0]

    def tolerant_calls(e):
        yield lambda: e.kmer_candidates_tolerant(g, opt, 0, fwd, m.seed_rule(2, 3))
        yield lambda: e.kmer_candidates_tolerant(g, opt, 1, rev, m.seed_rule(2, 3, "end1", c, 30.0))
        yield lambda: e.kmer_candidates_tolerant(rows, m.KmerOpt(*fields), 0, near, m.seed_rule(1, 3))
        yield lambda: e.kmer_candidates_tolerant(g, opt, 0, fwd, m.seed_rule(2, 3, "any", c, 40.0))
        yield lambda: e.kmer_candidates_tolerant(g, opt, 1, rev, m.seed_rule(1, 0))
        yield lambda: e.kmer_candidates_tolerant(rows, m.KmerOpt(*fields), 1, near, m.seed_rule(2, 0, "any", c, 30.0))
        yield lambda: e.kmer_candidates_tolerant(g, opt, 0, fwd[:5], m.seed_rule(0, 0))
        yield lambda: e.kmer_candidates_tolerant(g, opt, 1, rev, m.seed_rule(2, 3, "end1", m.Chem.primer3(), 30.0))
        yield lambda: e.kmer_candidates_tolerant(g, opt, 0, fwd, m.seed_rule(2, 3, "end1", c, 40.0))
        yield lambda: e.kmer_candidates_tolerant(g, opt, 1, rev[:7], m.seed_rule(2, 3))

    def others(e):
        return [lambda: e.panel_thin(g, opt, fwd, rev, 2, 3)[:3],
                lambda: e.panel_thin_thal(g, opt, fwd, rev, 2, 3, c, "end1", 30.0)[:3],
                lambda: e.segment_coverage_thal(g, opt, fwd, rev, 2, 3, c, "any", 30.0)["held"],
                lambda: e.cross_dimer(pool, c, -9000.0)["row_conflicts"]]

    fresh = []
    for i in range(10):
        e = m.Engine(0)
        try:
            fresh.append(list(tolerant_calls(e))[i]())
        finally:
            e.close()
    e = m.Engine(0)
    try:
        other_want = [f() for f in others(e)]
    finally:
        e.close()
    for i, call in enumerate(tolerant_calls(eng)):
        got = call()
        check(got, (wl(fresh[i]), fresh[i][2], fresh[i][3]), ("shared", i))
        other = others(eng)[i % 4]()
        want = other_want[i % 4]
        if isinstance(want, tuple):
            for a, b in zip(other, want):
                np.testing.assert_array_equal(a, b)
        else:
            np.testing.assert_array_equal(other, want)


def test_argument_errors_and_empty_inputs(eng, m):
    rows = m.synth.aligned_genomes(10, 3000)
    n, L = rows.shape
    opt = m.KmerOpt(500, 250, 50, 13, 100, 1)
    words, freqs = np.zeros(100, dtype=np.uint64), np.zeros(100, dtype=np.uint32)
    w2, f2 = np.zeros(100, dtype=np.uint64), np.zeros(100, dtype=np.uint32)
    cnt, c2 = C.c_int(0), C.c_int(0)
    ok = m.pack_oligos([bytes(rows[0, :13]).decode()])
    high = np.array([1 << 26], dtype=np.uint64)   # a bit above 2 k
    S = m.capi.KmerSets
    good = S(ok.ctypes.data, 1, None, 0)
    chem = m.Chem.ntthal()
    d = eng.put_rows_packed(rows)

    def single(sets, rule, direction=0, o=opt):
        return eng.L.msspe_kmer_candidates_tolerant_packed_dev(
            eng.ptr, C.c_void_p(d), n, L, C.byref(o), direction, C.byref(sets) if sets else None,
            C.byref(rule) if rule else None, words.ctypes.data, freqs.ctypes.data, 100, C.byref(cnt), None, None)

    def both(fwd, rev, rule):
        return eng.L.msspe_kmer_candidates_both_tolerant_packed_dev(
            eng.ptr, C.c_void_p(d), n, L, C.byref(opt), C.byref(fwd) if fwd else None, C.byref(rev) if rev else None,
            C.byref(rule) if rule else None, words.ctypes.data, freqs.ctypes.data, C.byref(cnt), w2.ctypes.data,
            f2.ctypes.data, C.byref(c2), 100, None, None, None, None)

    try:
        before = eng.kmer_candidates_packed(d, n, L, opt, 0)
        rule = m.seed_rule(1, 3)
        # the _sets calls' errors
        for s in (S(None, 2, None, 0), S(ok.ctypes.data, -1, None, 0), S(None, 0, None, 2), S(high.ctypes.data, 1, None, 0),
                  S(ok.ctypes.data, 1, high.ctypes.data, 1)):
            assert single(s, rule) == 1
            assert single(s, rule, 1) == 1
            assert both(s, good, rule) == 1 and both(good, s, rule) == 1
            assert eng.L.msspe_kmer_candidates_tolerant(eng.ptr, rows.ctypes.data, n, L, C.byref(opt), 0, C.byref(s),
                                                        C.byref(rule), words.ctypes.data, freqs.ctypes.data, 100,
                                                        C.byref(cnt), None, None) == 1
        assert single(good, rule, 2) == 1                        # a direction that is none
        # the rule's own: NULL, a mode outside 0..2, a thal mode without a chemistry
        assert single(good, None) == 1 and both(good, good, None) == 1
        for mode in (-1, 3):
            assert single(good, m.capi.SeedRule(1, 3, mode, C.pointer(chem), 30.0)) == 1
        for mode in (1, 2):
            assert single(good, m.capi.SeedRule(1, 3, mode, None, 30.0)) == 1
            assert both(good, good, m.capi.SeedRule(1, 3, mode, None, 30.0)) == 1
        # the mismatch coverage's: max_mismatches or exact_3p outside 0..k
        for M, E in ((-1, 3), (14, 3), (1, -1), (1, 14)):
            assert single(good, m.seed_rule(M, E)) == 1
        # the scored coverage's: k below 2 (MSSPE_ERR_K), in the thal modes only
        opt1 = m.KmerOpt(500, 250, 50, 1, 100, 1)
        one_word = m.pack_oligos(["A"])
        one = S(one_word.ctypes.data, 1, None, 0)
        assert single(one, m.seed_rule(0, 0, "any", chem, 30.0), 0, opt1) == 2
        assert single(one, m.seed_rule(0, 0), 0, opt1) == 0
        # sets == NULL, and empty lists: the unseeded call
        assert single(None, rule) == 0
        got = [(m.unpack_oligo(w, 13), int(f)) for w, f in zip(words[:cnt.value], freqs[:cnt.value])]
        assert got == wl(before)
        # records shorter than a segment: nothing to pick, nothing to report
        short = np.zeros((4, 300), dtype=np.uint8) + ord("A")
        w, f, cov, parts = eng.kmer_candidates_tolerant(short, opt, 0, [bytes(rows[0, :13]).decode()], rule)
        assert w == [] and cov.size == 0 and parts.size == 0
        # max_iterations 0: no winner, and the state all the same
        opt0 = m.KmerOpt(500, 250, 50, 13, 0, 1)
        seed = [bytes(rows[0, 5:18]).decode()]
        w, f, cov, parts = eng.kmer_candidates_tolerant(rows, opt0, 0, seed, m.seed_rule(0, 0))
        full = eng.kmer_candidates_tolerant(rows, opt, 0, seed, m.seed_rule(0, 0))
        assert w == [] and cov.any()
        np.testing.assert_array_equal(cov, full[2])
        np.testing.assert_array_equal(parts, full[3])
        # the context still works, and a plain call is what it was
        after = eng.kmer_candidates_packed(d, n, L, opt, 0)
        assert wl(after) == wl(before)
        with pytest.raises(ValueError):
            eng.kmer_candidates_tolerant(rows, opt, 0, ["ACGT"], rule)
        with pytest.raises(ValueError):
            eng.kmer_candidates_tolerant_packed(d, n, L, opt, 0, ["ACGTNACGTACGT"], rule)
    finally:
        eng.device_free(d)


def test_seeds_cover_although_every_word_is_excluded(eng, m, oracle, expected):
    """No word left in the index (everything excluded): nothing to pick, and the panel covers what it covers."""
    name, rows, fields, per_dir = expected[2]
    assert name == "ties-k5"
    segs = segments_of(oracle, rows, fields)
    r = Runner(eng, m, rows, fields)
    try:
        for direction in (0, 1):
            vocab = SeededModel(segs, direction).vocab
            seed = [x[1] for x in per_dir[direction][1] if x[0] == "near"][0]
            want = TolerantModel(segs, direction, rows, fields, vocab).candidates_tolerant(fields[4], fields[5], seed, 1, 3)
            free = TolerantModel(segs, direction, rows, fields).candidates_tolerant(fields[4], fields[5], seed, 1, 3)
            assert want[0] == [] and want[1].any()
            np.testing.assert_array_equal(want[1], free[1])
            check(r.run("packed", direction, seed, m.seed_rule(1, 3), vocab), want, (name, direction))
    finally:
        r.close()
