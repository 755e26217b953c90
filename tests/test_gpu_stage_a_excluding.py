"""Stage A with excluded words on the GPU (msspe_kmer_candidates_sets*, Engine.kmer_candidates*(exclude=...)).

For each case of tests/stage_a_excluding_model.py (the three of test_gpu_stage_a_seeded.py and one with 64-bit keys),
both directions, all three entry points and both loop drivers with and without graph replay, the device equals the
CPU restatement for the lists (a) to (e) of exclusion_lists(); (a), (b) and (e) must also differ from the plain
winners, so a kernel that does nothing cannot pass.  Empty lists are the seeded and unseeded calls; a plain call
after an excluded one on the same context equals a plain call before it; argument errors have their codes."""
import ctypes as C

import numpy as np
import pytest

from stage_a_excluding_model import CachedSegments, ExcludingModel, cases, exclusion_lists
from stage_a_seeded_model import SeededModel

pytestmark = pytest.mark.gpu

OPTS = [(cand, graph) for cand in (1, 0) for graph in (1, 0)]


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def expected(m, oracle):
    """Per case: rows, fields, and per direction the plain winners W and {label: (seed, exclude, want)} from the
    model -- computed once, shared by every parametrisation."""
    out = []
    for name, rows, fields in cases(m):
        segs = CachedSegments(oracle.Segments([bytes(x).decode() for x in rows], *fields[:4]))
        per_dir = {}
        for direction in (0, 1):
            plain = SeededModel(segs, direction)
            winners = plain.candidates(fields[4], fields[5])
            lists = {}
            for label, (seed, exclude) in exclusion_lists(name, direction, plain.vocab, winners, fields[3]).items():
                want = ExcludingModel(segs, direction, exclude).candidates(fields[4], fields[5], seed=seed)
                lists[label] = (seed, exclude, want)
            per_dir[direction] = (winners, lists)
        out.append((name, rows, fields, per_dir))
    return out


class Runner:
    """One alignment, resident both as host rows and as a packed device copy; the three entry points."""

    def __init__(self, eng, m, rows, fields):
        self.eng, self.opt, self.rows = eng, m.KmerOpt(*fields), rows
        self.d = eng.put_rows_packed(rows)

    def run(self, how, direction, seed=None, exclude=None):
        n, L = self.rows.shape
        if how == "host":
            w, f = self.eng.kmer_candidates(self.rows, self.opt, direction, seed=seed, exclude=exclude)
        elif how == "packed":
            w, f = self.eng.kmer_candidates_packed(self.d, n, L, self.opt, direction, seed=seed, exclude=exclude)
        else:
            kw = {("seed_fwd", "seed_rev")[direction]: seed, ("exclude_fwd", "exclude_rev")[direction]: exclude}
            w, f = self.eng.kmer_candidates_both_packed(self.d, n, L, self.opt, **kw)[direction]
        return list(zip(w, f.tolist()))

    def close(self):
        self.eng.device_free(self.d)


@pytest.mark.parametrize("cand,graph", OPTS, ids=[f"cand{c}-graph{g}" for c, g in OPTS])
def test_device_equals_the_model(eng, m, expected, cand, graph):
    eng.set_option("stage_a_candidates", cand)
    eng.set_option("stage_a_graph", graph)
    try:
        for name, rows, fields, per_dir in expected:
            r = Runner(eng, m, rows, fields)
            try:
                for direction in (0, 1):
                    winners, lists = per_dir[direction]
                    assert r.run("packed", direction) == winners, (name, direction)
                    for label, (seed, exclude, want) in lists.items():
                        if label in "abe":
                            assert want != winners, (name, direction, label)
                        if label == "d":
                            assert want == []
                        for how in ("host", "packed", "both"):
                            got = r.run(how, direction, seed=seed or None, exclude=exclude)
                            assert got == want, (name, direction, label, how, got[:3], want[:3])
                    # a plain call after the excluded ones, on the same context
                    assert r.run("packed", direction) == winners, (name, direction, "plain after excluded")
            finally:
                r.close()
    finally:
        eng.set_option("stage_a_candidates", 1)
        eng.set_option("stage_a_graph", 1)


def test_both_directions_excluded_in_one_call(eng, m, expected):
    for name, rows, fields, per_dir in expected:
        r = Runner(eng, m, rows, fields)
        try:
            n, L = rows.shape
            (s0, x0, want0), (s1, x1, want1) = per_dir[0][1]["c"], per_dir[1][1]["c"]
            (w0, f0), (w1, f1) = eng.kmer_candidates_both_packed(r.d, n, L, r.opt, seed_fwd=s0, seed_rev=s1,
                                                                 exclude_fwd=x0, exclude_rev=x1)
            assert list(zip(w0, f0.tolist())) == want0, name
            assert list(zip(w1, f1.tolist())) == want1, name
        finally:
            r.close()


def test_empty_lists_are_the_seeded_and_unseeded_calls(eng, m, expected):
    for name, rows, fields, per_dir in expected:
        r = Runner(eng, m, rows, fields)
        try:
            for direction in (0, 1):
                winners = per_dir[direction][0]
                seed = [w for w, _ in winners[1:3]]
                seeded = r.run("packed", direction, seed=seed)
                for how in ("host", "packed", "both"):
                    assert r.run(how, direction, exclude=[]) == winners, (name, how, direction)
                    assert r.run(how, direction, seed=[], exclude=[]) == winners, (name, how, direction)
                    assert r.run(how, direction, seed=seed, exclude=[]) == seeded, (name, how, direction)
            # sets == NULL: both lists empty
            n, L = rows.shape
            words = np.zeros(fields[4], dtype=np.uint64)
            freqs = np.zeros(fields[4], dtype=np.uint32)
            cnt = C.c_int(0)
            assert eng.L.msspe_kmer_candidates_sets_packed_dev(
                eng.ptr, C.c_void_p(r.d), n, L, C.byref(r.opt), 0, None, words.ctypes.data, freqs.ctypes.data,
                fields[4], C.byref(cnt)) == 0
            got = [(m.unpack_oligo(w, fields[3]), int(f)) for w, f in zip(words[:cnt.value], freqs[:cnt.value])]
            assert got == per_dir[0][0], name
        finally:
            r.close()


def test_argument_errors(eng, m):
    rows = m.synth.aligned_genomes(10, 3000)
    n, L = rows.shape
    opt = m.KmerOpt(500, 250, 50, 13, 100, 1)
    words = np.zeros(100, dtype=np.uint64)
    freqs = np.zeros(100, dtype=np.uint32)
    w2 = np.zeros(100, dtype=np.uint64)
    f2 = np.zeros(100, dtype=np.uint32)
    cnt, c2 = C.c_int(0), C.c_int(0)
    ok = m.pack_oligos([bytes(rows[0, :13]).decode()])
    high = np.array([1 << 26], dtype=np.uint64)   # a bit above 2 k
    S = m.capi.KmerSets
    bad = [S(None, 0, None, 2),                      # a NULL list with a positive count
           S(None, 2, None, 0),
           S(None, 0, ok.ctypes.data, -1),           # a negative count
           S(ok.ctypes.data, -1, None, 0),
           S(None, 0, high.ctypes.data, 1),          # a word with bits above 2 k, in either list
           S(high.ctypes.data, 1, ok.ctypes.data, 1)]
    good = S(None, 0, ok.ctypes.data, 1)
    d = eng.put_rows_packed(rows)
    try:
        before = eng.kmer_candidates_packed(d, n, L, opt, 0)
        for s in bad:
            assert eng.L.msspe_kmer_candidates_sets(eng.ptr, rows.ctypes.data, n, L, C.byref(opt), 0, C.byref(s),
                                                    words.ctypes.data, freqs.ctypes.data, 100, C.byref(cnt)) == 1
            assert eng.L.msspe_kmer_candidates_sets_packed_dev(eng.ptr, C.c_void_p(d), n, L, C.byref(opt), 1,
                                                               C.byref(s), words.ctypes.data, freqs.ctypes.data, 100,
                                                               C.byref(cnt)) == 1
            for fwd, rev in ((s, good), (good, s), (s, None), (None, s)):
                assert eng.L.msspe_kmer_candidates_both_sets_packed_dev(
                    eng.ptr, C.c_void_p(d), n, L, C.byref(opt), C.byref(fwd) if fwd else None,
                    C.byref(rev) if rev else None, words.ctypes.data, freqs.ctypes.data, C.byref(cnt),
                    w2.ctypes.data, f2.ctypes.data, C.byref(c2), 100) == 1
        # the context still works afterwards: a valid exclusion goes through, and a plain call is what it was
        w, _ = eng.kmer_candidates_packed(d, n, L, opt, 0, exclude=[bytes(rows[0, :13]).decode()])
        assert isinstance(w, list)
        after = eng.kmer_candidates_packed(d, n, L, opt, 0)
        assert after[0] == before[0] and after[1].tolist() == before[1].tolist()
        # Python: strings of the wrong length, or not ACGT
        with pytest.raises(ValueError):
            eng.kmer_candidates(rows, opt, 0, exclude=["ACGT"])
        with pytest.raises(ValueError):
            eng.kmer_candidates_packed(d, n, L, opt, 0, exclude=["A" * 14])
        with pytest.raises(ValueError):
            eng.kmer_candidates_both_packed(d, n, L, opt, exclude_rev=["ACGTNACGTACGT"])
        with pytest.raises(ValueError):
            eng.kmer_candidates_both_packed(d, n, L, opt, exclude_fwd=["ACGTNACGTACGT"])
    finally:
        eng.device_free(d)
