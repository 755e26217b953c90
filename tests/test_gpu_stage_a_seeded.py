"""Seeded stage A on the GPU (msspe_kmer_candidates_seeded*, Engine.kmer_candidates*(seed=...)).

The prefix invariant: with W the unseeded winners and m < |W|, seeding W[:m] (any order) with max_iterations - m
returns exactly W[m:], words and frequencies -- through all three entry points and both loop drivers, with and
without graph replays.  Arbitrary seeds (present, sharing segments, absent, repeated) against the CPU restatement in
tests/stage_a_seeded_model.py.  An empty seed is the unseeded call; argument errors have their documented codes."""
import ctypes as C
import json

import numpy as np
import pytest

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


def mutated(rows, length, rate, seed, gaps=False):
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, length)
    out = []
    for _ in range(rows):
        row = anc.copy()
        mut = rng.random(length) < rate
        row[mut] = rng.integers(0, 4, int(mut.sum()))
        s = "".join("ACGT"[x] for x in row)
        out.append(s[:120] + "-" * 7 + s[127:300] + "N" * 3 + s[303:] if gaps else s)
    return out


def as_array(seqs):
    return np.frombuffer("".join(seqs).encode(), dtype=np.uint8).reshape(len(seqs), -1)


# (name, rows as uint8, KmerOpt fields); "ties" (k = 3 / 5 on 40-column segments) ties at nearly every iteration
def cases(m):
    return [
        ("synth", m.synth.aligned_genomes(40, 6000), (500, 250, 50, 13, 1000, 1)),
        ("ties-k3", as_array(mutated(25, 400, 0.05, 5, gaps=True)), (40, 20, 12, 3, 1000, 1)),
        ("ties-k5", as_array(mutated(120, 400, 0.03, 7)), (40, 20, 12, 5, 1000, 2)),
    ]


class Runner:
    """One alignment, resident both as host rows and as a packed device copy; the three seeded entry points."""

    def __init__(self, eng, m, rows, fields):
        self.eng, self.m, self.rows, self.fields = eng, m, rows, fields
        self.d = eng.put_rows_packed(rows)

    def opt(self, iters=None):
        f = list(self.fields)
        if iters is not None:
            f[4] = iters
        return self.m.KmerOpt(*f)

    def run(self, how, direction, iters=None, seed=None):
        n, L = self.rows.shape
        if how == "host":
            w, f = self.eng.kmer_candidates(self.rows, self.opt(iters), direction, seed=seed)
        elif how == "packed":
            w, f = self.eng.kmer_candidates_packed(self.d, n, L, self.opt(iters), direction, seed=seed)
        else:
            kw = {("seed_fwd", "seed_rev")[direction]: seed}
            both = self.eng.kmer_candidates_both_packed(self.d, n, L, self.opt(iters), **kw)
            w, f = both[direction]
        return list(zip(w, f.tolist()))

    def close(self):
        self.eng.device_free(self.d)


def prefix_sizes(n):
    return sorted({x for x in (1, 2, 7, n // 2, n - 1) if 1 <= x < n})


@pytest.mark.parametrize("cand,graph", OPTS, ids=[f"cand{c}-graph{g}" for c, g in OPTS])
def test_prefix_invariant_on_synthetic_alignments(eng, m, cand, graph):
    eng.set_option("stage_a_candidates", cand)
    eng.set_option("stage_a_graph", graph)
    try:
        for name, rows, fields in cases(m):
            r = Runner(eng, m, rows, fields)
            try:
                rng = np.random.default_rng(len(name))
                for direction in (0, 1):
                    w = r.run("packed", direction)
                    assert len(w) >= 3, (name, direction)
                    assert r.run("host", direction) == w
                    for mm in prefix_sizes(len(w)):
                        seed = [x for x, _ in w[:mm]]
                        rng.shuffle(seed)
                        for how in ("host", "packed", "both"):
                            got = r.run(how, direction, fields[4] - mm, seed)
                            assert got == w[mm:], (name, direction, how, mm, got[:2], w[mm:mm + 2])
            finally:
                r.close()
    finally:
        eng.set_option("stage_a_candidates", 1)
        eng.set_option("stage_a_graph", 1)


def test_prefix_invariant_at_config2_size(eng, m, golden_dir):
    """The 10,000 x 30,000 alignment of BASELINE configs[2]: W is the oracle fixture's winner list."""
    fx = json.loads((golden_dir / "config2_10k.json").read_text())
    rows = m.synth.aligned_genomes(fx["rows"], fx["length"])
    o = fx["options"]
    r = Runner(eng, m, rows, (o["segment"], o["stride"], o["window"], o["k"], o["max_iterations"],
                              o["max_mismatch_segments"]))
    n, L = rows.shape
    rng = np.random.default_rng(2)
    try:
        w = {d: [(x, f) for x, f in fx["winners"][str(d)]] for d in (0, 1)}
        for cand in (1, 0):
            eng.set_option("stage_a_candidates", cand)
            try:
                for mm in prefix_sizes(min(len(w[0]), len(w[1]))):
                    seeds = {}
                    for d in (0, 1):
                        seeds[d] = [x for x, _ in w[d][:mm]]
                        rng.shuffle(seeds[d])
                        assert r.run("packed", d, o["max_iterations"] - mm, seeds[d]) == w[d][mm:], (cand, d, mm)
                    (w0, f0), (w1, f1) = eng.kmer_candidates_both_packed(
                        r.d, n, L, r.opt(o["max_iterations"] - mm), seed_fwd=seeds[0], seed_rev=seeds[1])
                    assert list(zip(w0, f0.tolist())) == w[0][mm:], (cand, "both", 0, mm)
                    assert list(zip(w1, f1.tolist())) == w[1][mm:], (cand, "both", 1, mm)
            finally:
                eng.set_option("stage_a_candidates", 1)
    finally:
        r.close()


@pytest.mark.parametrize("cand,graph", OPTS, ids=[f"cand{c}-graph{g}" for c, g in OPTS])
def test_arbitrary_seeds_equal_the_restatement(eng, m, oracle, cand, graph):
    """Seeds that are not winners: random words of the index, all the words of a few segments (seeds sharing
    segments), words absent from the alignment, and repeats."""
    eng.set_option("stage_a_candidates", cand)
    eng.set_option("stage_a_graph", graph)
    try:
        for name, rows, fields in cases(m):
            seqs = [bytes(x).decode() for x in rows]
            segs = oracle.Segments(seqs, *fields[:4])
            r = Runner(eng, m, rows, fields)
            try:
                k = fields[3]
                rng = np.random.default_rng(17 + k)
                for direction in (0, 1):
                    model = SeededModel(segs, direction)
                    words = sorted(model.index)
                    absent = []   # (at k = 3 every word may be present: then there is none)
                    for _ in range(200):
                        x = "".join("ACGT"[i] for i in rng.integers(0, 4, k))
                        if x not in model.index and x not in absent and len(absent) < 3:
                            absent.append(x)
                    some = [words[i] for i in rng.choice(len(words), min(25, len(words) // 4), replace=False)]
                    shared = [x for s in rng.choice(len(segs), 3, replace=False) for x in model.words[int(s)]]
                    for seed in (some, shared + absent, some[:5] + some[:5] + absent, absent or some[:1]):
                        want = model.candidates(fields[4], fields[5], seed)
                        for how in ("host", "packed", "both"):
                            assert r.run(how, direction, seed=seed) == want, (name, direction, how, len(seed))
            finally:
                r.close()
    finally:
        eng.set_option("stage_a_candidates", 1)
        eng.set_option("stage_a_graph", 1)


def test_empty_seed_is_the_unseeded_call(eng, m):
    for name, rows, fields in cases(m):
        r = Runner(eng, m, rows, fields)
        try:
            for direction in (0, 1):
                want = r.run("packed", direction)
                for how in ("host", "packed", "both"):
                    assert r.run(how, direction, seed=[]) == want, (name, how, direction)
            n, L = rows.shape
            plain = eng.kmer_candidates_both_packed(r.d, n, L, r.opt())
            seeded = eng.kmer_candidates_both_packed(r.d, n, L, r.opt(), seed_fwd=[], seed_rev=[])
            for d in (0, 1):
                assert plain[d][0] == seeded[d][0]
                np.testing.assert_array_equal(plain[d][1], seeded[d][1])
        finally:
            r.close()


def test_argument_errors(eng, m):
    rows = m.synth.aligned_genomes(10, 3000)
    n, L = rows.shape
    opt = m.KmerOpt(500, 250, 50, 13, 100, 1)
    words = np.zeros(100, dtype=np.uint64)
    freqs = np.zeros(100, dtype=np.uint32)
    cnt = C.c_int(0)
    L_ = eng.L
    ok_seed = m.pack_oligos([bytes(rows[0, :13]).decode()])
    high = np.array([1 << 26], dtype=np.uint64)   # a bit above 2 k
    d = eng.put_rows_packed(rows)
    try:
        # null seed with n_seed > 0, and a word with bits above 2 k: MSSPE_ERR_ARG (1), for all three entry points
        assert L_.msspe_kmer_candidates_seeded(eng.ptr, rows.ctypes.data, n, L, C.byref(opt), 0, None, 2,
                                               words.ctypes.data, freqs.ctypes.data, 100, C.byref(cnt)) == 1
        assert L_.msspe_kmer_candidates_seeded(eng.ptr, rows.ctypes.data, n, L, C.byref(opt), 0, high.ctypes.data, 1,
                                               words.ctypes.data, freqs.ctypes.data, 100, C.byref(cnt)) == 1
        assert L_.msspe_kmer_candidates_seeded_packed_dev(eng.ptr, C.c_void_p(d), n, L, C.byref(opt), 1, None, 1,
                                                          words.ctypes.data, freqs.ctypes.data, 100, C.byref(cnt)) == 1
        assert L_.msspe_kmer_candidates_seeded_packed_dev(eng.ptr, C.c_void_p(d), n, L, C.byref(opt), 1,
                                                          high.ctypes.data, 1, words.ctypes.data, freqs.ctypes.data,
                                                          100, C.byref(cnt)) == 1
        w2 = np.zeros(100, dtype=np.uint64)
        f2 = np.zeros(100, dtype=np.uint32)
        c2 = C.c_int(0)
        for sf, nf, sr, nr in ((None, 1, None, 0), (ok_seed.ctypes.data, 1, None, 3),
                               (high.ctypes.data, 1, None, 0), (None, 0, high.ctypes.data, 1)):
            assert L_.msspe_kmer_candidates_both_seeded_packed_dev(
                eng.ptr, C.c_void_p(d), n, L, C.byref(opt), sf, nf, sr, nr, words.ctypes.data, freqs.ctypes.data,
                C.byref(cnt), w2.ctypes.data, f2.ctypes.data, C.byref(c2), 100) == 1, (nf, nr)
        # the context still works afterwards, and a valid seed goes through
        w, _ = eng.kmer_candidates_packed(d, n, L, opt, 0, seed=[bytes(rows[0, :13]).decode()])
        assert isinstance(w, list)
        # Python: strings of the wrong length, or not ACGT
        with pytest.raises(ValueError):
            eng.kmer_candidates(rows, opt, 0, seed=["ACGT"])
        with pytest.raises(ValueError):
            eng.kmer_candidates_packed(d, n, L, opt, 0, seed=["A" * 14])
        with pytest.raises(ValueError):
            eng.kmer_candidates_both_packed(d, n, L, opt, seed_rev=["ACGTNACGTACGT"])
    finally:
        eng.device_free(d)
