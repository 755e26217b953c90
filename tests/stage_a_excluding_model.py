"""Stage A with excluded words, restated on the CPU: SeededModel (tests/stage_a_seeded_model.py) over a view of
pyoracle.Segments whose kmers(s, d) omits the excluded words -- an excluded word occurs in no search window, every
other word keeps its occurrences.  A seed that is also excluded is then absent from the index and does nothing.

Also the alignments and the exclusion lists that the CPU model test and the GPU test share, so that both run the
same lists."""
from __future__ import annotations

import numpy as np

from stage_a_seeded_model import SeededModel


class _Without:
    """pyoracle.Segments (or anything with its three calls) minus a set of words."""

    def __init__(self, segs, exclude):
        self.segs, self.exclude = segs, frozenset(exclude)

    def __len__(self):
        return len(self.segs)

    def partition_no(self, s):
        return self.segs.partition_no(s)

    def kmers(self, s, direction):
        return [w for w in self.segs.kmers(s, direction) if w not in self.exclude]


class ExcludingModel(SeededModel):
    def __init__(self, segs, direction: int, exclude=()):
        super().__init__(_Without(segs, exclude), direction)


class CachedSegments:
    """The three calls of pyoracle.Segments answered from lists read once (a model per exclusion list re-reads them)."""

    def __init__(self, segs):
        n = len(segs)
        self.part = [segs.partition_no(s) for s in range(n)]
        self.words = [[segs.kmers(s, d) for s in range(n)] for d in (0, 1)]

    def __len__(self):
        return len(self.part)

    def partition_no(self, s):
        return self.part[s]

    def kmers(self, s, direction):
        return self.words[direction][s]


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


def cases(m):
    """(name, rows as uint8, KmerOpt fields): the three cases of test_gpu_stage_a_seeded.py, built the same way, and
    one whose keys need 64 bits (k = 17: 35 key bits)."""
    return [
        ("synth", m.synth.aligned_genomes(40, 6000), (500, 250, 50, 13, 1000, 1)),
        ("ties-k3", as_array(mutated(25, 400, 0.05, 5, gaps=True)), (40, 20, 12, 3, 1000, 1)),
        ("ties-k5", as_array(mutated(120, 400, 0.03, 7)), (40, 20, 12, 5, 1000, 2)),
        ("wide-k17", as_array(mutated(60, 900, 0.02, 11)), (120, 60, 30, 17, 1000, 1)),
    ]


LONG_LIST = 5000   # vocabulary words of list (e): more than the kernel stages in LDS (4096 keys)


def exclusion_lists(name, direction, vocab, winners, k):
    """The lists of one case and direction, as {label: (seed, exclude)}:
    a  W[0] and W[3:5] of the unseeded winners W;
    b  a quarter of the vocabulary at random, words absent from the index, and repeats;
    c  (a) together with seeds W[1:3], W[1] in both lists;
    d  the whole vocabulary;
    e  (synth only) LONG_LIST vocabulary words and absent ones."""
    rng = np.random.default_rng([len(name), direction, k])
    have = set(vocab)
    absent = []   # (at k = 3 every word may be present: then there is none)
    for _ in range(200):
        x = "".join("ACGT"[i] for i in rng.integers(0, 4, k))
        if x not in have and x not in absent and len(absent) < 3:
            absent.append(x)
    w = [x for x, _ in winners]
    a = [w[0]] + w[3:5]
    quarter = [vocab[i] for i in rng.choice(len(vocab), max(1, len(vocab) // 4), replace=False)]
    lists = {
        "a": ([], a),
        "b": ([], quarter + absent + quarter[:5]),
        "c": (w[1:3], a + [w[1]]),
        "d": ([], list(vocab)),
    }
    if name == "synth":
        assert len(vocab) > LONG_LIST + 100
        pick = [vocab[i] for i in rng.choice(len(vocab), LONG_LIST, replace=False)]
        lists["e"] = ([], pick + absent)
    return lists
