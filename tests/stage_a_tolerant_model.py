"""A tolerant seeded stage A restated on the CPU (msspe_kmer_candidates_tolerant*, include/msspe_hip.h).

It is SeededModel (tests/stage_a_seeded_model.py) whose seed push takes its segment list not from the word's postings
but from a row of an incidence matrix computed with that direction's words only: panel_thin_model.incidence (mode 0: a
match within M mismatches, the last E bases exact) or panel_thin_thal_model.held_incidence (modes 1 and 2: a match
that thal scores stable at the threshold).  Direction 0 puts the seeds in as forward primers (head window), direction 1
as reverse primers (tail window, reverse-complemented candidate).  The winners' pushes, the loop and its stop rules
are SeededModel's; exclusions act on the index alone (stage_a_excluding_model._Without), never on what a seed covers.

Besides the winners it returns the state before the first iteration: ignored as uint8 (n_seq, P) and coverage as
uint32 (P).  Also renders the block od-msspe-hip prints for a seeding round."""
from __future__ import annotations

import numpy as np

import coverage_thal_model as ctm
import panel_thin_model as ptm
import panel_thin_thal_model as pttm
from stage_a_excluding_model import _Without
from stage_a_seeded_model import SeededModel

_ONE = np.float32(1.0)


def seed_incidence(rows: np.ndarray, fields, direction: int, seed, M: int, E: int, mode=0, tm_threshold: float = 0.0,
                   tables=None, args=None, cache=None):
    """(distinct seed words ascending, bool (n words, n_seq * P)): the segments each seed covers under the rule."""
    seg, stride, W, k = fields[:4]
    words = sorted(set(seed))
    fwd, rev = ([], words) if direction else (words, [])
    if mode in (0, None):
        I = ptm.incidence(rows, seg, stride, W, k, fwd, rev, M, E)
    else:
        res = ctm.coverage_thal(tables, rows, seg, stride, W, k, fwd, rev, M, E, mode, tm_threshold, args, cache=cache)
        I = pttm.held_incidence(res)
    return words, I


class TolerantModel(SeededModel):
    def __init__(self, segs, direction: int, rows: np.ndarray, fields, exclude=()):
        super().__init__(_Without(segs, exclude) if len(exclude) else segs, direction)
        self.rows, self.fields = np.ascontiguousarray(rows, dtype=np.uint8), tuple(fields)
        n, L = self.rows.shape
        self.n_seq = n
        self.P = ptm.n_partitions(L, fields[0], fields[1])
        assert len(self.part) == n * self.P and all(p == s % self.P for s, p in enumerate(self.part)), \
            "the model numbers segments s = r * P + j"

    def candidates_tolerant(self, max_iterations: int, max_mismatch_segments: int, seed=(), M: int = 0, E: int = 0,
                            mode=0, tm_threshold: float = 0.0, tables=None, args=None, cache=None):
        """(winners [(word, frequency)], seed_covered uint8 (n_seq, P), seed_partitions uint32 (P))."""
        _, I = seed_incidence(self.rows, self.fields, self.direction, seed, M, E, mode, tm_threshold, tables, args, cache)
        return self.candidates_from([np.flatnonzero(row).tolist() for row in I], max_iterations, max_mismatch_segments)

    def candidates_from(self, seed_segments, max_iterations: int, max_mismatch_segments: int):
        """SeededModel.candidates with every seed's segment list given (one list per distinct seed)."""
        ignored = [False] * len(self.words)
        coverage = np.zeros(self.P, dtype=np.uint32)
        counts = np.array([len(self.index[w]) for w in self.vocab], dtype=np.int64)

        def push(segs):   # main.rs:371-378 over a segment list: each covered, each distinct partition bumped once
            for s in segs:
                if not ignored[s]:
                    ignored[s] = True
                    for w in self.words[s]:
                        counts[self.wid[w]] -= 1
            for p in {self.part[s] for s in segs}:
                coverage[p] += 1

        for segs in seed_segments:
            push(segs)
        covered = np.array(ignored, dtype=np.uint8).reshape(self.n_seq, self.P)
        partitions = coverage.copy()
        out = []
        for _ in range(max_iterations):
            maxf = int(counts.max()) if len(counts) else 0
            if maxf <= 1:   # no live word left, or only singletons
                break
            best, best_score = None, None
            for i in np.flatnonzero(counts == maxf):   # ascending words
                w = self.vocab[int(i)]
                score, seen = np.float32(0.0), set()
                for s in self.index[w]:
                    p = self.part[s]
                    if ignored[s] or p in seen:
                        continue
                    seen.add(p)
                    score = np.float32(score + _ONE / (np.float32(coverage[p]) + _ONE))
                if best is None or score > best_score:   # the smallest word wins a tie
                    best, best_score = w, score
            out.append((best, maxf))
            push(self.index[best])
            if maxf < max_mismatch_segments:
                break
        return out, covered, partitions


def first_base_changed(words, vocab, k: int):
    """Each word with its 5' base changed so that the result is absent from `vocab` (and from the words made so far);
    a word for which no base does is left out."""
    have, out = set(vocab), []
    for w in words:
        for b in "ACGT":
            x = b + w[1:]
            if x != w and x not in have and x not in out:
                out.append(x)
                break
    return out


def render_block(M: int, E: int, fwd, rev, mode=0, tm_threshold: float = 0.0) -> str:
    """The text od-msspe-hip prints for a seeding round.  fwd / rev: (segments covered, segments, panel primers) of the
    direction; mode 0: the match rule alone, "any" / "end1" (1 / 2): thal at tm_threshold."""
    head = "\nSeeding (up to %d mismatches, last %d bases exact" % (M, E)
    if mode not in (0, None):
        name = {1: "ANY", 2: "END1", "any": "ANY", "end1": "END1"}[mode]
        head += "; thal %s, t >= %.2f C" % (name, float(np.float32(tm_threshold)))
    return head + "):\n  Forward: %d of %d segments covered by %d panel primers; Reverse: %d of %d segments covered by %d panel primers\n" % (
        tuple(fwd) + tuple(rev))
