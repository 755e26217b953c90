"""A short Python restatement of find_candidates_kmers (od-msspe/src/main.rs:331-406) that starts from a seeded
state: every distinct seed word in the direction's index gets the post-push update of main.rs:371-378 once before
the first iteration.  Built on pyoracle.Segments (its segments, words and partitions); tie scores are f32 sums in
ascending segment order, as partition_tie_score adds them.  Used by the CPU model test and as the GPU tests' checker.
"""
from __future__ import annotations

import numpy as np

_ONE = np.float32(1.0)


class SeededModel:
    def __init__(self, segs, direction: int):
        self.direction = direction
        n = len(segs)
        self.part = [segs.partition_no(s) for s in range(n)]
        self.words = [segs.kmers(s, direction) for s in range(n)]
        self.index: dict[str, list[int]] = {}
        for s in range(n):
            for w in self.words[s]:
                self.index.setdefault(w, []).append(s)   # ascending segment order
        self.vocab = sorted(self.index)                   # word ids in lexicographic order
        self.wid = {w: i for i, w in enumerate(self.vocab)}

    def candidates(self, max_iterations: int, max_mismatch_segments: int, seed=()) -> list[tuple[str, int]]:
        ignored = [False] * len(self.words)
        coverage: dict[int, int] = {}
        # live counts: the reference recounts them every iteration; taking covered segments out is the same number
        counts = np.array([len(self.index[w]) for w in self.vocab], dtype=np.int64)

        def push(word):   # main.rs:371-378: every posting covered, each distinct partition bumped once
            segs = self.index[word]
            for s in segs:
                if not ignored[s]:
                    ignored[s] = True
                    for w in self.words[s]:
                        counts[self.wid[w]] -= 1
            for p in {self.part[s] for s in segs}:
                coverage[p] = coverage.get(p, 0) + 1

        for w in sorted(set(seed)):
            if w in self.index:
                push(w)
        out = []
        for _ in range(max_iterations):
            maxf = int(counts.max()) if len(counts) else 0
            if maxf == 0:   # no live word left
                break
            if maxf == 1:
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
                    score = np.float32(score + _ONE / (np.float32(coverage.get(p, 0)) + _ONE))
                if best is None or score > best_score:   # the smallest word wins a tie
                    best, best_score = w, score
            out.append((best, maxf))
            push(best)
            if maxf < max_mismatch_segments:
                break
        return out
