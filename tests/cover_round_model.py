"""The round form of the reference's greedy vertex cover (od-msspe/src/main.rs:754-798), stated in numpy.

The sequential rule deletes the node with the most live neighbours (ties: the lexicographically greatest) until no live
node has a live neighbour.  The round form deletes, each round, every node whose key (live degree, lexicographic rank)
is greater than the key of each of its live neighbours other than itself; it ends in the same set and is
what csrc/conflict_cover.hip computes.  Self loops count: a node with its own bit set is its own neighbour, so its
degree includes itself while it is alive."""
from __future__ import annotations

import numpy as np


def symmetrise(b: np.ndarray, drop: np.ndarray | None = None) -> np.ndarray:
    """S = B | B^T of a bool (n, n) conflict matrix; drop (bool (n, n), symmetric): pairs that are never edges."""
    s = b | b.T
    if drop is not None:
        s = s & ~drop
    return s


def lex_rank(words: list[str]) -> np.ndarray:
    """rank[i] = position of words[i] in lexicographic order (the words are distinct)."""
    order = sorted(range(len(words)), key=lambda i: words[i])
    rank = np.empty(len(words), dtype=np.int64)
    rank[order] = np.arange(len(words))
    return rank


def round_cover(s: np.ndarray, rank: np.ndarray) -> tuple[np.ndarray, int]:
    """(deleted bool[n], rounds) of the round rule on a symmetric bool (n, n) matrix s; rounds counts the rounds that
    deleted nodes."""
    n = s.shape[0]
    alive = np.ones(n, dtype=bool)
    deleted = np.zeros(n, dtype=bool)
    off = s & ~np.eye(n, dtype=bool)
    rounds = 0
    while True:
        live = s & alive[None, :]
        deg = live.sum(1) * alive
        act = alive & (deg > 0)
        if not act.any():
            return deleted, rounds
        key = (deg.astype(np.int64) << 32) | rank
        nb_max = np.where(off & alive[None, :], key[None, :], -1).max(1) if n else np.zeros(0, np.int64)
        win = act & (key > nb_max)
        assert win.any()
        alive &= ~win
        deleted |= win
        rounds += 1


def random_words(n: int, k: int, rng: np.random.Generator) -> list[str]:
    """n distinct random k-mers."""
    out, seen = [], set()
    while len(out) < n:
        w = "".join("ACGT"[x] for x in rng.integers(0, 4, k))
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def hand_built(name: str, n: int) -> np.ndarray:
    """Directed conflict matrices (bool (n, n)) of the shapes the GPU tests run: star, path, clique, cycle, all-ties
    (a perfect matching: every node of degree 1), self-loop-only, empty, one-direction-only (a tournament-like upper
    triangle sampled at random: each pair in one order only)."""
    b = np.zeros((n, n), dtype=bool)
    idx = np.arange(n)
    if name == "star":
        b[0, 1:] = True
    elif name == "path":
        b[idx[:-1], idx[1:]] = True
    elif name == "clique":
        b[:] = True
        np.fill_diagonal(b, False)
    elif name == "cycle":
        if n > 1:
            b[idx, (idx + 1) % n] = True
    elif name == "all_ties":
        b[idx[0:n - 1:2], idx[1:n:2]] = True
    elif name == "self_loop_only":
        b[idx, idx] = idx % 3 == 0
    elif name == "empty":
        pass
    elif name == "one_direction":
        rng = np.random.default_rng(n)
        b = np.triu(rng.random((n, n)) < min(1.0, 8.0 / max(n, 1)), 1)
        b[idx[::5], idx[::5]] = True
    else:
        raise ValueError(name)
    return b


HAND_BUILT = ["star", "path", "clique", "cycle", "all_ties", "self_loop_only", "empty", "one_direction"]
