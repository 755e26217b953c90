"""The split of the conflict graph into reaction tubes (csrc/tube_split.hip), stated twice in numpy.

Graph: a symmetric bool (n, n) matrix s (cover_round_model.symmetrise).  A node with s[v, v] set is self-conflicting: it
goes to no tube, constrains nobody and nobody waits for it.  deg(v) = neighbours other than v (self-conflicting ones
included), key(v) = deg(v) << 32 | rank(v), static.

sequential(): visit the other nodes by descending key; v takes the lowest tube in [0, T) that holds no neighbour placed
earlier, or none (NONE = 255) -- and an unplaced node constrains nobody.

rounds(): what the device runs.  wait(v) = neighbours that are not self-conflicting and have a greater key; every node
with wait 0 decides at once (lowest tube not held by its decided, placed neighbours), each decision takes one off the
wait of every undecided neighbour, and a node whose wait reaches 0 decides in the next round."""
from __future__ import annotations

import numpy as np

from cover_round_model import HAND_BUILT, hand_built, lex_rank, random_words, symmetrise  # noqa: F401  (re-exported)

NONE = 255


def keys(s: np.ndarray, rank: np.ndarray) -> np.ndarray:
    n = s.shape[0]
    deg = (s & ~np.eye(n, dtype=bool)).sum(1).astype(np.int64)
    return (deg << 32) | np.asarray(rank, dtype=np.int64)


def sequential(s: np.ndarray, rank: np.ndarray, T: int) -> np.ndarray:
    """uint8[n]: the tube of every node, NONE for a node in no tube."""
    assert 1 <= T <= 64
    n = s.shape[0]
    tube = np.full(n, NONE, dtype=np.uint8)
    self_c = np.diag(s).copy() if n else np.zeros(0, bool)
    key = keys(s, rank)
    off = s & ~np.eye(n, dtype=bool)
    for v in sorted(np.nonzero(~self_c)[0].tolist(), key=lambda i: -int(key[i])):
        held = set(tube[off[v]].tolist())
        for t in range(T):
            if t not in held:
                tube[v] = t
                break
    return tube


def rounds(s: np.ndarray, rank: np.ndarray, T: int) -> tuple[np.ndarray, int]:
    """(uint8[n] tubes, rounds that decided nodes)."""
    assert 1 <= T <= 64
    n = s.shape[0]
    tube = np.full(n, NONE, dtype=np.uint8)
    if n == 0:
        return tube, 0
    self_c = np.diag(s).copy()
    key = keys(s, rank)
    off = s & ~np.eye(n, dtype=bool)
    counted = off & ~self_c[None, :] & (key[None, :] > key[:, None])
    wait = counted.sum(1).astype(np.int64)
    decided = self_c.copy()
    ready = ~self_c & (wait == 0)
    count = 0
    while ready.any():
        count += 1
        idx = np.nonzero(ready)[0]
        # tubes held by the decided, placed neighbours of each ready node (no two ready nodes are adjacent)
        nb = off[idx] & decided[None, :] & (tube != NONE)[None, :]
        held = np.zeros((idx.size, 65), dtype=bool)
        r, c = np.nonzero(nb)
        held[r, tube[c]] = True
        held[:, T:] = True
        first = held.argmin(1)                     # lowest free tube; all held: argmin gives 0 of an all-True row
        free = ~held[np.arange(idx.size), first]
        tube[idx] = np.where(free, first, NONE).astype(np.uint8)
        decided[idx] = True
        wait -= off[:, idx].sum(1)                 # every neighbour of a deciding node; only the undecided matter
        ready = ~decided & (wait == 0)
    assert decided.all()
    return tube, count


def check_assignment(s: np.ndarray, tube: np.ndarray, T: int) -> None:
    """Every tube is an independent set; tubes in use have no gaps; a self-conflicting node is in none; an unplaced node
    that is not self-conflicting has a neighbour in each of the T tubes."""
    n = s.shape[0]
    off = s & ~np.eye(n, dtype=bool)
    placed = tube != NONE
    assert (tube[placed] < T).all()
    a, b = np.nonzero(off)
    both = placed[a] & placed[b]
    assert not (tube[a[both]] == tube[b[both]]).any()
    used = np.unique(tube[placed])
    assert used.tolist() == list(range(used.size))
    self_c = np.diag(s) if n else np.zeros(0, bool)
    assert not placed[self_c].any()
    for v in np.nonzero(~placed & ~self_c)[0]:
        held = set(tube[off[v] & placed].tolist())
        assert held == set(range(T)), (v, held)
