"""The split of the conflict graph into tubes (tests/tube_round_model.py): the round form, which is what
csrc/tube_split.hip computes, equals the sequential rule on hand-built and random graphs (self loops, edges in one
direction only); the facts DESIGN.md 4.9 quotes hold; every assignment is proper; and the host's assign_tubes
(odm_assign_tubes, fed the edges as text) gives the same assignment.  No GPU needed."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import tube_round_model as trm

ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
SIZES = [1, 63, 64, 65, 300]
TUBES = [1, 2, 3, 64]


@pytest.fixture(scope="module")
def host():
    import msspe_amd
    msspe_amd.load_library()              # libod_msspe_host.so depends on libmsspe_hip.so
    return C.CDLL(str(HOST_LIB))


def host_tubes(host, words, b, T):
    a, c = np.nonzero(b)
    text = "\n".join(f"{words[i]},{words[j]}" for i, j in zip(a.tolist(), c.tolist())).encode()
    cap = 32 * len(words) + 64
    buf = C.create_string_buffer(cap)
    rc = host.odm_assign_tubes("\n".join(words).encode(), text, T, buf, cap)
    assert rc >= 0
    rows = [l.split("\t") for l in buf.value.decode().splitlines()]
    assert [r[0] for r in rows] == words
    return np.array([trm.NONE if r[1] == "-" else int(r[1]) for r in rows], dtype=np.uint8)


def random_graph(n, density, seed, one_direction):
    rng = np.random.default_rng(seed)
    b = rng.random((n, n)) < density
    if one_direction:
        b = np.triu(b, 1)
    idx = np.arange(n)
    b[idx, idx] = rng.random(n) < 0.01
    return trm.random_words(n, 12, rng), b


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", trm.HAND_BUILT)
def test_hand_built_round_form_equals_the_sequential_rule(host, name, n):
    words = trm.random_words(n, 13, np.random.default_rng(1000 + n))
    b = trm.hand_built(name, n)
    s, rank = trm.symmetrise(b), trm.lex_rank(words)
    for T in TUBES:
        want = trm.sequential(s, rank, T)
        got, _ = trm.rounds(s, rank, T)
        np.testing.assert_array_equal(got, want)
        trm.check_assignment(s, got, T)
        np.testing.assert_array_equal(host_tubes(host, words, b, T), want)


@pytest.mark.parametrize("n,density,one_direction", [(300, 0.03, False), (700, 0.01, True), (1200, 0.02, False),
                                                     (2000, 0.005, True)])
def test_random_graphs_round_form_equals_the_sequential_rule(host, n, density, one_direction):
    words, b = random_graph(n, density, 50 + n, one_direction)
    s, rank = trm.symmetrise(b), trm.lex_rank(words)
    for T in (1, 3, 8, 64):
        want = trm.sequential(s, rank, T)
        got, count = trm.rounds(s, rank, T)
        np.testing.assert_array_equal(got, want)
        trm.check_assignment(s, got, T)
        assert 0 < count <= n
    np.testing.assert_array_equal(host_tubes(host, words, b, 8), trm.sequential(s, rank, 8))


def test_hand_built_facts():
    words = trm.random_words(65, 13, np.random.default_rng(1065))
    rank = trm.lex_rank(words)
    # the 65-clique at 64 tubes: one node per round, the full mask at the last
    tube, count = trm.rounds(trm.symmetrise(trm.hand_built("clique", 65)), rank, 64)
    placed = tube[tube != trm.NONE]
    assert count == 65 and sorted(placed.tolist()) == list(range(64)) and int((tube == trm.NONE).sum()) == 1
    assert tube[int(np.argmin(rank))] == trm.NONE           # all degrees tie: the smallest oligo comes last
    for T in TUBES:
        tube, count = trm.rounds(trm.symmetrise(trm.hand_built("self_loop_only", 65)), rank, T)
        assert count == 1 and int((tube == trm.NONE).sum()) == 22 and set(tube[tube != trm.NONE].tolist()) == {0}
        for n in SIZES:
            w = trm.random_words(n, 13, np.random.default_rng(n))
            tube, count = trm.rounds(trm.symmetrise(trm.hand_built("empty", n)), trm.lex_rank(w), T)
            assert count == 1 and not tube.any()
    # a node that only conflicts with itself leaves nothing to decide
    tube, count = trm.rounds(np.ones((1, 1), dtype=bool), np.zeros(1, np.int64), 3)
    assert count == 0 and tube.tolist() == [trm.NONE]
    # star: the centre has the greatest degree and takes tube 0; one tube leaves every leaf out
    s = trm.symmetrise(trm.hand_built("star", 300))
    tube, count = trm.rounds(s, trm.lex_rank(trm.random_words(300, 13, np.random.default_rng(5))), 1)
    assert count == 2 and tube[0] == 0 and (tube[1:] == trm.NONE).all()


def test_random_graph_figures():
    """Density 0.005 at n = 2,000: the self loops are the only nodes 64 tubes leave out, and 8 tubes fill up."""
    words, b = random_graph(2000, 0.005, 7, False)
    s, rank = trm.symmetrise(b), trm.lex_rank(words)
    loops = int(np.diag(s).sum())
    t64, r64 = trm.rounds(s, rank, 64)
    t8, r8 = trm.rounds(s, rank, 8)
    assert r64 == r8                                         # the rounds depend on the keys alone
    assert int((t64 == trm.NONE).sum()) == loops
    assert int(t64[t64 != trm.NONE].max()) + 1 > 8
    assert int(t8[t8 != trm.NONE].max()) + 1 == 8 and int((t8 == trm.NONE).sum()) > loops


def test_vectorised_round_form_at_4160():
    words, b = random_graph(4160, 8 / 4160, 11, True)
    s, rank = trm.symmetrise(b), trm.lex_rank(words)
    tube, count = trm.rounds(s, rank, 3)
    trm.check_assignment(s, tube, 3)
    assert count > 1
