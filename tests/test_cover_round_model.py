"""The round form of the greedy vertex cover (tests/cover_round_model.py, what csrc/conflict_cover.hip computes) equals
the reference's sequential rule (oracle/ref_pipeline.py:vertex_cover, and the host's odm_vertex_cover for the larger
graphs) on hand-built and random graphs: self loops, edges in one direction only, all-tie regular graphs, isolated
nodes.  No GPU needed."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import cover_round_model as crm

ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"


@pytest.fixture(scope="module")
def host():
    import msspe_amd
    msspe_amd.load_library()              # libod_msspe_host.so depends on libmsspe_hip.so
    return C.CDLL(str(HOST_LIB))


def edges_of(b, words):
    a, c = np.nonzero(b)
    return {(words[i], words[j]) for i, j in zip(a.tolist(), c.tolist())}


def model_set(b, words):
    deleted, rounds = crm.round_cover(crm.symmetrise(b), crm.lex_rank(words))
    return {words[i] for i in np.nonzero(deleted)[0]}, rounds


def host_cover(host, words, edges):
    cap = 1 << 24
    buf = C.create_string_buffer(cap)
    rc = host.odm_vertex_cover("\n".join(words).encode(), "\n".join(f"{a},{b}" for a, b in edges).encode(), buf, cap)
    assert rc >= 0
    return set(buf.value.decode().split())


@pytest.mark.parametrize("name", crm.HAND_BUILT)
@pytest.mark.parametrize("n", [1, 2, 7, 63, 64, 65])
def test_hand_built_graphs_equal_the_sequential_rule(name, n):
    import ref_pipeline
    words = crm.random_words(n, 9, np.random.default_rng(n))
    b = crm.hand_built(name, n)
    got, _ = model_set(b, words)
    assert got == ref_pipeline.vertex_cover(words, edges_of(b, words))


def test_round_counts_of_simple_shapes():
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 1000):
        words = crm.random_words(n, 13, rng)
        rounds = {name: model_set(crm.hand_built(name, n), words)[1] for name in crm.HAND_BUILT}
        assert rounds["empty"] == 0
        assert rounds["star"] == (1 if n > 1 else 0)
        assert rounds["clique"] == max(n - 1, 0)        # one node per round: the greatest string of the rest
        assert rounds["all_ties"] == (1 if n > 1 else 0)   # every pair settled at once by the lexicographic tie-break
        assert rounds["self_loop_only"] == 1             # node 0 has a self loop at every n


@pytest.mark.parametrize("seed", range(6))
def test_random_graphs_small_equal_the_reference(seed):
    """Random directed graphs with self loops and asymmetric pairs against oracle/ref_pipeline.py."""
    import ref_pipeline
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(5, 60))
    words = crm.random_words(n, 6, rng)
    b = rng.random((n, n)) < rng.uniform(0.02, 0.3)
    got, _ = model_set(b, words)
    assert got == ref_pipeline.vertex_cover(words, edges_of(b, words))


@pytest.mark.parametrize("n,mean_deg,self_loops", [(1500, 11, True), (2000, 15, False), (2000, 27, True),
                                                    (4000, 16, False)])
def test_random_skewed_graphs_equal_the_host_cover(host, n, mean_deg, self_loops):
    """Skewed degrees (a Pareto weight per node, edge probability proportional to the product of the two weights),
    against the host's sequential cover (odm_vertex_cover, the same rule as ref_pipeline.vertex_cover)."""
    rng = np.random.default_rng(n + mean_deg)
    words = crm.random_words(n, 12, rng)
    w = rng.pareto(1.5, n) + 1.0
    p = np.outer(w, w)
    p *= mean_deg / p.sum(1).mean()
    b = rng.random((n, n)) < np.minimum(p, 1.0) / 2     # directed: each order drawn on its own
    if not self_loops:
        np.fill_diagonal(b, False)
    got, rounds = model_set(b, words)
    assert got == host_cover(host, words, edges_of(b, words))
    assert 0 < rounds < len(got)
