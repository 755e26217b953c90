"""The conflict-graph model (tests/conflict_graph_model.py) on the pools the GPU tests share: its pieces agree with
each other and with the oracle's own ANY decision, and every pool really holds what the GPU tests need -- all three
kinds and an END-only pair whose transpose is not set.  No GPU."""
import numpy as np
import pytest

import conflict_graph_model as M


@pytest.fixture(scope="module", params=M.POOL_RULES, ids=lambda p: "k%d-n%d-dg%g-tm%g" % p[0])
def case(request):
    (k, n, dg, tm), want = request.param
    pool, a, e = M.square_planes(k, n, dg, tm)
    return pool, a, e, want, (k, n, dg, tm)


def test_pool_is_distinct_and_of_one_length(case):
    pool, _, _, _, (k, n, _, _) = case
    assert len(pool) == n == len(set(pool)) and {len(s) for s in pool} == {k}
    assert M.distinct(["ACG", "ACG", "CCG", "ACG"]) == ["ACG", "CCG", "GCG", "TCG"]


def test_any_plane_is_the_oracles_decision(case, oracle, oracle_tables):
    pool, a, _, _, (_, _, dg, _) = case
    _, _, cf, _ = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(), dg)
    np.testing.assert_array_equal(a, cf)


def test_pool_holds_all_three_kinds_and_an_asymmetric_end_only_pair(case):
    """A pool without them tests nothing: the recorded counts keep a later edit of the pools honest."""
    _, a, e, want, _ = case
    kc = M.kind_counts(a, e)
    assert tuple(int(x) for x in kc) == want and all(x > 0 for x in want)
    end_only = e.astype(bool) & ~a.astype(bool)
    assert (end_only & ~M.union(a, e).T.astype(bool)).any()


def test_recorded_diagonal_and_asymmetric_counts():
    _, a, e = M.square_planes(13, 160, -12000.0, 25.0)
    end_only = e.astype(bool) & ~a.astype(bool)
    assert int(np.diag(end_only).sum()) == 2 and int(a.sum()) == 22 and int(e.sum()) == 46
    _, a, e = M.square_planes(13, 160, -9000.0, 10.0)
    end_only = e.astype(bool) & ~a.astype(bool)
    assert int((end_only & ~M.union(a, e).T.astype(bool)).sum()) == 124


def test_union_counts_and_edges_agree(case):
    _, a, e, _, (_, n, _, _) = case
    u = M.union(a, e)
    rc = M.row_counts(a, e)
    kc = M.kind_counts(a, e)
    ed = M.kind_edges(a, e)
    assert rc.sum() == u.sum() == kc.sum() == len(ed)
    assert rc.sum() == a.sum() + e.sum() - kc[2]                 # a pair under both rules counts once
    key = ed["a"].astype(np.int64) * n + ed["b"]
    assert (np.diff(key) > 0).all() and (ed["reserved"] == 0).all()
    np.testing.assert_array_equal(np.bincount(ed["a"], minlength=n).astype(np.uint32), rc)
    np.testing.assert_array_equal(u[ed["a"], ed["b"]], 1)
    np.testing.assert_array_equal((ed["kinds"] & M.KIND_ANY) != 0, a[ed["a"], ed["b"]] != 0)
    np.testing.assert_array_equal((ed["kinds"] & M.KIND_END) != 0, e[ed["a"], ed["b"]] != 0)
    for j, kinds in enumerate((M.KIND_ANY, M.KIND_END, M.KIND_ANY | M.KIND_END)):
        assert (ed["kinds"] == kinds).sum() == kc[j]
    np.testing.assert_array_equal(M.unpack_bits(M.pack_bits(u), n), u)
    assert M.pack_bits(u).shape == (n, (n + 63) // 64)


def test_single_rule_forms_are_the_planes(case):
    _, a, e, _, _ = case
    a1, e1 = M.enabled(a, e, use_end=False)
    np.testing.assert_array_equal(M.union(a1, e1), a)
    assert tuple(M.kind_counts(a1, e1)) == (a.sum(), 0, 0)
    a2, e2 = M.enabled(a, e, use_any=False)
    np.testing.assert_array_equal(M.union(a2, e2), e)
    assert tuple(M.kind_counts(a2, e2)) == (0, e.sum(), 0)


@pytest.mark.parametrize("block_rows", [1, 7, 64, 1000])
def test_row_blocks_give_the_one_piece_result(case, block_rows):
    _, a, e, _, _ = case
    edges, counts = M.by_blocks(a, e, block_rows)
    np.testing.assert_array_equal(edges, M.kind_edges(a, e))
    np.testing.assert_array_equal(counts, M.row_counts(a, e))


def test_sub_block_edges_carry_pool_indices(case):
    _, a, e, _, (_, n, _, _) = case
    rows, cols = (n // 4, n // 4 * 3), (5, n - 20)
    ed = M.kind_edges(M.block(a, rows, cols), M.block(e, rows, cols), rows[0], cols[0])
    full = M.kind_edges(a, e)
    keep = (full["a"] >= rows[0]) & (full["a"] < rows[1]) & (full["b"] >= cols[0]) & (full["b"] < cols[1])
    np.testing.assert_array_equal(ed, full[keep])
