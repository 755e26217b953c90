"""msspe_conflict_graph* on the MI355X: the conflict graph under a pair of rules (thal ANY decided on dG, thal END1
decided on t), its row counts, kind counts and ordered edge list, against the CPU model (tests/conflict_graph_model.py,
built on the oracle); the single-rule forms against the two existing screens bit for bit; the rule forms of the graph
consumers against their _dev / bitmap forms fed the model's union bitmap."""
import ctypes as C

import numpy as np
import pytest

import conflict_graph_model as M

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A5A5A5A5A
GUARD = 64
CASES = [p[0] + ("ntthal",) for p in M.POOL_RULES] + [(13, 160, -12000.0, 25.0, "primer3")]


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


def chem_of(m, name):
    return m.Chem.ntthal() if name == "ntthal" else m.Chem.primer3()


def dev_words(m, words):
    import torch
    return torch.from_numpy(m.pack_oligos(words).view(np.int64)).cuda()


class Out:
    """Device outputs of one block, each pre-filled and with guard words around it."""

    def __init__(self, n_rows_total, rows, cols, capacity):
        import torch
        self.nr, self.words = rows[1] - rows[0], (cols[1] - cols[0] + 63) // 64
        self.cap = capacity
        self.bm = torch.full((2 * GUARD + self.nr * self.words,), FILL, dtype=torch.int64, device="cuda")
        self.rc = torch.full((n_rows_total + GUARD,), 5, dtype=torch.int32, device="cuda")
        self.kinds = torch.tensor([3, 4, 5, 77], dtype=torch.int64, device="cuda")
        self.edges = torch.full((2 * (capacity + GUARD),), FILL, dtype=torch.int64, device="cuda")   # 16-byte records
        self.count = torch.tensor([123, 77], dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def bm_ptr(self):
        return self.bm.data_ptr() + 8 * GUARD

    def read(self):
        bm = self.bm.cpu().numpy().view(np.uint64)
        assert (bm[:GUARD] == FILL).all() and (bm[len(bm) - GUARD:] == FILL).all()      # words around the block survive
        rc = self.rc.cpu().numpy()
        kinds = self.kinds.cpu().numpy()
        assert kinds[3] == 77
        count = self.count.cpu().numpy()
        assert count[1] == 77
        raw = self.edges.cpu().numpy().view(np.uint64)
        have = min(int(count[0]), self.cap)
        assert (raw[2 * have:] == FILL).all()                                           # nothing behind the list
        return {"bitmap": bm[GUARD:len(bm) - GUARD].reshape(self.nr, self.words), "row_conflicts": rc,
                "kind_counts": kinds[:3].astype(np.uint64) - np.array([3, 4, 5], dtype=np.uint64),
                "edges": raw[:2 * have].view(M.KIND_EDGE).copy(), "count": int(count[0])}


def graph_block(m, eng, d_pool, n, k, chem, rule, rows, cols, capacity=4096):
    """The block through msspe_conflict_graph_dev and again through msspe_conflict_graph_edges_dev (every output asked
    for both times): the two agree; returns the second."""
    a, b = Out(n, rows, cols, 0), Out(n, rows, cols, capacity)
    eng.conflict_graph_dev(d_pool.data_ptr(), n, k, chem, rule, rows, cols, a.rc.data_ptr(), a.bm_ptr(),
                           a.kinds.data_ptr())
    eng.conflict_graph_edges_dev(d_pool.data_ptr(), n, k, chem, rule, rows, cols, b.edges.data_ptr(), capacity,
                                 b.count.data_ptr(), b.rc.data_ptr(), b.bm_ptr(), b.kinds.data_ptr())
    eng.synchronize()
    ra, rb = a.read(), b.read()
    for f in ("bitmap", "row_conflicts", "kind_counts"):
        np.testing.assert_array_equal(ra[f], rb[f], f)
    assert ra["count"] == 123            # the form without edges has no count to write
    return rb


def check_block(got, any_cf, end_cf, n, rows, cols):
    """Outputs of a block against the model's planes of the whole pool."""
    a, e = M.block(any_cf, rows, cols), M.block(end_cf, rows, cols)
    np.testing.assert_array_equal(got["bitmap"], M.pack_bits(M.union(a, e)))            # padding bits clear
    want_rc = np.full(n + GUARD, 5, dtype=np.int64)
    want_rc[rows[0]:rows[1]] += M.row_counts(a, e)
    np.testing.assert_array_equal(got["row_conflicts"], want_rc)                        # += onto a non-zero start
    np.testing.assert_array_equal(got["kind_counts"], M.kind_counts(a, e))
    want_edges = M.kind_edges(a, e, rows[0], cols[0])
    assert got["count"] == len(want_edges)
    np.testing.assert_array_equal(got["edges"], want_edges[:len(got["edges"])])


# ---- 1. the shared pools under both rules ----------------------------------------------------------------------------
@pytest.mark.parametrize("k,n,dg,tm,chem_name", CASES)
def test_pools_equal_the_model(m, eng, k, n, dg, tm, chem_name):
    pool, any_cf, end_cf = M.square_planes(k, n, dg, tm, chem_name)
    chem, rule = chem_of(m, chem_name), m.ConflictRule.of(dg, tm)
    got = graph_block(m, eng, dev_words(m, pool), n, k, chem, rule, (0, n), (0, n))
    check_block(got, any_cf, end_cf, n, (0, n), (0, n))
    assert all(x > 0 for x in got["kind_counts"])
    # the host forms: outputs assigned
    host = eng.conflict_graph(pool, chem, rule)
    np.testing.assert_array_equal(host["bitmap"], got["bitmap"])
    np.testing.assert_array_equal(host["row_conflicts"], M.row_counts(any_cf, end_cf))
    np.testing.assert_array_equal(host["kind_counts"], M.kind_counts(any_cf, end_cf))
    edges, count = eng.conflict_graph_edges(pool, chem, rule)
    assert count == len(edges)
    np.testing.assert_array_equal(edges, M.kind_edges(any_cf, end_cf))


# ---- 2. one rule: the existing screens, bit for bit ------------------------------------------------------------------
def single_rule_case(m, eng, pair_bound):
    import torch
    k, n, dg, tm = 13, 160, -9000.0, 10.0
    pool, any_cf, end_cf = M.square_planes(k, n, dg, tm)
    chem = m.Chem.ntthal()
    d_pool = dev_words(m, pool)
    rows, cols = (3, 150), (0, n)
    eng.set_option("pair_bound", pair_bound)
    try:
        for rule, screen, thr, plane in ((m.ConflictRule.of(dg, None), eng.cross_dimer_dev, dg, any_cf),
                                         (m.ConflictRule.of(None, tm), eng.cross_dimer_end_dev, tm, end_cf)):
            ref = Out(n, rows, cols, 0)
            screen(d_pool.data_ptr(), n, k, chem, thr, rows, cols, ref.rc.data_ptr(), ref.bm_ptr())
            eng.synchronize()
            want = ref.read()
            got = Out(n, rows, cols, 0)
            eng.conflict_graph_dev(d_pool.data_ptr(), n, k, chem, rule, rows, cols, got.rc.data_ptr(), got.bm_ptr(),
                                   got.kinds.data_ptr())
            eng.synchronize()
            assert torch.equal(got.bm, ref.bm) and torch.equal(got.rc, ref.rc)          # whole buffers, guards included
            res = got.read()
            z = np.zeros_like(plane)
            pa, pe = (plane, z) if rule.use_any else (z, plane)
            np.testing.assert_array_equal(res["kind_counts"], M.kind_counts(M.block(pa, rows, cols), M.block(pe, rows, cols)))
            np.testing.assert_array_equal(M.unpack_bits(want["bitmap"], n), M.block(plane, rows, cols))
            # the same rule through the planes of the scratch (the edge form): the same outputs, and the edges
            check_block(graph_block(m, eng, d_pool, n, k, chem, rule, rows, cols), pa, pe, n, rows, cols)
    finally:
        eng.set_option("pair_bound", "auto")


def test_single_rule_forms_are_the_existing_screens(m, eng):
    single_rule_case(m, eng, "auto")


def test_single_rule_forms_without_the_bound_stage(m, eng):
    single_rule_case(m, eng, 0)


def test_any_rule_takes_the_mirrored_bound_route(m, eng):
    """use_any alone on a square block is msspe_cross_dimer_dev's own path: the bound first stage mirrors."""
    pool = m.synth.pool_strings(m.synth.random_pool(2048, 13))
    d_pool = dev_words(m, pool)
    chem, n = m.Chem.ntthal(), len(pool)
    outs = []
    for call in ("screen", "graph"):
        o = Out(n, (0, n), (0, n), 0)
        eng.set_option("pair_bound", 1)
        try:
            eng.info("bound_mirrored")
            if call == "screen":
                eng.cross_dimer_dev(d_pool.data_ptr(), n, 13, chem, -9000.0, (0, n), (0, n), o.rc.data_ptr(), o.bm_ptr())
            else:
                eng.conflict_graph_dev(d_pool.data_ptr(), n, 13, chem, m.ConflictRule.of(-9000.0, None), (0, n), (0, n),
                                       o.rc.data_ptr(), o.bm_ptr())
            eng.synchronize()
            outs.append((o.read(), eng.info("bound_mirrored")))
        finally:
            eng.set_option("pair_bound", "auto")
    np.testing.assert_array_equal(outs[0][0]["bitmap"], outs[1][0]["bitmap"])
    np.testing.assert_array_equal(outs[0][0]["row_conflicts"], outs[1][0]["row_conflicts"])
    assert outs[0][1] == outs[1][1] > 0


# ---- 3. word and block geometry --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_pool_sizes_around_a_word(m, eng, n):
    pool, any_cf, end_cf = M.square_planes(13, 160, -9000.0, 10.0)
    got = graph_block(m, eng, dev_words(m, pool[:n]), n, 13, m.Chem.ntthal(), m.ConflictRule.of(-9000.0, 10.0), (0, n),
                      (0, n))
    check_block(got, any_cf[:n, :n], end_cf[:n, :n], n, (0, n), (0, n))


def test_sub_block_overwrites_inside_and_keeps_outside(m, eng):
    pool, any_cf, end_cf = M.square_planes(13, 160, -9000.0, 10.0)
    rows, cols = (37, 101), (5, 133)
    got = graph_block(m, eng, dev_words(m, pool), 160, 13, m.Chem.ntthal(), m.ConflictRule.of(-9000.0, 10.0), rows, cols)
    check_block(got, any_cf, end_cf, 160, rows, cols)          # the pattern inside is gone, Out.read checked outside
    assert got["count"] > 0 and (got["edges"]["a"] >= 37).all() and (got["edges"]["b"] >= 5).all()


# ---- 4. rows per block of the scratch planes -------------------------------------------------------------------------
def test_block_rows_never_change_the_outputs(m, eng):
    pool, any_cf, end_cf = M.square_planes(13, 160, -9000.0, 10.0)
    d_pool = dev_words(m, pool)
    res = {}
    try:
        for br in (1, 7, 64, 0):                   # 7 leaves a partial last block
            eng.set_option("conflict_graph_block_rows", br)
            res[br] = graph_block(m, eng, d_pool, 160, 13, m.Chem.ntthal(), m.ConflictRule.of(-9000.0, 10.0), (0, 160),
                                  (0, 160))
            check_block(res[br], any_cf, end_cf, 160, (0, 160), (0, 160))
        grown = eng.info("conflict_graph_grows")
        res["again"] = graph_block(m, eng, d_pool, 160, 13, m.Chem.ntthal(), m.ConflictRule.of(-9000.0, 10.0), (0, 160),
                                   (0, 160))
        assert eng.info("conflict_graph_grows") == grown      # the scratch has the call's size: no further allocation
    finally:
        eng.set_option("conflict_graph_block_rows", 0)
    for br in (1, 7, 64, "again"):
        for f in ("bitmap", "row_conflicts", "kind_counts", "edges"):
            np.testing.assert_array_equal(res[br][f], res[0][f], f"{br} {f}")
    with pytest.raises(m.MsspeError):
        eng.set_option("conflict_graph_block_rows", -1)


# ---- 5. pool A against pool B ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ab_pools():
    P13, P20 = M.end_pool(13, 48, 8), M.end_pool(20, 40, 9)
    for j in range(10):                        # oligos that pair with the other pool's 3' ends, in both directions
        P20[j] = (M.rc(P13[j][-13:]) + P20[j])[:20]
        P13[20 + j] = (M.rc(P20[20 + j][-10:]) + P13[20 + j])[:13]
    return P13, P20


@pytest.fixture(scope="module")
def ab_planes(ab_pools, oracle, oracle_tables):
    P13, P20 = ab_pools
    return {(13, 20): M.ab_planes(oracle, oracle_tables, P13, P20, -9000.0, 10.0),
            (20, 13): M.ab_planes(oracle, oracle_tables, P20, P13, -9000.0, 10.0)}


@pytest.mark.parametrize("k_a,k_b", [(13, 20), (20, 13)])
def test_ab_equals_per_pair_oracle_calls(m, eng, ab_pools, ab_planes, k_a, k_b):
    A, B = ab_pools if k_a == 13 else ab_pools[::-1]
    any_cf, end_cf = ab_planes[(k_a, k_b)]
    assert all(x > 0 for x in M.kind_counts(any_cf, end_cf))
    chem, rule = m.Chem.ntthal(), m.ConflictRule.of(-9000.0, 10.0)
    n_a, n_b = len(A), len(B)
    d_a, d_b = dev_words(m, A), dev_words(m, B)
    for rows, cols in (((0, n_a), (0, n_b)), ((3, n_a - 2), (1, n_b - 3))):
        a, b = Out(n_a, rows, cols, 0), Out(n_a, rows, cols, 4096)
        eng.conflict_graph_ab_dev(d_a.data_ptr(), n_a, k_a, d_b.data_ptr(), n_b, k_b, chem, rule, rows, cols,
                                  a.rc.data_ptr(), a.bm_ptr(), a.kinds.data_ptr())
        eng.conflict_graph_ab_edges_dev(d_a.data_ptr(), n_a, k_a, d_b.data_ptr(), n_b, k_b, chem, rule, rows, cols,
                                        b.edges.data_ptr(), 4096, b.count.data_ptr(), b.rc.data_ptr(), b.bm_ptr(),
                                        b.kinds.data_ptr())
        eng.synchronize()
        ra, rb = a.read(), b.read()
        np.testing.assert_array_equal(ra["bitmap"], rb["bitmap"])
        for got in (ra, rb):
            got["edges"], got["count"] = rb["edges"], rb["count"]
            check_block(got, any_cf, end_cf, n_a, rows, cols)
    edges, count = eng.conflict_graph_ab_edges(A, B, chem, rule)
    np.testing.assert_array_equal(edges, M.kind_edges(any_cf, end_cf))
    assert count == len(edges)


def test_swapping_the_pools_swaps_the_3p_end(ab_planes):
    """END of (A, B) anchors A's 3' end, END of (B, A) anchors B's: the two planes are not each other's transpose."""
    e_ab, e_ba = ab_planes[(13, 20)][1], ab_planes[(20, 13)][1]
    assert (e_ab != e_ba.T).any()


# ---- 6. the edge list's capacity -------------------------------------------------------------------------------------
def test_edge_capacity(m, eng):
    k, n, dg, tm = 13, 160, -12000.0, 25.0
    pool, any_cf, end_cf = M.square_planes(k, n, dg, tm)
    want = M.kind_edges(any_cf, end_cf)
    need = len(want)
    chem, rule = m.Chem.ntthal(), m.ConflictRule.of(dg, tm)
    d_pool = dev_words(m, pool)
    for cap in (0, need - 1, need):
        o = Out(n, (0, n), (0, n), cap)
        eng.conflict_graph_edges_dev(d_pool.data_ptr(), n, k, chem, rule, (0, n), (0, n),
                                     o.edges.data_ptr() if cap else 0, cap, o.count.data_ptr())
        eng.synchronize()
        got = o.read()                               # checks the guard words behind the first `cap` records
        assert got["count"] == need
        np.testing.assert_array_equal(got["edges"], want[:cap])
        if cap < need:
            with pytest.raises(m.MsspeError) as ei:
                eng.conflict_graph_edges(pool, chem, rule, capacity=cap)
            assert ei.value.code == 5 and ei.value.count == need
            np.testing.assert_array_equal(ei.value.edges[:cap], want[:cap])
            with pytest.raises(m.MsspeError) as ei:
                eng.conflict_graph_ab_edges(pool, pool, chem, rule, capacity=cap)
            assert ei.value.code == 5 and ei.value.count == need
        else:
            edges, count = eng.conflict_graph_edges(pool, chem, rule, capacity=cap)
            assert count == need
            np.testing.assert_array_equal(edges, want)
            edges, count = eng.conflict_graph_ab_edges(pool, pool, chem, rule, capacity=cap)   # A = B: the same pairs
            np.testing.assert_array_equal(edges, want)


# ---- 7. a larger pool against the two existing screens ---------------------------------------------------------------
def test_3000_random_13mers_equal_the_or_of_the_two_screens(m, eng):
    n, k, dg, tm = 3000, 13, -9000.0, 10.0
    pool = m.synth.pool_strings(m.synth.random_pool(n, k))
    chem, rule = m.Chem.ntthal(), m.ConflictRule.of(dg, tm)
    any_cf = M.unpack_bits(eng.cross_dimer(pool, chem, dg, want_dg=False)["bitmap"], n)
    end_cf = M.unpack_bits(eng.cross_dimer_end(pool, chem, tm, want_dg=False, want_tm=False)["bitmap"], n)
    want = M.kind_edges(any_cf, end_cf)
    assert all(x > 0 for x in M.kind_counts(any_cf, end_cf))
    cap = len(want) + 10
    d_pool = dev_words(m, pool)
    res = {}
    try:
        for br in (0, 701):
            eng.set_option("conflict_graph_block_rows", br)
            o = Out(n, (0, n), (0, n), cap)
            eng.conflict_graph_edges_dev(d_pool.data_ptr(), n, k, chem, rule, (0, n), (0, n), o.edges.data_ptr(), cap,
                                         o.count.data_ptr(), o.rc.data_ptr(), o.bm_ptr(), o.kinds.data_ptr())
            eng.synchronize()
            res[br] = o.read()
            check_block(res[br], any_cf, end_cf, n, (0, n), (0, n))
    finally:
        eng.set_option("conflict_graph_block_rows", 0)


# ---- 8. the rule forms of the consumers ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def consumer_case(m):
    k, n, dg, tm = 13, 160, -12000.0, 25.0
    pool, any_cf, end_cf = M.square_planes(k, n, dg, tm)
    end_only = end_cf.astype(bool) & ~any_cf.astype(bool)
    assert np.diag(end_only).sum() == 2          # the self-conflict path differs from the ANY-only run
    return pool, M.pack_bits(M.union(any_cf, end_cf)), dg, tm


@pytest.mark.parametrize("drop", [0, 1])
def test_cover_rule_form(m, eng, consumer_case, drop):
    import torch
    pool, bits, dg, tm = consumer_case
    n, chem = len(pool), m.Chem.ntthal()
    d_pool = dev_words(m, pool)
    d_bm = torch.from_numpy(bits.view(np.int64).copy()).cuda()
    d_del = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.conflict_cover_dev(d_pool.data_ptr(), n, 13, d_bm.data_ptr(), d_del.data_ptr(), drop_self_pairs=bool(drop))
    want = d_del.cpu().numpy().astype(bool)
    got = eng.conflict_cover(pool, chem, dg, drop_self_pairs=bool(drop), end_tm_threshold=tm)
    np.testing.assert_array_equal(got, want)
    any_only = eng.conflict_cover(pool, chem, dg, drop_self_pairs=bool(drop))
    assert (got != any_only).any()               # without the END rule the test would pass on the old call


@pytest.mark.parametrize("drop", [0, 1])
def test_tubes_rule_form(m, eng, consumer_case, drop):
    import torch
    pool, bits, dg, tm = consumer_case
    n, chem = len(pool), m.Chem.ntthal()
    d_pool = dev_words(m, pool)
    d_bm = torch.from_numpy(bits.view(np.int64).copy()).cuda()
    for T in (1, 3):
        d_tube = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        used, unplaced = eng.conflict_tubes_dev(d_pool.data_ptr(), n, 13, d_bm.data_ptr(), d_tube.data_ptr(), T,
                                                drop_self_pairs=bool(drop))
        got = eng.conflict_tubes(pool, chem, dg, T, drop_self_pairs=bool(drop), end_tm_threshold=tm)
        np.testing.assert_array_equal(got[0], d_tube.cpu().numpy())
        assert got[1:] == (used, unplaced)
        any_only = eng.conflict_tubes(pool, chem, dg, T, drop_self_pairs=bool(drop))
        assert (got[0] != any_only[0]).any()
    if not drop:                                 # the two END-only diagonal bits: two more oligos in no tube
        assert got[2] >= 2


def planted_alignment(fwd, rev):
    """8 genomes of 20 segments (400 long, stride 170): each segment starts with a forward primer and ends with the
    reverse complement of a reverse primer, so every primer of the pool covers two segments."""
    rng = np.random.default_rng(31)
    n_seq, P = 8, 20
    L = 170 * (P - 1) + 400
    g = rng.integers(0, 4, (n_seq, L))
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[g].copy()
    for r in range(n_seq):
        for p in range(P):
            j = r * P + p
            f, v = fwd[j % len(fwd)], M.rc(rev[j % len(rev)])
            g[r, p * 170 + 5:p * 170 + 5 + 13] = np.frombuffer(f.encode(), dtype=np.uint8)
            at = p * 170 + 400 - 13 - 5
            g[r, at:at + 13] = np.frombuffer(v.encode(), dtype=np.uint8)
    return g


@pytest.mark.parametrize("drop", [0, 1])
def test_panel_select_rule_form(m, eng, consumer_case, drop):
    pool, bits, dg, tm = consumer_case
    fwd, rev = pool[:80], pool[80:]
    g = planted_alignment(fwd, rev)
    opt, chem = m.KmerOpt(400, 170, 50, 13, 0, 0), m.Chem.ntthal()
    keys = ("order", "gains", "keep", "tube", "barred", "covered", "covered_all", "covered_kept", "tubes_used")
    for T in (1, 2):
        want = eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), bits, T, drop_self_pairs=bool(drop), form="packed")
        got = eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), None, T, drop_self_pairs=bool(drop), form="screen",
                               chem=chem, threshold=dg, end_tm_threshold=tm)
        for key in keys:
            np.testing.assert_array_equal(got[key], want[key], key)
        assert len(got["order"]) > 20
        any_only = eng.panel_select(g, opt, fwd, rev, m.seed_rule(2, 3), None, T, drop_self_pairs=bool(drop),
                                    form="screen", chem=chem, threshold=dg)
        assert any((np.asarray(got[key]).shape != np.asarray(any_only[key]).shape) or
                   (np.asarray(got[key]) != np.asarray(any_only[key])).any() for key in ("order", "keep", "tube", "barred"))


# ---- 9. argument errors ----------------------------------------------------------------------------------------------
def test_argument_errors(m, eng):
    import torch
    chem, L = m.Chem.ntthal(), eng.L
    both, none = m.ConflictRule.of(-9000.0, 10.0), m.ConflictRule(0, -9000.0, 0, 10.0)
    d_pool = torch.zeros(8, dtype=torch.int64, device="cuda")
    d_bm = torch.full((8,), FILL, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    p = d_pool.data_ptr()

    def dev(n=8, k=13, rows=(0, 8), cols=(0, 8), chem_ref=C.byref(chem), rule_ref=C.byref(both), pool=p, bm=None):
        return L.msspe_conflict_graph_dev(eng.ptr, pool, n, k, chem_ref, rule_ref, rows[0], rows[1], cols[0], cols[1],
                                          None, bm, None)

    assert dev(rule_ref=None) == 1 and dev(chem_ref=None) == 1 and dev(rule_ref=C.byref(none)) == 1
    assert dev(k=1) == 2 and dev(k=33) == 2
    assert dev(rows=(5, 3)) == 1 and dev(cols=(0, 9)) == 1 and dev(rows=(-1, 2)) == 1
    assert dev(pool=None) == 1
    assert dev(n=0, rows=(0, 0), cols=(0, 0), bm=d_bm.data_ptr()) == 0
    assert dev(rows=(3, 3), bm=d_bm.data_ptr()) == 0 and dev(cols=(8, 8), bm=d_bm.data_ptr()) == 0
    eng.synchronize()
    assert (d_bm.cpu().numpy().view(np.uint64) == FILL).all()      # n == 0, empty blocks: nothing written
    ab = (eng.ptr, p, 8, 13, p, 8)
    assert L.msspe_conflict_graph_ab_dev(*ab, 33, C.byref(chem), C.byref(both), 0, 8, 0, 8, None, None, None) == 2
    assert L.msspe_conflict_graph_ab_dev(*ab, 20, None, C.byref(both), 0, 8, 0, 8, None, None, None) == 1
    assert L.msspe_conflict_graph_ab_dev(*ab, 20, C.byref(chem), C.byref(none), 0, 8, 0, 8, None, None, None) == 1
    assert L.msspe_conflict_graph_ab_dev(*ab, 20, C.byref(chem), C.byref(both), 0, 9, 0, 8, None, None, None) == 1
    edges_args = (eng.ptr, p, 8, 13, C.byref(chem), C.byref(both), 0, 8, 0, 8, None, None, None)
    assert L.msspe_conflict_graph_edges_dev(*edges_args, None, 0, None) == 1              # no count
    assert L.msspe_conflict_graph_edges_dev(*edges_args, None, 4, d_cnt.data_ptr()) == 1  # a capacity without a buffer
    eng.synchronize()
    assert int(d_cnt.item()) == 9
    with pytest.raises(m.MsspeError) as ei:
        eng.conflict_graph(["ACGTNACGTACGT"] * 2, chem, both)
    assert ei.value.code == 1
    with pytest.raises(m.MsspeError) as ei:
        eng.conflict_graph_ab_edges(["ACGTACGTACGTA"], ["ACGTACGTAXGTA"], chem, both)
    assert ei.value.code == 1
    with pytest.raises(m.MsspeError) as ei:
        eng.conflict_graph_edges(["ACGTACGTACGTA"], chem, none)
    assert ei.value.code == 1
    assert eng.conflict_graph_edges([], chem, both)[1] == 0
    pool = b"ACGTACGTACGTA" + b"CCGTACGTACGTA"
    out = np.zeros(2, dtype=np.uint8)
    assert L.msspe_conflict_cover_rule(eng.ptr, pool, 2, 13, C.byref(chem), C.byref(none), 0, out.ctypes.data, None) == 1
    assert L.msspe_conflict_cover_rule(eng.ptr, pool, 2, 13, C.byref(chem), None, 0, out.ctypes.data, None) == 1
    assert L.msspe_conflict_tubes_rule(eng.ptr, pool, 2, 13, C.byref(chem), C.byref(none), 0, 2, out.ctypes.data, None,
                                       None) == 1
    assert L.msspe_conflict_cover_rule(eng.ptr, pool, 2, 13, C.byref(chem), C.byref(both), 0, out.ctypes.data, None) == 0
