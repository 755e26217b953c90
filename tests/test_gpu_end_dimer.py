"""The END screen (msspe_cross_dimer_end*: thal END1 for every ordered pair, od-msspe's SELF_END rule applied to a
pair) on the MI355X.  The CPU oracle is the checker: Primer3 2.6.1 thal type END1 per ordered pair
(pyoracle.pool_pairs / pyoracle.thal with mode END1), and the decision !(round_fixed_f32(max(0, t), 2) < thr) computed
here from the oracle's t.  dG and t are compared bit for bit."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


def rand_oligos(rng, n, k, alphabet="ACGT"):
    return ["".join(alphabet[x] for x in rng.integers(0, len(alphabet), k)) for _ in range(n)]


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def end_pool(k, n, seed):
    """Random oligos of length k with the shapes END1 cares about: self-complementary oligos (even k; pairs of two
    of them run the dense kernel), partners that pair with another oligo's 3' end, and pairs whose last DP row is
    empty (oligo 1 ends in A, the partner holds no T) with and without a base pair at cell (1, 1) (oligo 1's first
    base against the partner's last)."""
    rng = np.random.default_rng(seed * 100 + k)
    P = rand_oligos(rng, n, k)
    q = 0
    for j in range(0, min(16, n // 4)):          # 3'-complementary partners
        a = P[j]
        tail = a[-min(k, max(2, (3 * k) // 4)):]
        P[n // 2 + j] = (rc(tail) + P[n // 2 + j])[:k]
        q += 1
    if k % 2 == 0:                               # self-complementary oligos
        for j in range(6):
            h = rand_oligos(rng, 1, k // 2)[0]
            P[n // 4 + j] = h + rc(h)
    for j in range(4):                           # empty last row: oligo 1 = ...A, partners without T
        a = "C" + rand_oligos(rng, 1, k - 2, "ACG")[0] + "A" if k > 2 else "CA"
        with_bp = rand_oligos(rng, 1, k - 1, "ACG")[0] + "G"      # last base G pairs with a's first C
        without = rand_oligos(rng, 1, k - 1, "ACG")[0] + "A"
        P[n - 1 - 3 * j], P[n - 2 - 3 * j], P[n - 3 - 3 * j] = a, with_bp[-k:], without[-k:]
    return P


def t_end(t):
    return np.maximum(t, 0.0)


def end_rule(oracle, t, thr):
    """od-msspe's SELF_END rule on a pair: conflict iff !(round_fixed_f32(t_end, 2) < thr)."""
    thr32 = float(np.float32(thr))
    te = t_end(t)
    out = np.zeros(te.shape, dtype=np.uint8)
    for idx, v in np.ndenumerate(te):
        out[idx] = not oracle.round_fixed_f32(float(v), 2) < thr32
    return out


def oracle_square(oracle, tables, pool, args):
    _, dg, _, tt = oracle.pool_pairs(tables, pool, args, 0.0, mode=oracle.END1, want_t=True)
    return dg, tt


def oracle_ab(oracle, tables, A, B, args):
    dg = np.empty((len(A), len(B)))
    tt = np.empty((len(A), len(B)))

    def row(i):
        for j, b in enumerate(B):
            r = oracle.thal(tables, A[i], b, oracle.END1, args)
            dg[i, j] = np.inf if r.no_structure else r.dG
            tt[i, j] = 0.0 if r.no_structure else r.t

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(row, range(len(A))))
    return dg, tt


def bits(bitmap, ncols):
    return np.unpackbits(bitmap.view(np.uint8), axis=1, bitorder="little")[:, :ncols]


def check(oracle, out, dg, tt, thr):
    np.testing.assert_array_equal(out["dg"], dg)
    np.testing.assert_array_equal(out["tm"], tt)
    cf = end_rule(oracle, tt, thr)
    np.testing.assert_array_equal(bits(out["bitmap"], dg.shape[1]), cf)
    np.testing.assert_array_equal(out["row_conflicts"], cf.sum(1).astype(np.uint32))
    return cf


CHEMS = {"ntthal": (lambda m: m.Chem.ntthal(), lambda o: o.ntthal_args()),
         "primer3": (lambda m: m.Chem.primer3(), lambda o: o.p3_args())}


# ---- 1. 13-mers, 160^2, under both chemistries and three thresholds -------------------------------------------------
@pytest.mark.parametrize("chem_name", list(CHEMS))
def test_pool13_planes_and_decisions(m, eng, oracle, oracle_tables, chem_name):
    chem, args = CHEMS[chem_name][0](m), CHEMS[chem_name][1](oracle)
    pool = end_pool(13, 160, 1)
    dg, tt = oracle_square(oracle, oracle_tables, pool, args)
    te = t_end(tt)
    exact = float(np.float32(oracle.round_fixed_f32(float(np.sort(te[te > 0])[-40]), 2)))   # a pair sits on the edge
    for thr in (47.0, 10.0, exact):
        out = eng.cross_dimer_end(pool, chem, thr, want_dg=True, want_tm=True)
        cf = check(oracle, out, dg, tt, thr)
        if thr == exact:
            assert cf.sum() >= 40               # "<" against "<=": the pair at the threshold conflicts
        fast = eng.cross_dimer_end(pool, chem, thr, want_dg=False, want_tm=False)   # decisions only: same bits
        np.testing.assert_array_equal(fast["bitmap"], out["bitmap"])
        np.testing.assert_array_equal(fast["row_conflicts"], out["row_conflicts"])
    assert end_rule(oracle, tt, 10.0).sum() > 0


# ---- 2. every length ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 5, 10, 14, 16, 17, 20, 25, 32])
def test_lengths_match_the_oracle(m, eng, oracle, oracle_tables, k):
    n = 48 if k >= 25 else 96
    pool = end_pool(k, n, 2)
    dg, tt = oracle_square(oracle, oracle_tables, pool, oracle.ntthal_args())
    for thr in (10.0, 0.0):
        out = eng.cross_dimer_end(pool, m.Chem.ntthal(), thr, want_dg=True, want_tm=True)
        cf = check(oracle, out, dg, tt, thr)
        if thr == 0.0:
            assert cf.all()                      # tm_threshold <= 0: every pair conflicts
    assert np.isinf(dg).any() and np.isfinite(dg).any()


def test_small_max_loop_runs_the_wave_kernel_first(m, eng, oracle, oracle_tables):
    pool = end_pool(13, 128, 3)
    dg, tt = oracle_square(oracle, oracle_tables, pool, oracle.ntthal_args(max_loop=5))
    eng.profile_enable(True)
    out = eng.cross_dimer_end(pool, m.Chem.ntthal(max_loop=5), 10.0, want_dg=True, want_tm=True)
    launches, _ = eng.profile_read()
    eng.profile_enable(False)
    assert launches >= 1
    check(oracle, out, dg, tt, 10.0)


# ---- 3. every route gives the same results ---------------------------------------------------------------------------
def low_complexity_pool(k, n, seed):
    """Random oligos plus dinucleotide repeats: their pairs have large DP tables (the wide list, the wave list)."""
    rng = np.random.default_rng(seed)
    P = end_pool(k, n, seed)
    reps = ["AC", "GT", "CA", "TG", "AG", "CT", "AT", "TA", "GC", "CG"]
    for j in range(40):
        r = reps[j % len(reps)]
        s = (r * k)[:k] if j % 3 else ((r * k)[: k - 3] + rand_oligos(rng, 1, 3)[0])
        P[10 + j] = s
    return P


@pytest.mark.parametrize("k", [13, 20])
def test_every_route_gives_identical_results(m, eng, oracle, oracle_tables, k):
    pool = low_complexity_pool(k, 1200 if k == 13 else 400, 4)
    chem = m.Chem.ntthal()
    rows = np.random.default_rng(k).choice(len(pool), 12, replace=False)
    routes = {}
    try:
        for fg in (0, 1):
            for wk in (0, 1):
                for cap in (0, 20):
                    eng.set_option("force_generic", fg)
                    eng.set_option("wave_kernel", wk)
                    eng.set_option("list_cap_log2", cap)
                    eng.last_overflow_pairs()
                    eng.profile_enable(True)
                    out = eng.cross_dimer_end(pool, chem, 10.0, want_dg=True, want_tm=True)
                    launches, _ = eng.profile_read()
                    eng.profile_enable(False)
                    routes[(fg, wk, cap)] = (out, launches, eng.last_overflow_pairs())
    finally:
        eng.set_option("force_generic", 0)
        eng.set_option("wave_kernel", 1)
        eng.set_option("list_cap_log2", 0)
    base = routes[(1, 0, 0)][0]                      # the dense kernel over the whole block
    for key, (out, launches, handed) in routes.items():
        for f in ("dg", "tm", "bitmap", "row_conflicts"):
            np.testing.assert_array_equal(out[f], base[f], err_msg=f"{key} {f}")
        if key[0] == 1 or (k == 20 and key[1] == 0):
            assert launches == 0, key                # no first stage: the dense kernel took the block
        else:
            assert launches >= 1 and handed > 0, key   # a first stage ran and handed pairs on
    assert routes[(0, 1, 20)][1] > 1 or k == 20       # 1,440,000 pairs and 2^20-entry lists: several launches
    # the shared result against the oracle on a few rows
    for r in rows:
        _, dg, _, tt = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(), 0.0, mode=oracle.END1,
                                         rows=(int(r), int(r) + 1), want_t=True)
        np.testing.assert_array_equal(base["dg"][r], dg[0])
        np.testing.assert_array_equal(base["tm"][r], tt[0])


# ---- 4. sub-blocks, device entry points, edges -----------------------------------------------------------------------
def test_sub_blocks_clear_the_bitmap_and_accumulate_counts(m, eng, oracle, oracle_tables):
    import torch
    pool = end_pool(13, 300, 5)
    n = len(pool)
    _, tt = oracle_square(oracle, oracle_tables, pool, oracle.ntthal_args())
    cf = end_rule(oracle, tt, 10.0)
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    r0, r1, c0, c1 = 37, 211, 70, 263
    words = (c1 - c0 + 63) // 64
    d_bm = torch.full(((r1 - r0) * words,), -1, dtype=torch.int64, device="cuda")
    d_rc = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    d_tm = torch.empty((r1 - r0) * (c1 - c0), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    chem = m.Chem.ntthal()
    eng.cross_dimer_end_dev(d_pool.data_ptr(), n, 13, chem, 10.0, (r0, r1), (c0, c1), d_rc.data_ptr(),
                            d_bm.data_ptr(), 0, d_tm.data_ptr())
    eng.synchronize()
    bm = d_bm.cpu().numpy().view(np.uint64).reshape(r1 - r0, words)
    np.testing.assert_array_equal(bits(bm, c1 - c0), cf[r0:r1, c0:c1])
    want = np.full(n, 5, dtype=np.int64)
    want[r0:r1] += cf[r0:r1, c0:c1].sum(1).astype(np.int64)
    np.testing.assert_array_equal(d_rc.cpu().numpy(), want)
    np.testing.assert_array_equal(d_tm.cpu().numpy().reshape(r1 - r0, c1 - c0), tt[r0:r1, c0:c1])
    # decisions only: same bits; the counts accumulate again
    eng.cross_dimer_end_dev(d_pool.data_ptr(), n, 13, chem, 10.0, (r0, r1), (c0, c1), d_rc.data_ptr(),
                            d_bm.data_ptr())
    eng.synchronize()
    np.testing.assert_array_equal(bits(d_bm.cpu().numpy().view(np.uint64).reshape(r1 - r0, words), c1 - c0),
                                  cf[r0:r1, c0:c1])
    want[r0:r1] += cf[r0:r1, c0:c1].sum(1).astype(np.int64)
    np.testing.assert_array_equal(d_rc.cpu().numpy(), want)


def test_end2_by_transpose_and_pair_compl_end(m, eng, oracle, oracle_tables):
    pool = end_pool(16, 96, 6)
    out = eng.cross_dimer_end(pool, m.Chem.ntthal(), 47.0, want_dg=True, want_tm=True)
    _, _, _, t2 = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(), 0.0, mode=oracle.END2, want_t=True)
    _, _, _, t1 = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(), 0.0, mode=oracle.END1, want_t=True)
    np.testing.assert_array_equal(out["tm"].T, t2)
    pc = eng.pair_compl_end(pool, m.Chem.ntthal())
    np.testing.assert_array_equal(pc, np.maximum(t_end(t1), t_end(t2)))
    np.testing.assert_array_equal(pc, pc.T)


def test_edges(m, eng, oracle, oracle_tables):
    import torch
    pool = end_pool(13, 200, 7)
    n = len(pool)
    _, tt = oracle_square(oracle, oracle_tables, pool, oracle.ntthal_args())
    cf = end_rule(oracle, tt, 10.0)
    need = int(cf.sum())
    assert need > 2
    edges, count = eng.cross_dimer_end_edges(pool, m.Chem.ntthal(), 10.0)
    assert count == need
    ab = np.stack([edges["a"], edges["b"]], 1).astype(np.int64)
    np.testing.assert_array_equal(ab, np.argwhere(cf))          # sorted by (a, b), exactly the conflicts
    want_t = np.array([oracle.round_fixed_f32(float(t_end(tt[a, b])), 2) for a, b in ab], dtype=np.float32)
    np.testing.assert_array_equal(edges["t"], want_t)
    with pytest.raises(m.MsspeError) as ei:
        eng.cross_dimer_end_edges(pool, m.Chem.ntthal(), 10.0, capacity=need - 1)
    assert ei.value.code == 5 and ei.value.count == need
    # device edges: raw t, the bitmap as a set
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    d_edges = torch.zeros(2 * need * 2, dtype=torch.int64, device="cuda")   # 16-byte records
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.cross_dimer_end_edges_dev(d_pool.data_ptr(), n, 13, m.Chem.ntthal(), 10.0, (0, n), (0, n),
                                  d_edges.data_ptr(), 2 * need, d_count.data_ptr())
    eng.synchronize()
    assert int(d_count.item()) == need
    rec = d_edges.cpu().numpy().view(np.dtype([("a", np.uint32), ("b", np.uint32), ("t", np.float64)]))[:need]
    assert set(zip(rec["a"].tolist(), rec["b"].tolist())) == set(map(tuple, np.argwhere(cf).tolist()))
    np.testing.assert_array_equal(rec["t"], tt[rec["a"], rec["b"]])


# ---- 5. A x B ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_a,k_b", [(13, 20), (20, 13), (2, 17), (29, 31)])
def test_ab_shapes_match_the_oracle(m, eng, oracle, oracle_tables, k_a, k_b):
    A, B = end_pool(k_a, 64, 8), end_pool(k_b, 80, 9)
    for j in range(12):                       # B oligos pairing with A's 3' ends
        tail = A[j][-min(k_a, k_b):]
        B[j] = (rc(tail) + B[j])[:k_b]
    dg, tt = oracle_ab(oracle, oracle_tables, A, B, oracle.ntthal_args())
    out = eng.cross_dimer_end_ab(A, B, m.Chem.ntthal(), 10.0, want_dg=True, want_tm=True)
    check(oracle, out, dg, tt, 10.0)
    fast = eng.cross_dimer_end_ab(A, B, m.Chem.ntthal(), 10.0, want_dg=False, want_tm=False)
    np.testing.assert_array_equal(fast["bitmap"], out["bitmap"])


def test_ab_equal_lengths_equal_the_square_screen(m, eng):
    A, B = end_pool(13, 120, 10), end_pool(13, 150, 11)
    sq = eng.cross_dimer_end(A + B, m.Chem.ntthal(), 10.0, want_dg=True, want_tm=True)
    ab = eng.cross_dimer_end_ab(A, B, m.Chem.ntthal(), 10.0, want_dg=True, want_tm=True)
    np.testing.assert_array_equal(ab["dg"], sq["dg"][:120, 120:])
    np.testing.assert_array_equal(ab["tm"], sq["tm"][:120, 120:])
    np.testing.assert_array_equal(bits(ab["bitmap"], 150), bits(sq["bitmap"], 270)[:120, 120:])


# ---- 6. isolation from thal ANY ------------------------------------------------------------------------------------
def test_end_and_any_never_share_a_cut(m, eng, oracle, oracle_tables):
    pool = end_pool(13, 128, 12)
    chem = m.Chem.ntthal()
    thr = 47.0
    any1 = eng.cross_dimer(pool, chem, thr, want_dg=True)
    end = eng.cross_dimer_end(pool, chem, thr, want_dg=True, want_tm=True)
    any2 = eng.cross_dimer(pool, chem, thr, want_dg=True)
    for f in ("dg", "bitmap", "row_conflicts"):
        np.testing.assert_array_equal(any1[f], any2[f])
    _, dg, cf, _ = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(), thr)
    np.testing.assert_array_equal(bits(any1["bitmap"], len(pool)), cf)
    _, tt = oracle_square(oracle, oracle_tables, pool, oracle.ntthal_args())
    np.testing.assert_array_equal(bits(end["bitmap"], len(pool)), end_rule(oracle, tt, thr))
    assert cf.sum() != end_rule(oracle, tt, thr).sum()


# ---- 7. argument errors ------------------------------------------------------------------------------------------------
def test_argument_errors(m, eng):
    import torch
    chem = m.Chem.ntthal()
    d_pool = torch.zeros(8, dtype=torch.int64, device="cuda")
    p = d_pool.data_ptr()
    L = eng.L

    def dev(k=13, rows=(0, 8), cols=(0, 8), chem_ref=C_ref(chem), pool=p):
        return L.msspe_cross_dimer_end_dev(eng.ptr, pool, 8, k, chem_ref, 47.0, rows[0], rows[1], cols[0], cols[1],
                                           None, None, None, None)

    assert dev(k=1) == 2 and dev(k=33) == 2
    assert dev(rows=(5, 3)) == 1 and dev(cols=(0, 9)) == 1 and dev(rows=(-1, 2)) == 1
    assert dev(chem_ref=None) == 1
    assert dev(pool=None) == 1
    assert L.msspe_cross_dimer_end_ab_dev(eng.ptr, p, 8, 13, p, 8, 33, C_ref(chem), 47.0, 0, 8, 0, 8,
                                          None, None, None, None) == 2
    assert L.msspe_cross_dimer_end_ab_dev(eng.ptr, p, 8, 13, p, 8, 20, None, 47.0, 0, 8, 0, 8,
                                          None, None, None, None) == 1
    with pytest.raises(m.MsspeError) as ei:
        eng.cross_dimer_end(["ACGTNACGTACGT"] * 2, chem)
    assert ei.value.code == 1
    with pytest.raises(m.MsspeError) as ei:
        eng.cross_dimer_end_ab(["ACGTACGTACGTA"], ["ACGTACGTAXGTA"], chem)
    assert ei.value.code == 1
    rc = L.msspe_cross_dimer_end_edges_dev(eng.ptr, p, 8, 13, C_ref(chem), 47.0, 0, 8, 0, 8, None, None, 4, None)
    assert rc == 1


def C_ref(chem):
    import ctypes
    return ctypes.byref(chem)


# ---- 8. scale --------------------------------------------------------------------------------------------------------
def test_scale_8192_with_list_flushes(m, eng, oracle, oracle_tables):
    import torch
    n, k = 8192, 13
    pool = m.synth.pool_strings(m.synth.random_pool(n, k))
    chem = m.Chem.ntthal()
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    words = (n + 63) // 64
    d_bm = torch.zeros(n * words, dtype=torch.int64, device="cuda")
    d_rc = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_dg = torch.empty(n * n, dtype=torch.float64, device="cuda")
    d_tm = torch.empty(n * n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    try:
        eng.set_option("list_cap_log2", 20)         # 2^20-pair launches: 64 of them, and a flush after each
        eng.last_overflow_pairs()
        eng.profile_enable(True)
        eng.cross_dimer_end_dev(d_pool.data_ptr(), n, k, chem, 10.0, (0, n), (0, n), d_rc.data_ptr(),
                                d_bm.data_ptr(), d_dg.data_ptr(), d_tm.data_ptr())
        eng.synchronize()
        launches, _ = eng.profile_read()
        eng.profile_enable(False)
        handed = eng.last_overflow_pairs()
        assert launches > 1 and handed > 0
        # decisions only, the same bits
        d_bm2 = torch.zeros_like(d_bm)
        d_rc2 = torch.zeros_like(d_rc)
        eng.cross_dimer_end_dev(d_pool.data_ptr(), n, k, chem, 10.0, (0, n), (0, n), d_rc2.data_ptr(),
                                d_bm2.data_ptr())
        eng.synchronize()
    finally:
        eng.set_option("list_cap_log2", 0)
    assert torch.equal(d_bm, d_bm2) and torch.equal(d_rc, d_rc2)
    rows = np.sort(np.random.default_rng(8192).choice(n, 32, replace=False))
    bm = d_bm.view(n, words)[torch.from_numpy(rows).cuda()].cpu().numpy().view(np.uint64)
    dg = d_dg.view(n, n)[torch.from_numpy(rows).cuda()].cpu().numpy()
    tm = d_tm.view(n, n)[torch.from_numpy(rows).cuda()].cpu().numpy()
    rcs = d_rc.cpu().numpy()
    for q, r in enumerate(rows):
        _, odg, _, ott = oracle.pool_pairs(oracle_tables, pool, oracle.ntthal_args(), 0.0, mode=oracle.END1,
                                           rows=(int(r), int(r) + 1), want_t=True)
        np.testing.assert_array_equal(dg[q], odg[0])
        np.testing.assert_array_equal(tm[q], ott[0])
        cf = end_rule(oracle, ott, 10.0)[0]
        np.testing.assert_array_equal(bits(bm[q:q + 1], n)[0], cf)
        assert rcs[r] == cf.sum()
