"""The long hand-over chain of the thal ANY screen against the oracle, on pools small enough to compare whole planes.

A screen block of up to 2^23 pairs takes the short chain behind the first stage (integer list stage -> one wave per
pair -> dense kernel); larger blocks, the headline screen among them, take the long one:

    first stage -> integer list stage -> split-table list mode (split_list) -> f64 56-slot list stage -> wide table
                -> one wave per pair -> dense kernel

Option short_chain = 0 sends every block down the long chain, so that pools of a few hundred oligos, whose whole dG /
Tm planes the oracle computes in seconds, reach every stage of it.  The engine's per-list hand-over counters
(msspe_get_info "hand_over_list_<q>", Engine.hand_over_lists()) show which stages received pairs; with split_list = 1
list q is read by LONG_CHAIN[q].

Bar, as everywhere in the suite: dG and Tm planes bit for bit, identical bitmaps, counts and edge lists.
"""
import numpy as np
import pytest

from helpers import reverse_complement

pytestmark = pytest.mark.gpu

LONG_CHAIN = ("integer list", "split list", "main list", "wide", "wave", "dense")

# msspe_chem / pyoracle.ntthal_args keywords
CHEMS = {
    "ntthal": {},
    "primer3": dict(mv=50.0, dv=1.5, dntp=0.6, dna_conc=50.0, temp_c=37.0),
    "t60_dv0": dict(temp_c=60.0, dv=0.0),
    "t10_mv1500": dict(temp_c=10.0, mv=1500.0, dv=0.0),      # positive salt term
}
# Thresholds near the 30 % point of each (length, chemistry)'s finite dG values in chain_pool(k) (0.57 ... 0.95 of
# the pairs have a structure): a quarter of the pairs conflict from 7 bases on, and the cut runs through the bulk.
THRESHOLDS = {
    2: (500.0, 900.0, 1300.0, 100.0),
    3: (-100.0, 300.0, 1100.0, -800.0),
    5: (-1200.0, -600.0, 600.0, -2100.0),
    7: (-2100.0, -1300.0, 300.0, -3200.0),
    9: (-2800.0, -1800.0, 0.0, -4200.0),
    11: (-3400.0, -2300.0, -200.0, -4900.0),
    12: (-3500.0, -2400.0, -200.0, -5100.0),
    13: (-3700.0, -2600.0, -300.0, -5400.0),
    14: (-4100.0, -2900.0, -500.0, -6000.0),
    15: (-4200.0, -2900.0, -500.0, -6200.0),
    16: (-4400.0, -3100.0, -600.0, -6400.0),
}
KS = (2, 3, 5, 7, 9, 11, 12, 13, 14, 15)
TIE_14 = ["GCGGCGGCCGCCGC", "GCCGGCCGGGCGGG", "GGCCGGCCGGGCGG"]   # test_a_resolved_pick_whose_walks_meet_a_tie_stays_open
BIG_N = 1040          # 1,081,600 pairs > 2^20: with list_cap_log2 = 20 the lists flush between launches


def chain_pool(k: int, n: int | None = None) -> list[str]:
    """n oligos of length k (none of the sizes a multiple of 64), shuffled: homopolymers (poly-A x poly-T: k^2
    cells), palindromes (even k: self-complementary, so pairs of two of them reach the dense kernel), dinucleotide
    repeats, A/T-only and G/C-only oligos (tables beyond the integer list stage), T/C-only and A/G-only oligos (no
    complementary cell against their own kind: dG = inf), Dirichlet-skewed compositions, uniform ones and exact
    duplicates; for 14-mers the three oligos whose walks meet a tie."""
    n = n or (613 if k <= 9 else 533 if k <= 13 else 467 if k <= 15 else 421)
    rng = np.random.default_rng(500 + k + n)
    word = lambda letters, p=None: "".join(rng.choice(list(letters), k, p=p))
    pool = [b * k for b in "ACGT"]
    for _ in range(12):
        half = word("ACGT")[:k // 2]
        pool.append(half + ("A" if k % 2 else "") + reverse_complement(half))
    pool += [("GC" * k)[:k], ("AT" * k)[:k], ("TA" * k)[:k], ("CG" * k)[:k]]
    if k == 14:
        pool += TIE_14
    n_rest = n - len(pool) - 12
    pool += [word("AT") for _ in range(n_rest // 10)]
    pool += [word("GC") for _ in range(n_rest // 10)]
    pool += [word("TC") for _ in range(n_rest // 12)]
    pool += [word("AG") for _ in range(n_rest // 12)]
    pool += [word("ACGT", rng.dirichlet([0.4] * 4)) for _ in range(n_rest // 5)]
    pool += [word("ACGT") for _ in range(n - len(pool) - 12)]
    pool += [pool[int(i)] for i in rng.integers(0, len(pool), 12)]
    assert len(pool) == n and n % 64 and all(len(s) == k for s in pool)
    return [pool[int(i)] for i in rng.permutation(n)]


_POOLS: dict = {}
_ORACLE: dict = {}
_STAGE_PAIRS: dict = {}     # (k, chemistry) -> hand-over lists of the long-chain screen with planes


def pool_of(k, n=None):
    if (k, n) not in _POOLS:
        _POOLS[(k, n)] = chain_pool(k, n)
    return _POOLS[(k, n)]


def thr_of(k, chem):
    return THRESHOLDS[k][list(CHEMS).index(chem)]


def oracle_of(oracle, tables, k, chem, n=None, max_loop=30):
    """(count, dg, conflicts, t) of the whole pool at the case's threshold, computed once per module."""
    key = (k, n, chem, max_loop)
    if key not in _ORACLE:
        args = oracle.ntthal_args(max_loop=max_loop, **CHEMS[chem])
        _ORACLE[key] = oracle.pool_pairs(tables, pool_of(k, n), args, thr_of(k, chem), want_t=True)
    return _ORACLE[key]


def chem_of(m, chem, max_loop=30):
    return m.Chem.ntthal(max_loop=max_loop, **CHEMS[chem])


def bits(bm, n):
    return np.unpackbits(bm.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def screen(eng, m, pool, chem, thr, **kw):
    """cross_dimer with the hand-over lists of that call alone."""
    eng.hand_over_lists()
    out = eng.cross_dimer(pool, chem, thr, **kw)
    return out, eng.hand_over_lists()


def assert_oracle(out, ref, n):
    _, dg, cf, tt = ref
    np.testing.assert_array_equal(out["dg"], dg)
    np.testing.assert_array_equal(out["tm"], tt)
    np.testing.assert_array_equal(bits(out["bitmap"], n), cf.astype(bool))
    np.testing.assert_array_equal(out["row_conflicts"], cf.sum(1).astype(np.uint32))


def assert_chain_length(lists, stages):
    """A route of `stages` stages behind the first one reads lists 0 .. stages - 1 and writes no list beyond."""
    assert all(v == 0 for v in lists[stages:]), lists


@pytest.fixture(scope="module")
def eng():
    import msspe_amd
    e = msspe_amd.Engine(0)
    e.set_option("short_chain", 0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


def _edges_as_the_reference_reads_them(oracle, dg_values):
    """Edge::get_dg(): "%g" -> f32 -> "{:.2}" -> f32 (delta_g.rs:10-15), per distinct value."""
    uniq, inv = np.unique(dg_values, return_inverse=True)
    r = np.array([oracle.round_fixed_f32(float(oracle.round_g_f32(float(x))), 2) for x in uniq], dtype=np.float32)
    return r[inv]


@pytest.mark.parametrize("chem", list(CHEMS))
@pytest.mark.parametrize("k", KS)
def test_long_chain_equals_the_oracle(eng, m, oracle, oracle_tables, k, chem):
    """Whole planes, bitmap and counts of the long chain against the oracle; then the same pool and chemistry as the
    decisions-only call, as the edge list, and on the short chain: the same bits."""
    pool = pool_of(k)
    n = len(pool)
    thr = thr_of(k, chem)
    ref = oracle_of(oracle, oracle_tables, k, chem)
    out, lists = screen(eng, m, pool, chem_of(m, chem), thr, want_dg=True, want_tm=True)
    _STAGE_PAIRS[(k, chem)] = lists
    print(f"hand-over k={k} {chem}: " + ", ".join(f"{s} {v}" for s, v in zip(LONG_CHAIN, lists)))
    assert_oracle(out, ref, n)
    cnt, dg, cf, _ = ref
    if k >= 7:
        assert 0.02 < cnt / (n * n) < 0.9, cnt / (n * n)
    else:
        assert cnt > 0
    assert lists[0] > 0                      # the integer list stage received pairs
    assert_chain_length(lists, len(LONG_CHAIN))

    fast = eng.cross_dimer(pool, chem_of(m, chem), thr, want_dg=False, want_tm=False)
    np.testing.assert_array_equal(fast["bitmap"], out["bitmap"])
    np.testing.assert_array_equal(fast["row_conflicts"], out["row_conflicts"])

    edges, count = eng.cross_dimer_edges(pool, chem_of(m, chem), thr)
    want = np.argwhere(cf.astype(bool))
    assert count == len(want) == cnt
    np.testing.assert_array_equal(np.stack([edges["a"], edges["b"]], 1), want)
    np.testing.assert_array_equal(edges["dg"], _edges_as_the_reference_reads_them(oracle, dg[cf.astype(bool)]))

    eng.set_option("short_chain", 1)
    try:
        short, short_lists = screen(eng, m, pool, chem_of(m, chem), thr, want_dg=False, want_tm=False)
    finally:
        eng.set_option("short_chain", 0)
    np.testing.assert_array_equal(short["bitmap"], out["bitmap"])
    np.testing.assert_array_equal(short["row_conflicts"], out["row_conflicts"])
    assert_chain_length(short_lists, 3)      # integer list stage -> one wave per pair -> dense kernel


def test_every_stage_of_the_long_chain_received_pairs(eng, m):
    """Summed over the cases of test_long_chain_equals_the_oracle (run again here, GPU only, where that test did not
    run in this session), every stage of the long chain received pairs: the integer list stage, the split-table list
    mode, the f64 56-slot list stage, the wide table, one wave per pair and the dense kernel."""
    totals = np.zeros(7, dtype=np.int64)
    for k in KS:
        for chem in CHEMS:
            lists = _STAGE_PAIRS.get((k, chem))
            if lists is None:
                _, lists = screen(eng, m, pool_of(k), chem_of(m, chem), thr_of(k, chem), want_dg=True, want_tm=True)
            totals += np.array(lists, dtype=np.int64)
    print("hand-over totals: " + ", ".join(f"{s} {v}" for s, v in zip(LONG_CHAIN, totals)))
    for stage, v in zip(LONG_CHAIN, totals):
        assert v > 0, f"the {stage} stage received no pair"


# option settings of the long chain: each alone and the pairs that shorten it the most
SWITCHES = [
    dict(pair_kernel="int"),
    dict(split_list=0),
    dict(wave_kernel=0),
    dict(row_oob=0),
    dict(split_list=0, wave_kernel=0),
    dict(pair_kernel="int", split_list=0, row_oob=0),
]
DEFAULTS = dict(pair_kernel="auto", split_list=1, wave_kernel=1, row_oob=1)


@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: "-".join(f"{a}{b}" for a, b in s.items()))
@pytest.mark.parametrize("k", [11, 13, 14, 15])
def test_every_switch_on_the_long_chain(eng, m, oracle, oracle_tables, k, switch):
    """The first stage (row-specialised or general integer kernel), with and without the split-table list mode, with
    and without one wave per pair: the oracle's planes, and a chain of as many stages as the route has."""
    pool = pool_of(k)
    ref = oracle_of(oracle, oracle_tables, k, "ntthal")
    for key, v in switch.items():
        eng.set_option(key, v)
    try:
        out, lists = screen(eng, m, pool, chem_of(m, "ntthal"), thr_of(k, "ntthal"), want_dg=True, want_tm=True)
        fast = eng.cross_dimer(pool, chem_of(m, "ntthal"), thr_of(k, "ntthal"), want_dg=False, want_tm=False)
    finally:
        for key in switch:
            eng.set_option(key, DEFAULTS[key])
    print(f"hand-over k={k} {switch}: {lists}")
    assert_oracle(out, ref, len(pool))
    np.testing.assert_array_equal(fast["bitmap"], out["bitmap"])
    assert lists[0] > 0
    stages = 6 - (switch.get("split_list", 1) == 0) - (switch.get("wave_kernel", 1) == 0)
    assert_chain_length(lists, stages)


@pytest.mark.parametrize("k", [11, 13, 14, 15])
def test_lists_that_flush_between_launches(eng, m, oracle, oracle_tables, k):
    """list_cap_log2 = 20 on a pool of more than 2^20 pairs: the launches shrink to what a list holds and the lists
    are flushed through the whole chain between them; planes and bits are the oracle's."""
    pool = pool_of(k, BIG_N)
    assert BIG_N * BIG_N > 1 << 20
    ref = oracle_of(oracle, oracle_tables, k, "ntthal", n=BIG_N)
    eng.set_option("list_cap_log2", 20)
    try:
        out, lists = screen(eng, m, pool, chem_of(m, "ntthal"), thr_of(k, "ntthal"), want_dg=True, want_tm=True)
        fast = eng.cross_dimer(pool, chem_of(m, "ntthal"), thr_of(k, "ntthal"), want_dg=False, want_tm=False)
    finally:
        eng.set_option("list_cap_log2", 0)
    print(f"hand-over k={k} n={BIG_N} list_cap_log2=20: {lists}")
    assert_oracle(out, ref, BIG_N)
    np.testing.assert_array_equal(fast["bitmap"], out["bitmap"])
    np.testing.assert_array_equal(fast["row_conflicts"], out["row_conflicts"])
    assert lists[0] > 0 and lists[1] > 0


def cuts_at_pairs_own_values(m, dg):
    """Thresholds that are pairs' own dG as f32, near the 0.2 %, 1 %, 5 %, 20 % and 50 % points of the finite values:
    from each point on, the first value whose cut has a pair of the plane within 1e-3 cal/mol (the decisions-only
    margin), else the value at the point."""
    uniq = np.unique(dg[np.isfinite(dg)])
    cuts = []
    for q in (0.002, 0.01, 0.05, 0.2, 0.5):
        i0 = int(q * uniq.size)
        thr = float(np.float32(uniq[i0]))
        for v in uniq[i0:i0 + 4000]:
            t = float(np.float32(v))
            c = m.g_cut(t)
            j = int(np.searchsorted(uniq, c))
            if any(abs(uniq[i] - c) < 1e-3 for i in (j - 1, j) if 0 <= i < uniq.size):
                thr = t
                break
        cuts.append(thr)
    return cuts


@pytest.mark.parametrize("chem", list(CHEMS))
@pytest.mark.parametrize("k", [11, 13, 15])
def test_decisions_at_cuts_that_are_pairs_own_values_on_the_long_chain(eng, m, oracle, oracle_tables, k, chem):
    """Thresholds that are the dG of pairs of the pool, as the f32 the reference compares in: the decisions-only
    call's shortcuts (a tied pick that cannot conflict, thal_pairs_int.hip / thal_pairs_row.hip kCutMargin) must
    still give the oracle's plane cut the reference's way, in the bitmap, the counts and the edge list."""
    pool = pool_of(k)
    n = len(pool)
    _, dg, _, _ = oracle_of(oracle, oracle_tables, k, chem)
    near = 0
    for thr in cuts_at_pairs_own_values(m, dg):
        want = dg <= m.g_cut(thr)
        near += int((np.abs(dg - m.g_cut(thr)) < 1e-3).sum())
        fast = eng.cross_dimer(pool, chem_of(m, chem), thr, want_dg=False, want_tm=False)
        np.testing.assert_array_equal(bits(fast["bitmap"], n), want)
        np.testing.assert_array_equal(fast["row_conflicts"], want.sum(1).astype(np.uint32))
        edges, count = eng.cross_dimer_edges(pool, chem_of(m, chem), thr)
        assert count == int(want.sum())
        np.testing.assert_array_equal(np.stack([edges["a"], edges["b"]], 1), np.argwhere(want))
    assert near > 0      # pairs sat inside the margin


@pytest.mark.parametrize("k", [11, 13, 14])
def test_sub_block_on_the_long_chain(eng, m, oracle, oracle_tables, k):
    """cross_dimer_dev on a rectangle (r0, r1) x (c0, c1): the list stages write through the column permutation of
    the composition sort and the block's offsets into the block's cells, and nowhere else (guard words around every
    output, counts of the rows outside the block stay zero)."""
    import torch
    pool = pool_of(k)
    n = len(pool)
    r0, r1, c0, c1 = 37, n - 50, 70, n - 21
    nr, nc = r1 - r0, c1 - c0
    words = (nc + 63) // 64
    guard = 4096
    _, dg, cf, tt = oracle_of(oracle, oracle_tables, k, "ntthal")
    d_pool = torch.from_numpy(m.pack_oligos(pool).view(np.int64)).cuda()
    d_rc = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_dg = torch.full((2 * guard + nr * nc,), 7.0, dtype=torch.float64, device="cuda")
    d_tm = torch.full((2 * guard + nr * nc,), -3.0, dtype=torch.float64, device="cuda")
    d_bm = torch.full((2 * guard + nr * words,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    eng.hand_over_lists()
    eng.synchronize()        # the reset above is enqueued on the engine's own stream
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        eng.cross_dimer_dev(d_pool.data_ptr(), n, k, chem_of(m, "ntthal"), thr_of(k, "ntthal"), (r0, r1), (c0, c1),
                            d_rc.data_ptr(), d_bm.data_ptr() + 8 * guard, d_dg.data_ptr() + 8 * guard,
                            d_tm.data_ptr() + 8 * guard)
        torch.cuda.synchronize()
    finally:
        eng.reset_stream()
    lists = eng.hand_over_lists()
    print(f"hand-over k={k} block: {lists}")
    assert lists[0] > 0 and lists[1] > 0
    g_dg, g_tm, g_bm = d_dg.cpu().numpy(), d_tm.cpu().numpy(), d_bm.cpu().numpy()
    for buf, fill in ((g_dg, 7.0), (g_tm, -3.0), (g_bm, 0x5A5A5A5A5A5A5A5A)):
        assert (buf[:guard] == fill).all() and (buf[-guard:] == fill).all()
    np.testing.assert_array_equal(g_dg[guard:-guard].reshape(nr, nc), dg[r0:r1, c0:c1])
    np.testing.assert_array_equal(g_tm[guard:-guard].reshape(nr, nc), tt[r0:r1, c0:c1])
    got = bits(g_bm[guard:-guard].reshape(nr, words).view(np.uint64), nc)
    np.testing.assert_array_equal(got, cf[r0:r1, c0:c1].astype(bool))
    want = np.zeros(n, dtype=np.int64)
    want[r0:r1] = cf[r0:r1, c0:c1].sum(1)
    np.testing.assert_array_equal(d_rc.cpu().numpy().astype(np.int64), want)


@pytest.mark.parametrize("k", [9, 13, 14, 15, 16])
def test_max_loop_at_the_route_boundary(eng, m, oracle, oracle_tables, k):
    """max_loop = 2k - 5 sends the block to the split-table first stage (one wave per pair, the dense kernel behind
    it); 2k - 4 keeps the register-table route and its long chain, and since no internal loop of a k x k table is
    longer than 2k - 4, gives what max_loop = 30 gives, bit for bit.  16-mers with split_min_k = 99, so that 2k - 4
    does not go to the split-table kernel anyway."""
    pool = pool_of(k)
    thr = thr_of(k, "ntthal")
    if k == 16:
        eng.set_option("split_min_k", 99)
    try:
        for max_loop in (2 * k - 5, 2 * k - 4):
            ref = oracle_of(oracle, oracle_tables, k, "ntthal", max_loop=max_loop)
            out, lists = screen(eng, m, pool, chem_of(m, "ntthal", max_loop), thr, want_dg=True, want_tm=True)
            print(f"hand-over k={k} max_loop={max_loop}: {lists}")
            assert_oracle(out, ref, len(pool))
            assert ref[0] > 0
            if max_loop == 2 * k - 5:
                assert_chain_length(lists, 2)      # split-table first stage -> one wave per pair -> dense kernel
            else:
                assert lists[1] > 0                # the integer list stage handed pairs on
        full = eng.cross_dimer(pool, chem_of(m, "ntthal", 30), thr, want_dg=True, want_tm=True)
    finally:
        eng.set_option("split_min_k", 16)
    for key in ("dg", "tm", "bitmap", "row_conflicts"):
        np.testing.assert_array_equal(out[key], full[key])
