"""One pool screened against another, the two of different oligo lengths (msspe_cross_dimer_ab*,
msspe_cross_dimer_edges_mixed), on the MI355X.  The CPU oracle is the checker: thal ANY per ordered pair
(pyoracle.thal, Primer3 2.6.1 thal.c restated, which takes len1 != len2) and the reference's decision
(pyoracle.edge_decision).  The reference itself only ever screens one --kmer-size against itself, so none of its
vectors has unequal lengths: the mixed results are pinned to the oracle alone."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = -9000.0


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


def rand_oligos(rng, n, k):
    return ["".join("ACGT"[x] for x in rng.integers(0, 4, k)) for _ in range(n)]


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def self_comp(rng, k):
    half = "".join("ACGT"[x] for x in rng.integers(0, 4, k // 2))
    return half + rc(half)


def pools(k_a, k_b, n_a=160, n_b=224, seed=0):
    """Random pools with constructed conflicts: B rows holding the reverse complement of a substring of an A row
    (or A's reverse complement inside random flanks), self-complementary oligos on both sides (even lengths),
    homopolymers and their complements."""
    rng = np.random.default_rng(seed * 1000 + k_a * 33 + k_b)
    A, B = rand_oligos(rng, n_a, k_a), rand_oligos(rng, n_b, k_b)
    for j in range(min(40, n_a, n_b)):
        a = A[j]
        if k_b <= k_a:
            at = int(rng.integers(0, k_a - k_b + 1))
            B[j] = rc(a[at:at + k_b])
        else:
            at = int(rng.integers(0, k_b - k_a + 1))
            B[j] = B[j][:at] + rc(a) + B[j][at + k_a:]
    for q in range(6):
        if k_a % 2 == 0:
            A[n_a - 1 - q] = self_comp(rng, k_a)
        if k_b % 2 == 0:
            B[n_b - 1 - q] = self_comp(rng, k_b)
    A[n_a - 8], A[n_a - 9] = "A" * k_a, "G" * k_a
    B[n_b - 8], B[n_b - 9] = "T" * k_b, "C" * k_b
    return A, B


def oracle_block(oracle, tables, A, B, args, thr=THR):
    """(dG, t, conflict) over A x B: +inf / 0 / 0 where thal finds no structure."""
    dg = np.empty((len(A), len(B)))
    tt = np.empty((len(A), len(B)))

    def row(i):
        for j, b in enumerate(B):
            r = oracle.thal(tables, A[i], b, oracle.ANY, args)
            dg[i, j] = np.inf if r.no_structure else r.dG
            tt[i, j] = 0.0 if r.no_structure else r.t

    with ThreadPoolExecutor(16) as ex:       # the oracle library releases the GIL and is re-entrant
        list(ex.map(row, range(len(A))))
    cf = np.zeros(dg.shape, dtype=np.uint8)
    for i, j in zip(*np.nonzero(dg < thr + 1000.0)):   # a conflict needs dG within rounding of the threshold
        cf[i, j] = oracle.edge_decision(float(dg[i, j]), thr)
    return dg, tt, cf


def bits(bitmap, ncols):
    return np.unpackbits(bitmap.view(np.uint8), axis=1, bitorder="little")[:, :ncols]


# ---- 1. equal lengths through the A x B entry points: the single-pool chain, bit for bit ------------------------
@pytest.mark.parametrize("k", [13, 20])
def test_equal_lengths_equal_the_square_block(m, eng, k):
    import torch
    rng = np.random.default_rng(k)
    A, B = rand_oligos(rng, 300, k), rand_oligos(rng, 400, k)
    B[:20] = [rc(a) for a in A[:20]]
    chem = m.Chem.ntthal()
    sq = eng.cross_dimer(A + B, chem, THR, want_dg=True, want_tm=True)
    ab = eng.cross_dimer_ab(A, B, chem, THR, want_dg=True, want_tm=True)
    np.testing.assert_array_equal(ab["dg"], sq["dg"][:300, 300:])
    np.testing.assert_array_equal(ab["tm"], sq["tm"][:300, 300:])
    np.testing.assert_array_equal(bits(ab["bitmap"], 400), bits(sq["bitmap"], 700)[:300, 300:])
    # row counts restricted to B's columns: the square screen over that block
    d_pool = torch.from_numpy(m.pack_oligos(A + B).view(np.int64)).cuda()
    d_rc = torch.zeros(700, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.cross_dimer_dev(d_pool.data_ptr(), 700, k, chem, THR, (0, 300), (300, 700), d_rc.data_ptr())
    eng.synchronize()
    np.testing.assert_array_equal(ab["row_conflicts"], d_rc[:300].cpu().numpy().astype(np.uint32))
    assert ab["row_conflicts"].sum() >= 20
    # decisions only (no planes): the same bits
    fast = eng.cross_dimer_ab(A, B, chem, THR, want_dg=False)
    np.testing.assert_array_equal(bits(fast["bitmap"], 400), bits(ab["bitmap"], 400))
    np.testing.assert_array_equal(fast["row_conflicts"], ab["row_conflicts"])


# ---- 2. mixed shapes against the oracle -------------------------------------------------------------------------
SHAPES = [(13, 20), (20, 13), (13, 14), (16, 25), (8, 32), (32, 8), (2, 17), (29, 31)]
CHEMS = {
    "ntthal25": (lambda m: m.Chem.ntthal(), lambda o: o.ntthal_args()),
    "ntthal37": (lambda m: m.Chem.ntthal(temp_c=37.0), lambda o: o.ntthal_args(temp_c=37.0)),
    "primer3": (lambda m: m.Chem.primer3(), lambda o: o.p3_args()),
    "maxloop7": (lambda m: m.Chem.ntthal(max_loop=7), lambda o: o.ntthal_args(max_loop=7)),
}


@pytest.mark.parametrize("chem_name", list(CHEMS))
@pytest.mark.parametrize("k_a,k_b", SHAPES)
def test_mixed_shapes_match_the_oracle(m, eng, oracle, oracle_tables, k_a, k_b, chem_name):
    A, B = pools(k_a, k_b)
    chem, args = CHEMS[chem_name][0](m), CHEMS[chem_name][1](oracle)
    out = eng.cross_dimer_ab(A, B, chem, THR, want_dg=True, want_tm=True)
    dg, tt, cf = oracle_block(oracle, oracle_tables, A, B, args)
    np.testing.assert_array_equal(out["dg"], dg)
    np.testing.assert_array_equal(out["tm"], tt)
    np.testing.assert_array_equal(bits(out["bitmap"], len(B)), cf)
    np.testing.assert_array_equal(out["row_conflicts"], cf.sum(1).astype(np.uint32))
    if chem_name == "ntthal25" and min(k_a, k_b) >= 8:
        assert cf.sum() >= 20          # the constructed pairs conflict at -9000 (a 2-mer cannot reach it)
    fast = eng.cross_dimer_ab(A, B, chem, THR, want_dg=False)
    np.testing.assert_array_equal(bits(fast["bitmap"], len(B)), cf)


# ---- 3. every stage of the rectangular chain gives the same answer ----------------------------------------------
@pytest.mark.parametrize("k_a,k_b", [(16, 22), (13, 20)])
def test_every_stage_of_the_chain_agrees(m, eng, k_a, k_b):
    A, B = pools(k_a, k_b, 1024, 1536, seed=1)
    chem = m.Chem.ntthal()
    eng.last_overflow_pairs()
    eng.pair_stage_stats()
    ref = eng.cross_dimer_ab(A, B, chem, THR, want_dg=True, want_tm=True)
    handed_on = eng.last_overflow_pairs()
    stats = eng.pair_stage_stats()
    # the split-table stage answered the pairs itself: the hot path is the new kernel, not the dense one
    assert handed_on <= 0.03 * len(A) * len(B), (handed_on, stats)
    for key, value in [("force_generic", 1), ("wave_kernel", 0), ("split_lanes", 2), ("split_lanes", 4),
                       ("split_lanes", 8), ("list_cap_log2", 20)]:
        default = {"force_generic": 0, "wave_kernel": 1, "split_lanes": 0, "list_cap_log2": 0}[key]
        eng.set_option(key, value)
        try:
            got = eng.cross_dimer_ab(A, B, chem, THR, want_dg=True, want_tm=True)
        finally:
            eng.set_option(key, default)
        for name in ("dg", "tm", "bitmap", "row_conflicts"):
            np.testing.assert_array_equal(got[name], ref[name], err_msg=f"{key}={value}: {name}")


def test_long_columns_without_the_wave_kernel(m, eng, oracle, oracle_tables):
    """Short rows against long columns with the wave kernel switched off: the split kernel, else the dense kernel
    answers -- never the square-only first stages, which would read the columns as row-length oligos."""
    A, B = pools(8, 32)
    eng.set_option("wave_kernel", 0)
    try:
        out = eng.cross_dimer_ab(A, B, m.Chem.ntthal(), THR, want_dg=True, want_tm=True)
    finally:
        eng.set_option("wave_kernel", 1)
    dg, tt, cf = oracle_block(oracle, oracle_tables, A, B, oracle.ntthal_args())
    np.testing.assert_array_equal(out["dg"], dg)
    np.testing.assert_array_equal(out["tm"], tt)
    np.testing.assert_array_equal(bits(out["bitmap"], len(B)), cf)


def test_tables_without_the_split_kernel(m, oracle, tmp_path):
    """Parameter files off the 0.01 e.u. grid: no split-table kernel.  A rectangle of 8-mer rows (which the square
    register-table chain would take) goes to the wave kernel, and with that off to the dense kernel; both equal
    the oracle on the same files."""
    from param_variants import _perturbed, _read_bundle
    sections = _perturbed(_read_bundle(oracle.default_bundle()), 0.003, 0.0)
    path = tmp_path / "offgrid.bundle"
    path.write_text("# test bundle\n" + "".join(
        f"@ {name} {sum(len(l.split()) for l in lines)}\n" + "\n".join(lines) + "\n"
        for name, lines in sections.items()))
    tables = oracle.Tables(path)
    A, B = pools(8, 20, 96, 128, seed=3)
    dg, tt, cf = oracle_block(oracle, tables, A, B, oracle.ntthal_args())
    e = m.Engine(0, params_path=str(path))
    try:
        for wave in (1, 0):
            e.set_option("wave_kernel", wave)
            out = e.cross_dimer_ab(A, B, m.Chem.ntthal(), THR, want_dg=True, want_tm=True)
            np.testing.assert_array_equal(out["dg"], dg, err_msg=f"wave_kernel={wave}")
            np.testing.assert_array_equal(out["tm"], tt, err_msg=f"wave_kernel={wave}")
            np.testing.assert_array_equal(bits(out["bitmap"], len(B)), cf, err_msg=f"wave_kernel={wave}")
        edges, count = e.cross_dimer_edges_mixed(A + B, m.Chem.ntthal(), THR)   # the (8, 20) block of a mixed pool
        ab = [(int(x["a"]), int(x["b"]) - len(A)) for x in edges if x["a"] < len(A) <= x["b"]]
        assert ab == list(zip(*(v.tolist() for v in np.nonzero(cf))))
    finally:
        e.close()


def test_list_flushes_keep_every_pair(m, eng):
    """A hand-over list of 2^20 entries under a 2^21-pair screen: several flushes, same answers."""
    A, B = pools(16, 22, 1024, 2560, seed=2)
    chem = m.Chem.ntthal()
    ref = eng.cross_dimer_ab(A, B, chem, THR, want_dg=True)
    eng.set_option("list_cap_log2", 20)
    try:
        got = eng.cross_dimer_ab(A, B, chem, THR, want_dg=True)
    finally:
        eng.set_option("list_cap_log2", 0)
    np.testing.assert_array_equal(got["dg"], ref["dg"])
    np.testing.assert_array_equal(got["bitmap"], ref["bitmap"])


# ---- 4. blocks, outputs and errors ------------------------------------------------------------------------------
def test_blocks_dirty_bitmap_and_device_edges(m, eng):
    import torch
    A, B = pools(16, 25)
    chem = m.Chem.ntthal()
    full = eng.cross_dimer_ab(A, B, chem, THR, want_dg=True, want_tm=True)
    r0, r1, c0, c1 = 17, 140, 33, 201
    d_a = torch.from_numpy(m.pack_oligos(A).view(np.int64)).cuda()
    d_b = torch.from_numpy(m.pack_oligos(B).view(np.int64)).cuda()
    words = (c1 - c0 + 63) // 64
    d_rc = torch.zeros(len(A), dtype=torch.int32, device="cuda")
    d_bm = torch.full((r1 - r0, words), -1, dtype=torch.int64, device="cuda")   # dirty: the call clears it
    d_dg = torch.full((r1 - r0, c1 - c0), 7.0, dtype=torch.float64, device="cuda")
    d_tm = torch.full((r1 - r0, c1 - c0), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.cross_dimer_ab_dev(d_a.data_ptr(), len(A), 16, d_b.data_ptr(), len(B), 25, chem, THR, (r0, r1), (c0, c1),
                           d_rc.data_ptr(), d_bm.data_ptr(), d_dg.data_ptr(), d_tm.data_ptr())
    eng.synchronize()
    np.testing.assert_array_equal(d_dg.cpu().numpy(), full["dg"][r0:r1, c0:c1])
    np.testing.assert_array_equal(d_tm.cpu().numpy(), full["tm"][r0:r1, c0:c1])
    want_bits = bits(full["bitmap"], len(B))[r0:r1, c0:c1]
    np.testing.assert_array_equal(bits(d_bm.cpu().numpy().view(np.uint64), c1 - c0), want_bits)
    rc_want = np.zeros(len(A), dtype=np.uint32)
    rc_want[r0:r1] = want_bits.sum(1)
    np.testing.assert_array_equal(d_rc.cpu().numpy().astype(np.uint32), rc_want)
    assert want_bits.sum() > 0
    # the edge list of the block: A and B indices, raw dG
    cap = 4096
    d_edges = torch.zeros((cap, 2), dtype=torch.int64, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.cross_dimer_ab_edges_dev(d_a.data_ptr(), len(A), 16, d_b.data_ptr(), len(B), 25, chem, THR, (r0, r1),
                                 (c0, c1), d_edges.data_ptr(), cap, d_count.data_ptr())
    eng.synchronize()
    cnt = int(d_count.item())
    rec = d_edges[:cnt].cpu().numpy().view(np.dtype([("a", np.uint32), ("b", np.uint32), ("dg", np.float64)]))
    rec = rec.reshape(-1)
    got = sorted((int(e["a"]), int(e["b"]), float(e["dg"])) for e in rec)
    ii, jj = np.nonzero(want_bits)
    want = sorted((int(i) + r0, int(j) + c0, float(full["dg"][i + r0, j + c0])) for i, j in zip(ii, jj))
    assert got == want


def test_host_edges_sorted_rounded_and_capacity(m, eng, oracle, oracle_tables):
    A, B = pools(20, 13)
    chem = m.Chem.ntthal()
    edges, count = eng.cross_dimer_ab_edges(A, B, chem, THR)
    dg, _, cf = oracle_block(oracle, oracle_tables, A, B, oracle.ntthal_args())
    ii, jj = np.nonzero(cf)
    assert count == len(ii) > 1
    np.testing.assert_array_equal(edges["a"], ii.astype(np.uint32))      # np.nonzero is row-major: sorted by (a, b)
    np.testing.assert_array_equal(edges["b"], jj.astype(np.uint32))
    want = [oracle.round_fixed_f32(oracle.round_g_f32(float(dg[i, j])), 2) for i, j in zip(ii, jj)]
    np.testing.assert_array_equal(edges["dg"], np.array(want, dtype=np.float32))
    with pytest.raises(m.MsspeError) as ei:
        eng.cross_dimer_ab_edges(A, B, chem, THR, capacity=1)
    assert ei.value.code == 5 and ei.value.count == count


def test_argument_errors_and_empty_pools(m, eng):
    chem = m.Chem.ntthal()
    A, B = pools(13, 20, 8, 8)
    for bad in (["A" * 33] * 2, ["A"] * 2):
        with pytest.raises(m.MsspeError) as ei:
            eng.cross_dimer_ab(bad, B, chem, THR)
        assert ei.value.code == 2              # MSSPE_ERR_K
        with pytest.raises(m.MsspeError) as ei:
            eng.cross_dimer_ab(A, bad, chem, THR)
        assert ei.value.code == 2
    with pytest.raises(m.MsspeError) as ei:
        eng.cross_dimer_ab(A, ["ACGTNACGTACGTACGTACG"] + B[1:], chem, THR)
    assert ei.value.code == 1                  # MSSPE_ERR_ARG: not ACGT
    with pytest.raises(m.MsspeError) as ei:
        eng.cross_dimer_edges_mixed(["ACGTACGTAC", "ACGTUACGT"], chem, THR)
    assert ei.value.code == 1
    with pytest.raises(m.MsspeError) as ei:
        eng.cross_dimer_edges_mixed(["ACGTACGTAC", "A" * 33], chem, THR)
    assert ei.value.code == 2
    out = eng.cross_dimer_ab([], B, chem, THR)
    assert out["row_conflicts"].shape == (0,) and out["dg"].shape == (0, 8)
    out = eng.cross_dimer_ab(A, [], chem, THR)
    assert out["row_conflicts"].shape == (8,) and not out["row_conflicts"].any()
    assert eng.cross_dimer_edges_mixed([], chem, THR)[1] == 0
    assert eng.cross_dimer_ab_edges([], B, chem, THR)[1] == 0


# ---- 5. one pool of mixed lengths -------------------------------------------------------------------------------
def test_mixed_pool_edges_match_the_oracle(m, eng, oracle, oracle_tables):
    rng = np.random.default_rng(5)
    pool = []
    for k in range(12, 23):
        pool += rand_oligos(rng, 36, k)
    # complementary partners across lengths, self-complementary and homopolymer oligos
    for q in range(24):
        a = pool[int(rng.integers(0, len(pool)))]
        cut = int(rng.integers(12, len(a) + 1))
        pool.append(rc(a[:cut]) if q % 2 else "".join("ACGT"[x] for x in rng.integers(0, 4, 3)) + rc(a)[:19])
    pool += [self_comp(rng, 14), self_comp(rng, 20), "A" * 16, "T" * 21]
    pool = [pool[i] for i in rng.permutation(len(pool))]
    edges, count = eng.cross_dimer_edges_mixed(pool, m.Chem.ntthal(), THR)
    dg, _, cf = oracle_block(oracle, oracle_tables, pool, pool, oracle.ntthal_args())
    ii, jj = np.nonzero(cf)
    assert count == len(ii) > 24
    np.testing.assert_array_equal(edges["a"], ii.astype(np.uint32))
    np.testing.assert_array_equal(edges["b"], jj.astype(np.uint32))
    want = [oracle.round_fixed_f32(oracle.round_g_f32(float(dg[i, j])), 2) for i, j in zip(ii, jj)]
    np.testing.assert_array_equal(edges["dg"], np.array(want, dtype=np.float32))


@pytest.mark.parametrize("k", [13, 20])
def test_mixed_call_on_one_length_equals_cross_dimer_edges(m, eng, k):
    rng = np.random.default_rng(k + 100)
    pool = rand_oligos(rng, 250, k)
    pool[:10] = [rc(p) for p in pool[10:20]]
    e1, c1 = eng.cross_dimer_edges(pool, m.Chem.ntthal(), THR)
    e2, c2 = eng.cross_dimer_edges_mixed(pool, m.Chem.ntthal(), THR)
    assert c1 == c2 > 0
    np.testing.assert_array_equal(e1, e2)
