"""The greedy vertex cover of the conflict graph on the device (msspe_conflict_cover*, csrc/conflict_cover.hip) against
the reference's sequential rule: the round model (tests/cover_round_model.py, itself checked against
oracle/ref_pipeline.py:vertex_cover) on hand-built bitmaps, deleted set and round count; the host's odm_vertex_cover fed
with the edge list of the same screen on thermodynamic pools."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import cover_round_model as crm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
COMP = str.maketrans("ACGT", "TGCA")


@pytest.fixture(scope="module")
def m():
    import msspe_amd
    return msspe_amd


@pytest.fixture(scope="module")
def eng(m):
    e = m.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def host(m):
    return C.CDLL(str(HOST_LIB))


def revcomp(w):
    return w.translate(COMP)[::-1]


def distinct(words):
    return list(dict.fromkeys(words))


def bitmap_words(b, pad_garbage=False):
    """bool (n, n) -> uint64 (n, ceil(n/64)), bit j of row i = b[i, j]; pad_garbage: every bit beyond n set."""
    n = b.shape[0]
    wds = (n + 63) // 64
    full = np.zeros((n, wds * 64), dtype=bool)
    full[:, :n] = b
    if pad_garbage:
        full[:, n:] = True
    return np.packbits(full, axis=1, bitorder="little").view(np.uint64).reshape(n, wds)


def cover_dev(m, eng, words, b, drop=False, pad_garbage=False):
    import torch
    n, k = len(words), len(words[0])
    d_pool = torch.from_numpy(m.pack_oligos(words).view(np.int64)).cuda()
    d_bm = torch.from_numpy(bitmap_words(b, pad_garbage).view(np.int64)).cuda()
    d_del = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nd = eng.conflict_cover_dev(d_pool.data_ptr(), n, k, d_bm.data_ptr(), d_del.data_ptr(), drop_self_pairs=drop)
    deleted = d_del.cpu().numpy()
    assert set(np.unique(deleted).tolist()) <= {0, 1}
    assert nd == int(deleted.sum())
    return deleted.astype(bool), eng.info("cover_rounds")


def host_cover(host, words, edges):
    text = "\n".join(f"{words[a]},{words[b]}" for a, b in edges).encode()
    cap = 32 * len(words) + 64
    buf = C.create_string_buffer(cap)
    rc = host.odm_vertex_cover("\n".join(words).encode(), text, buf, cap)
    assert rc >= 0
    got = set(buf.value.decode().split())
    return np.array([w in got for w in words])


def edges(eng, words, chem, thr):
    try:
        e, _ = eng.cross_dimer_edges(words, chem, thr, capacity=1 << 22)
    except Exception as err:          # MSSPE_ERR_CAPACITY: retry with the count the call reported
        if not hasattr(err, "count"):
            raise
        e, _ = eng.cross_dimer_edges(words, chem, thr, capacity=err.count)
    return list(zip(e["a"].tolist(), e["b"].tolist()))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("name", crm.HAND_BUILT)
def test_hand_built_bitmaps_equal_the_round_model(m, eng, name, n):
    words = crm.random_words(n, 13, np.random.default_rng(1000 + n))
    b = crm.hand_built(name, n)
    want, want_rounds = crm.round_cover(crm.symmetrise(b), crm.lex_rank(words))
    got, rounds = cover_dev(m, eng, words, b, pad_garbage=(name == "one_direction"))
    np.testing.assert_array_equal(got, want)
    assert rounds == want_rounds


def test_hand_built_drop_self_pairs(m, eng):
    """drop_self_pairs on a bitmap: the diagonal and the reverse-complement partners are no edges (16-mers, so that
    palindromes exist)."""
    rng = np.random.default_rng(9)
    half = crm.random_words(40, 8, rng)
    words = distinct([h + revcomp(h) for h in half[:10]] + [w for h in half[10:25] for w in (h * 2, revcomp(h * 2))]
                     + crm.random_words(200, 16, rng))
    n = len(words)
    b = rng.random((n, n)) < 0.03
    index = {w: i for i, w in enumerate(words)}
    drop = np.zeros((n, n), dtype=bool)
    for i, w in enumerate(words):
        drop[i, i] = True
        if revcomp(w) in index:
            drop[i, index[revcomp(w)]] = True
            b[i, index[revcomp(w)]] = True       # every partner pair conflicts in the input
    np.fill_diagonal(b, True)
    want, want_rounds = crm.round_cover(crm.symmetrise(b, drop), crm.lex_rank(words))
    got, rounds = cover_dev(m, eng, words, b, drop=True)
    np.testing.assert_array_equal(got, want)
    assert rounds == want_rounds
    kept, _ = cover_dev(m, eng, words, b, drop=False)
    assert not np.array_equal(kept, got)


@pytest.mark.parametrize("n", [500, 2000, 5000])
@pytest.mark.parametrize("thr", [-9000.0, -6000.0, -12000.0])
def test_thermodynamic_pools_equal_the_host_cover(m, eng, host, n, thr):
    words = distinct(m.synth.pool_strings(m.synth.random_pool(n, 13, seed=4100 + n)))
    chem = m.Chem.ntthal()
    got = eng.conflict_cover(words, chem, thr)
    rounds = eng.info("cover_rounds")
    want = host_cover(host, words, edges(eng, words, chem, thr))
    np.testing.assert_array_equal(got, want)
    assert (rounds > 0) == bool(want.any())


def test_drop_self_pairs_on_a_seeded_pool(m, eng, host):
    """--check-self-dimers false: self-complementary 14-mers and reverse-complement pairs in the pool; the host side
    drops the edges ntthal_pair_sent() never sends (a == b or revcomp(b) == a, od-msspe/src/delta_g.rs:64-69)."""
    rng = np.random.default_rng(14)
    pals = [h + revcomp(h) for h in crm.random_words(30, 7, rng)]
    pairs = [x for w in crm.random_words(30, 14, rng) for x in (w, revcomp(w))]
    words = distinct(pals + pairs + m.synth.pool_strings(m.synth.random_pool(1500, 14, seed=77)))
    assert all(len(w) == 14 for w in words)
    chem = m.Chem.ntthal()
    es = [(a, b) for a, b in edges(eng, words, chem, -9000.0)
          if not (a == b or revcomp(words[b]) == words[a])]
    want = host_cover(host, words, es)
    got = eng.conflict_cover(words, chem, -9000.0, drop_self_pairs=True)
    np.testing.assert_array_equal(got, want)
    assert not np.array_equal(got, eng.conflict_cover(words, chem, -9000.0))


@pytest.mark.parametrize("k", [15, 16])
def test_long_oligo_pools_equal_the_host_cover(m, eng, host, k):
    """15-mers (row kernel) and 16-mers (split-table kernel) as the screen's first stage."""
    words = distinct(m.synth.pool_strings(m.synth.random_pool(2000, k, seed=500 + k)))
    chem = m.Chem.ntthal()
    want = host_cover(host, words, edges(eng, words, chem, -9000.0))
    np.testing.assert_array_equal(eng.conflict_cover(words, chem, -9000.0), want)


def test_16384_pool_equals_the_host_cover(m, eng, host):
    words = distinct(m.synth.pool_strings(m.synth.random_pool(16384, 13)))
    chem = m.Chem.ntthal()
    want = host_cover(host, words, edges(eng, words, chem, -9000.0))
    np.testing.assert_array_equal(eng.conflict_cover(words, chem, -9000.0), want)


def test_headline_pool_survivors_are_independent(m, eng):
    """bench.py's 65,536-primer headline pool (its few duplicate 13-mers removed: the graph's nodes are distinct).  The
    host cover would need the 23-million-edge list as strings and sets and is too slow to compare here; instead the
    survivors must form an independent set of S = B | B^T (checked on the device), and the host-pool call and the
    device-pointer call on the screen's own bitmap give the same output."""
    import torch
    words = distinct(m.synth.pool_strings(m.synth.random_pool(65536, 13)))
    n, chem = len(words), m.Chem.ntthal()
    first = eng.conflict_cover(words, chem, -9000.0)
    rounds = eng.info("cover_rounds")
    assert 0 < rounds < int(first.sum())
    d_pool = torch.from_numpy(m.pack_oligos(words).view(np.int64)).cuda()
    wds = (n + 63) // 64
    d_bm = torch.zeros((n, wds), dtype=torch.int64, device="cuda")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        eng.cross_dimer_dev(d_pool.data_ptr(), n, 13, chem, -9000.0, (0, n), (0, n), d_bitmap=d_bm.data_ptr())
        d_del = torch.zeros(n, dtype=torch.uint8, device="cuda")
        eng.conflict_cover_dev(d_pool.data_ptr(), n, 13, d_bm.data_ptr(), d_del.data_ptr())
        torch.cuda.synchronize()
    finally:
        eng.reset_stream()
    second = d_del.cpu().numpy().astype(bool)
    np.testing.assert_array_equal(first, second)
    assert eng.info("cover_rounds") == rounds
    bits = np.zeros(wds * 64, dtype=bool)
    bits[:n] = ~second
    surv_words = torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int64)).cuda()
    rows = torch.from_numpy(np.nonzero(~second)[0]).cuda()
    for r0 in range(0, rows.numel(), 8192):    # B restricted to the survivors' rows and columns is empty
        blk = d_bm[rows[r0:r0 + 8192]]
        assert not torch.any(torch.bitwise_and(blk, surv_words[None, :])).item()


def test_errors(m, eng):
    import torch
    chem = m.Chem.ntthal()
    words = crm.random_words(10, 13, np.random.default_rng(2))
    with pytest.raises(m.MsspeError) as e:
        eng.conflict_cover(words + [words[3]], chem, -9000.0)
    assert e.value.code == 1
    d_pool = torch.from_numpy(m.pack_oligos(words + [words[3]]).view(np.int64)).cuda()
    d_bm = torch.zeros((11, 1), dtype=torch.int64, device="cuda")
    d_del = torch.zeros(11, dtype=torch.uint8, device="cuda")
    with pytest.raises(m.MsspeError) as e:
        eng.conflict_cover_dev(d_pool.data_ptr(), 11, 13, d_bm.data_ptr(), d_del.data_ptr())
    assert e.value.code == 1 and "duplicate" in str(e.value)
    with pytest.raises(m.MsspeError) as e:        # the oligo-length status of the msspe_cross_dimer* siblings
        eng.conflict_cover_dev(d_pool.data_ptr(), 10, 33, d_bm.data_ptr(), d_del.data_ptr())
    assert e.value.code == 2
    with pytest.raises(m.MsspeError) as e:
        eng.conflict_cover(["A" * 33, "C" * 33], chem, -9000.0)
    assert e.value.code == 2
    with pytest.raises(m.MsspeError) as e:        # above the cap: refused before any buffer is read
        eng.conflict_cover_dev(d_pool.data_ptr(), 262145, 13, d_bm.data_ptr(), d_del.data_ptr())
    assert e.value.code == 1
    with pytest.raises(m.MsspeError) as e:
        eng.conflict_cover(["ACGTNACGTACGT", "ACGTAACGTACGT"], chem, -9000.0)
    assert e.value.code == 1
    assert eng.conflict_cover_dev(0, 0, 13, 0, 0) == 0
    assert eng.conflict_cover([], chem, -9000.0).shape == (0,)
    # the context still works after the errors
    b = crm.hand_built("star", 10)
    got, rounds = cover_dev(m, eng, words, b)
    assert got.tolist() == [True] + [False] * 9 and rounds == 1
