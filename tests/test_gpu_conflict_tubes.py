"""The conflict graph split into reaction tubes on the device (msspe_conflict_tubes*, csrc/tube_split.hip) against the
round model (tests/tube_round_model.py, itself checked against the sequential rule and the host's assign_tubes without a
GPU): tube array, tubes used, unplaced and round count on hand-built bitmaps, on rows of more than 64 words, with
drop_self_pairs, and on a thermodynamic pool, where the host's odm_assign_tubes is fed the edge list of the same
screen."""
import ctypes as C
import functools
from pathlib import Path

import numpy as np
import pytest

import tube_round_model as trm

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HOST_LIB = ROOT / "open-msspe-design_amd" / "libod_msspe_host.so"
COMP = str.maketrans("ACGT", "TGCA")
SENTINEL = 7
POOL_SEED = 4100


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


def bitmap_bool(words64, n):
    return np.unpackbits(np.ascontiguousarray(words64).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def tubes_dev(m, eng, words, b, T, drop=False, pad_garbage=False, stream=False):
    """(tube uint8[n], used, unplaced, rounds) of one msspe_conflict_tubes_dev call, the output pre-filled with 7."""
    import torch
    n, k = len(words), len(words[0])
    d_pool = torch.from_numpy(m.pack_oligos(words).view(np.int64)).cuda()
    d_bm = torch.from_numpy(bitmap_words(b, pad_garbage).view(np.int64)).cuda()
    d_tube = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if stream:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        used, unplaced = eng.conflict_tubes_dev(d_pool.data_ptr(), n, k, d_bm.data_ptr(), d_tube.data_ptr(), T,
                                                drop_self_pairs=drop)
        torch.cuda.synchronize()
    finally:
        if stream:
            eng.reset_stream()
    return d_tube.cpu().numpy(), used, unplaced, eng.info("tube_rounds")


def same_as_model(got, s, rank, T):
    tube, used, unplaced, rounds = got
    want, want_rounds = trm.rounds(s, rank, T)
    np.testing.assert_array_equal(tube, want)
    placed = want[want != trm.NONE]
    assert used == (int(placed.max()) + 1 if placed.size else 0)
    assert unplaced == int((want == trm.NONE).sum())
    assert rounds == want_rounds
    return want


@functools.lru_cache(maxsize=None)
def hand_built_case(name, n):
    words = trm.random_words(n, 13, np.random.default_rng(1000 + n))
    b = trm.hand_built(name, n)
    return words, b, trm.symmetrise(b), trm.lex_rank(words)


@pytest.mark.parametrize("T", [1, 2, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("name", trm.HAND_BUILT)
def test_hand_built_bitmaps_equal_the_round_model(m, eng, name, n, T):
    words, b, s, rank = hand_built_case(name, n)
    want = same_as_model(tubes_dev(m, eng, words, b, T, pad_garbage=(name == "one_direction")), s, rank, T)
    if name == "clique" and n == 65 and T == 64:      # the full mask: 64 tubes taken, the last node finds none
        assert int((want == trm.NONE).sum()) == 1 and eng.info("tube_rounds") == 65


@functools.lru_cache(maxsize=None)
def wide_case():
    n = 4160                                            # 65 words per row: the row walk takes a second step
    rng = np.random.default_rng(4160)
    words = trm.random_words(n, 13, rng)
    b = np.triu(rng.random((n, n)) < 8.0 / n, 1)
    idx = np.arange(n)
    b[idx[::5], idx[::5]] = True
    leaves = np.concatenate([np.arange(3, 4096, 97), np.arange(4096, n - 1, 3)])
    b[n - 1, leaves] = True                             # a star around the last node, leaves beyond word 63 included
    return words, b, trm.symmetrise(b), trm.lex_rank(words)


@pytest.mark.parametrize("T", [3, 64])
def test_rows_of_more_than_64_words(m, eng, T):
    words, b, s, rank = wide_case()
    assert s[len(words) - 1, 4096:].sum() > 10
    want = same_as_model(tubes_dev(m, eng, words, b, T, pad_garbage=True), s, rank, T)
    trm.check_assignment(s, want, T)


def test_drop_self_pairs(m, eng):
    """drop_self_pairs on a bitmap: the diagonal and the reverse-complement partners are no edges (16-mers, so that
    palindromes exist)."""
    rng = np.random.default_rng(9)
    half = trm.random_words(40, 8, rng)
    words = distinct([h + revcomp(h) for h in half[:10]] + [w for h in half[10:25] for w in (h * 2, revcomp(h * 2))]
                     + trm.random_words(200, 16, rng))
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
    rank = trm.lex_rank(words)
    for T in (2, 64):
        got = tubes_dev(m, eng, words, b, T, drop=True)
        same_as_model(got, trm.symmetrise(b, drop), rank, T)
        kept = tubes_dev(m, eng, words, b, T, drop=False)
        same_as_model(kept, trm.symmetrise(b), rank, T)
        assert not np.array_equal(kept[0], got[0])
    assert (kept[0] == trm.NONE).all()           # every node conflicts with itself without the flag


def edges(eng, words, chem, thr):
    try:
        e, _ = eng.cross_dimer_edges(words, chem, thr, capacity=1 << 22)
    except Exception as err:          # MSSPE_ERR_CAPACITY: retry with the count the call reported
        if not hasattr(err, "count"):
            raise
        e, _ = eng.cross_dimer_edges(words, chem, thr, capacity=err.count)
    return list(zip(e["a"].tolist(), e["b"].tolist()))


@pytest.fixture(scope="module")
def thermo(m, eng):
    words = distinct(m.synth.pool_strings(m.synth.random_pool(2000, 13, seed=POOL_SEED)))
    chem = m.Chem.ntthal()
    out = eng.cross_dimer(words, chem, -9000.0, want_dg=False, want_tm=False, want_bitmap=True)
    bitmap = out["bitmap"] if isinstance(out, dict) else out.bitmap
    b = bitmap_bool(np.asarray(bitmap).reshape(len(words), -1), len(words))
    return words, chem, b, edges(eng, words, chem, -9000.0)


@pytest.mark.parametrize("T", [4, 64])
def test_thermodynamic_pool(m, eng, host, thermo, T):
    words, chem, b, es = thermo
    n = len(words)
    s, rank = trm.symmetrise(b), trm.lex_rank(words)
    self_c = np.diag(s)
    tube, used, unplaced = eng.conflict_tubes(words, chem, -9000.0, T)
    same_as_model((tube, used, unplaced, eng.info("tube_rounds")), s, rank, T)
    # the host's sequential rule on the edge list of the same pool
    text = "\n".join(f"{words[a]},{words[c]}" for a, c in es).encode()
    cap = 32 * n + 64
    buf = C.create_string_buffer(cap)
    assert host.odm_assign_tubes("\n".join(words).encode(), text, T, buf, cap) >= 0
    rows = [l.split("\t") for l in buf.value.decode().splitlines()]
    assert [r[0] for r in rows] == words
    np.testing.assert_array_equal(tube, np.array([trm.NONE if r[1] == "-" else int(r[1]) for r in rows], np.uint8))
    # independently of both: no conflicting pair shares a tube
    for a, c in es:
        if a != c and tube[a] != trm.NONE:
            assert tube[a] != tube[c], (a, c)
    edge_self = np.zeros(n, dtype=bool)
    nb_tubes = [set() for _ in range(n)]
    for a, c in es:
        if a == c:
            edge_self[a] = True
        else:
            if tube[c] != trm.NONE:
                nb_tubes[a].add(int(tube[c]))
            if tube[a] != trm.NONE:
                nb_tubes[c].add(int(tube[a]))
    np.testing.assert_array_equal(edge_self, self_c)
    assert not (tube[edge_self] != trm.NONE).any()
    out = np.nonzero((tube == trm.NONE) & ~edge_self)[0]
    assert used > 1
    if T == 4:
        assert out.size > 0                     # something to assign: four tubes do not hold this pool
        for v in out:
            assert nb_tubes[v] == {0, 1, 2, 3}, v
    else:
        assert out.size == 0                    # 64 tubes leave only the self-conflicting primers out
        assert unplaced == int(edge_self.sum())


def test_one_context_callers_stream_and_the_cover_in_between(m, eng):
    """Buffers kept across calls, a smaller n after a larger one, the caller's stream, and the cover (which shares S and
    the key buffers) on the same context in between."""
    import torch
    big = hand_built_case("one_direction", 1000)
    small = hand_built_case("one_direction", 65)

    def cover(case):
        words, b = case[0], case[1]
        n = len(words)
        d_pool = torch.from_numpy(m.pack_oligos(words).view(np.int64)).cuda()
        d_bm = torch.from_numpy(bitmap_words(b).view(np.int64)).cuda()
        d_del = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        nd = eng.conflict_cover_dev(d_pool.data_ptr(), n, 13, d_bm.data_ptr(), d_del.data_ptr())
        return d_del.cpu().numpy(), nd, eng.info("cover_rounds")

    before = cover(big)
    same_as_model(tubes_dev(m, eng, big[0], big[1], 3, stream=True), big[2], big[3], 3)
    mid = cover(big)
    same_as_model(tubes_dev(m, eng, small[0], small[1], 3, stream=True), small[2], small[3], 3)
    after_small = cover(small)
    same_as_model(tubes_dev(m, eng, big[0], big[1], 64, stream=True), big[2], big[3], 64)
    after = cover(big)
    for got in (mid, after):
        np.testing.assert_array_equal(got[0], before[0])
        assert got[1:] == before[1:]
    import cover_round_model as crm
    want, want_rounds = crm.round_cover(small[2], small[3])
    np.testing.assert_array_equal(after_small[0].astype(bool), want)
    assert after_small[2] == want_rounds


def test_errors(m, eng):
    import torch
    chem = m.Chem.ntthal()
    words = trm.random_words(10, 13, np.random.default_rng(2))
    d_pool = torch.from_numpy(m.pack_oligos(words + [words[3]]).view(np.int64)).cuda()
    d_bm = torch.zeros((11, 1), dtype=torch.int64, device="cuda")
    d_tube = torch.full((11,), SENTINEL, dtype=torch.uint8, device="cuda")
    for T in (0, 65):
        with pytest.raises(m.MsspeError) as e:
            eng.conflict_tubes(words, chem, -9000.0, T)
        assert e.value.code == 1
        with pytest.raises(m.MsspeError) as e:
            eng.conflict_tubes_dev(d_pool.data_ptr(), 10, 13, d_bm.data_ptr(), d_tube.data_ptr(), T)
        assert e.value.code == 1
    with pytest.raises(m.MsspeError) as e:
        eng.conflict_tubes(words + [words[3]], chem, -9000.0, 4)
    assert e.value.code == 1
    with pytest.raises(m.MsspeError) as e:
        eng.conflict_tubes_dev(d_pool.data_ptr(), 11, 13, d_bm.data_ptr(), d_tube.data_ptr(), 4)
    assert e.value.code == 1 and "duplicate" in str(e.value)
    high = m.pack_oligos(words).copy()
    high[4] |= np.uint64(1) << np.uint64(40)          # a bit above 2 k = 26
    d_high = torch.from_numpy(high.view(np.int64)).cuda()
    with pytest.raises(m.MsspeError) as e:
        eng.conflict_tubes_dev(d_high.data_ptr(), 10, 13, d_bm.data_ptr(), d_tube.data_ptr(), 4)
    assert e.value.code == 1 and "2 k" in str(e.value)
    assert eng.conflict_tubes_dev(d_pool.data_ptr(), 0, 13, d_bm.data_ptr(), d_tube.data_ptr(), 4) == (0, 0)
    torch.cuda.synchronize()
    assert (d_tube.cpu().numpy() == SENTINEL).all()   # n == 0 and the refused calls wrote nothing
    tube, used, unplaced = eng.conflict_tubes([], chem, -9000.0, 4)
    assert tube.shape == (0,) and (used, unplaced) == (0, 0)
    # the context still works after the errors
    case = hand_built_case("star", 63)
    same_as_model(tubes_dev(m, eng, case[0], case[1], 2), case[2], case[3], 2)
